"""Write (WriteWorkflow) around libctg.so: the array work of the job body of
the reference's ``write/write.py`` -- every segmentation workflow's last task,
which replaces each fragment id of a volume by its segment id --

    load_assignments   _load_assignments, write/write.py:249-278
    write_block        _write_block / _write_block_with_offsets with
                       _apply_node_labels, write/write.py:158-241
    write_max_id       _write_maxlabel, write/write.py:281-289

on the GPU (rag.assignment_dense / assignment_sparse, rag.apply_assignment) with
the N5 I/O around it.  The assignment is uploaded once per job and reused for
every block; where the reference builds a dict per block from np.unique of the
block (write.py:170-181), the whole table sits in device memory as a hash table.

Not mirrored: label-multiset input (LabelMultisetWrapper) and the 2-D array
branch of _apply_node_labels (write.py:178-179), which _load_assignments never
reaches: it turns every 2-D table into a dict.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from . import rag
from .ndist import _open


def load_assignments(path, key=None, n_threads=1):
    """The node assignment at ``path`` as a device-resident ``rag.Assignment``
    (write.py:249-278): without ``key`` a pickled dict (sparse); with it a
    dataset -- 1-D: the dense table A(l) = ds[l]; (n, 2) or (2, n): (key,
    value) pairs (sparse)."""
    if key is None:
        if os.path.split(path)[1].split('.')[-1] != 'pkl':
            raise ValueError('Assignments need to be pickled map if no key is given')   # write.py:98-100, :252
        with open(path, 'rb') as f:
            node_labels = pickle.load(f)
        if not isinstance(node_labels, dict):
            raise TypeError('the pickled assignment must be a dict, got %s' % type(node_labels).__name__)
        n = len(node_labels)
        keys = np.fromiter(node_labels.keys(), dtype=np.uint64, count=n)
        values = np.fromiter(node_labels.values(), dtype=np.uint64, count=n)
        return rag.assignment_sparse(keys, values)
    with _open(path, 'r') as f:
        ds = f[key]
        if ds.ndim not in (1, 2):
            raise ValueError('node labels must be 1-D or 2-D, got %d-D' % ds.ndim)
        ds.n_threads = n_threads
        node_labels = np.asarray(ds[:])
    if node_labels.ndim == 0:                       # a single label (write.py:263-266)
        node_labels = node_labels.reshape(1)
    if node_labels.ndim == 1:
        return rag.assignment_dense(node_labels)
    if node_labels.shape[1] == 2:                   # (a (2, 2) table reads as rows of pairs, as in write.py:271-274)
        return rag.assignment_sparse(node_labels[:, 0], node_labels[:, 1])
    if node_labels.shape[0] == 2:
        return rag.assignment_sparse(node_labels[0, :], node_labels[1, :])
    raise ValueError('Invalid shape for 2d node labels')


def write_block(ds_in, ds_out, bb, assignment, offset=None, allow_empty_assignments=False):
    """One block of the job (write.py:187-241): read ``ds_in[bb]``, shift its
    nonzero ids by ``offset`` (the block's entry of the offsets file, or None),
    map them through ``assignment`` and write ``ds_out[bb]``.  Returns whether
    it wrote: an all-zero block writes nothing (write.py:230-232).  An id
    without an entry raises (KeyError / IndexError) before anything is written
    unless ``allow_empty_assignments`` (sparse assignments: such ids stay)."""
    seg = ds_in[bb]
    out, info = rag.apply_assignment(assignment, seg, offset=int(offset or 0),
                                     allow_missing=bool(allow_empty_assignments))
    if int(info['nonzero'][0]) == 0:
        return False
    ds_out[bb] = out
    return True


def write_max_id(ds, assignment):
    """``maxId`` of the output dataset: the largest value of the assignment
    (write.py:281-289), folded once when it was uploaded."""
    ds.attrs['maxId'] = int(assignment.max_value)
