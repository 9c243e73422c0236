"""Mirror of the ``nifty.tools`` names the task bodies call: ``blocking``
(cluster_tools_amd/blocking.py) and the two relabelling functions ``take``
(write/write.py:166) and ``takeDict`` (write/write.py:181,
multicut/solve_subproblems.py:175, multicut/sub_solutions.py:208,
watershed/two_pass_assignments.py:129, features/region_features.py:131, ...),
which run on the GPU through cluster_tools_amd.rag.apply_assignment.

Where a job relabels many blocks with one table, upload it once
(rag.assignment_dense / rag.assignment_sparse) and call rag.apply_assignment
per block instead, as cluster_tools_amd/write.py does: these two functions
upload their table on every call.
"""
from __future__ import annotations

import numpy as np

from . import rag
from .blocking import blocking   # noqa: F401  (nifty.tools.blocking)


def _labels(toRelabel):
    x = np.asarray(toRelabel)
    if x.dtype.kind not in 'ui':
        raise TypeError('toRelabel must hold integer labels, got %s' % x.dtype)
    if x.dtype.kind == 'i' and x.size and int(x.min()) < 0:
        raise ValueError('toRelabel holds negative labels')
    return x


def _fits(max_value, dtype, what):
    if max_value > int(np.iinfo(dtype).max):
        raise OverflowError('%s %d does not fit the result dtype %s' % (what, max_value, np.dtype(dtype)))


def take(relabeling, toRelabel):
    """``nifty.tools.take``: relabeling[toRelabel], of the shape of
    ``toRelabel`` and the dtype of ``relabeling``.  ``relabeling`` is a 1-D
    integer table; a label of len(relabeling) or more raises IndexError."""
    table = np.asarray(relabeling)
    if table.ndim != 1:
        raise ValueError('relabeling must be 1-D, got shape %s' % (table.shape,))
    if table.dtype.kind not in 'ui':
        raise TypeError('relabeling must hold integers, got %s' % table.dtype)
    if table.dtype.kind == 'i' and table.size and int(table.min()) < 0:
        raise OverflowError('relabeling holds negative values: they do not fit the uint64 table')
    x = _labels(toRelabel)
    with rag.assignment_dense(table.astype(np.uint64, copy=False)) as a:
        out, _ = rag.apply_assignment(a, x)
    return out.reshape(x.shape).astype(table.dtype, copy=False)   # (values of the table: they fit its dtype)


def takeDict(relabeling, toRelabel):
    """``nifty.tools.takeDict``: the dict ``relabeling`` applied to every
    element of ``toRelabel``, of its shape and dtype.  A label that is no key
    raises KeyError; a value that does not fit the dtype of ``toRelabel`` raises
    OverflowError (the reference truncates it, write/write.py:180)."""
    if not hasattr(relabeling, 'keys') or not hasattr(relabeling, 'values'):
        raise TypeError('relabeling must be a dict, got %s' % type(relabeling).__name__)
    x = _labels(toRelabel)
    n = len(relabeling)
    try:
        keys = np.fromiter(relabeling.keys(), dtype=np.uint64, count=n)
        values = np.fromiter(relabeling.values(), dtype=np.uint64, count=n)
    except (OverflowError, ValueError, TypeError):
        raise OverflowError('the keys and values of relabeling must be integers in [0, 2^64)') from None
    if n:
        _fits(int(values.max()), x.dtype, 'the value')
    with rag.assignment_sparse(keys, values) as a:
        out, _ = rag.apply_assignment(a, x)
    return out.reshape(x.shape).astype(x.dtype, copy=False)
