"""Thresholded components (ThresholdedComponentsWorkflow) around libctg.so:
the array work of the job bodies of the reference's ``thresholded_components``
package --

    block_components   _cc_block / _cc_block_with_mask, block_components.py:143-233
    merge_offsets      merge_offsets.py:106-122
    block_faces        _process_face / _process_faces, block_faces.py:87-137, with
                       vu.iterate_faces and get_face (utils/volume_utils.py:187-236)
    merge_assignments  merge_assignments.py:115-132

-- on the GPU (rag.threshold_components, rag.merge_assignments,
rag.unique_pairs) with the N5 I/O around it.  The last link of the chain is
``write`` with the offsets file (write.write_block(..., offset=)).

Not mirrored: resized masks (load_mask's ResizedVolume: the mask must have the
volume's shape) and label-multiset input.  merge_assignments returns the
consecutive table the reference computes and then does not save
(merge_assignments.py:131 assigns it to a misspelt name); DESIGN.md 0 (k).
"""
from __future__ import annotations

import numpy as np

from . import fastfilters, rag


def _normalize(x):
    """vu.normalize (utils/volume_utils.py:98-105)."""
    x = x.astype('float32')
    x -= x.min()
    max_val = x.max()
    if max_val > 0:
        x /= max_val
    return x


def _read_input(ds_in, bb, channel):
    """The block's samples (block_components.py:150-159): the box itself, one
    channel's box, or the mean over a channel list -> (array, prepared): a
    prepared array is float64 host data that still goes through normalize."""
    if channel is None:
        return ds_in[bb], False
    if isinstance(channel, int):                                   # the mean of one channel is the channel
        return np.asarray(ds_in[(slice(channel, channel + 1),) + bb]).squeeze(axis=0), False
    shape = (len(channel),) + tuple(b.stop - b.start for b in bb)
    input_ = np.zeros(shape, dtype=ds_in.dtype)
    for chan_id, chan in enumerate(channel):
        input_[chan_id] = np.asarray(ds_in[(slice(chan, chan + 1),) + bb]).squeeze(axis=0)
    return np.mean(input_, axis=0), True


def block_components(ds_in, ds_out, bb, threshold, threshold_mode, mask=None, channel=None, sigma=0,
                     connectivity=3):
    """One block of the job (block_components.py:143-233): threshold
    ``ds_in[bb]`` (normalised over the block, :161), label the components and
    write them to ``ds_out[bb]``.  Returns the block's offset contribution: 0,
    with nothing written, for a block whose mask is empty (:194-197) or that has
    no foreground (:175-177, :226-228), else the largest label + 1 (:182).
    ``mask``: None or a dataset / array of the volume's shape.  ``connectivity``
    3 is skimage.morphology.label's on a boolean array (:179)."""
    if threshold_mode not in rag.CC_MODES:
        raise RuntimeError('Thresholding Mode %s not supported' % threshold_mode)      # :173
    in_mask = None
    if mask is not None:
        in_mask = np.asarray(mask[bb]).astype('bool')                                  # :194
        if in_mask.sum() == 0:
            return 0
    input_, prepared = _read_input(ds_in, bb, channel)
    if prepared or sigma > 0 or input_.dtype not in (np.float32, np.uint8):
        # the host does what the kernel's two operations cannot: the float64 mean of
        # a channel list (:159), other sample types, the smoothing between two
        # normalisations (:161-164).  The call's own normalisation then repeats the
        # last one on values that are already in [0, 1].
        input_ = _normalize(np.asarray(input_))
        if sigma > 0:
            input_ = fastfilters.gaussianSmoothing(input_, sigma)
    labels, n = rag.threshold_components(input_, threshold, threshold_mode, mask=in_mask, normalize=True,
                                         connectivity=connectivity)
    if n == 0:
        return 0
    ds_out[bb] = labels
    return n + 1


def merge_offsets(per_block):
    """merge_offsets.py:106-122: {block id: offset contribution} of every block
    -> dict(offsets = the exclusive running sum by block id, empty_blocks = the
    ids that contributed 0, n_labels = the sum + 1)."""
    blocks = list(map(int, per_block.keys()))
    offset_list = list(per_block.values())
    key_sort = np.argsort(blocks)
    offset_list = np.array([offset_list[k] for k in key_sort], dtype='uint64')
    if offset_list.size == 0:
        return dict(offsets=[], empty_blocks=[], n_labels=1)
    last_offset = offset_list[-1]
    empty_blocks = np.where(offset_list == 0)[0].tolist()
    offset_list = np.roll(offset_list, 1)
    offset_list[0] = 0
    offset_list = np.cumsum(offset_list).tolist()
    n_labels = int(offset_list[-1] + last_offset + 1)
    return dict(offsets=[int(o) for o in offset_list], empty_blocks=[int(b) for b in empty_blocks], n_labels=n_labels)


def block_faces(ds, blocking, block_id, offsets, empty_blocks):
    """_process_faces (block_faces.py:116-137): the sorted unique (a, b) id
    pairs over the faces between block ``block_id`` and its upper neighbour on
    each axis (vu.iterate_faces with return_only_lower: direction False names
    the neighbour past the block's end), or None.  A pair joins the two voxels
    opposite each other across the face where both are nonzero, each id shifted
    by its block's offset (:99-109)."""
    if block_id in empty_blocks:
        return None
    block_a = blocking.getBlock(block_id)
    parts = []
    for axis in range(3):
        ngb_id = blocking.getNeighborId(block_id, axis, False)
        if ngb_id == -1 or ngb_id in empty_blocks:
            continue
        # the two planes on either side of the face (get_face, halo 1)
        face = tuple(slice(beg, end) if dim != axis else slice(end - 1, end + 1)
                     for dim, (beg, end) in enumerate(zip(block_a.begin, block_a.end)))
        seg = np.asarray(ds[face])
        labels_a = np.take(seg, 0, axis=axis).astype(np.uint64)
        labels_b = np.take(seg, 1, axis=axis).astype(np.uint64)
        have_labels = np.logical_and(labels_a != 0, labels_b != 0)
        if not have_labels.any():
            continue
        labels_a = labels_a[have_labels] + np.uint64(offsets[block_id])
        labels_b = labels_b[have_labels] + np.uint64(offsets[ngb_id])
        parts.append(np.stack([labels_a, labels_b], axis=1))
    if not parts:
        return None
    return rag.unique_pairs(np.concatenate(parts, axis=0))[0]


def merge_assignments(pair_arrays, n_labels):
    """merge_assignments.py:115-132: the jobs' pair arrays (None or empty ones
    skipped) concatenated and made unique, then the union-find over
    0 .. n_labels - 1 -> the consecutive table.  No pairs: the identity."""
    parts = [np.asarray(p, dtype=np.uint64).reshape(-1, 2) for p in pair_arrays if p is not None and len(p)]
    if parts:
        pairs = rag.unique_pairs(np.concatenate(parts, axis=0))[0]
        if int(pairs.max()) + 1 > n_labels:                                             # :127
            raise ValueError('%d, %d' % (int(pairs.max()) + 1, n_labels))
    else:
        pairs = np.zeros((0, 2), dtype=np.uint64)
    return rag.merge_assignments(pairs, n_labels)[0]
