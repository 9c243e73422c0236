"""Region centers (morphology/region_centers.py:106-133) around libctg.so: per
object, the voxel of its bounding box that lies deepest inside it -- the
arg-max of the distance to the nearest voxel outside the object -- from one
``rag.distance_transform`` call on the box as read, straight on the labels
(CTG_EDT_SRC_EQUAL | CTG_EDT_TO_BACKGROUND), without the host-side mask.
"""
from __future__ import annotations

import numpy as np

from . import rag


def region_centers_for_label_range(ds_in, ds_out, bb_start, bb_stop, label_begin, label_end, ignore_label, resolution):
    """region_centers.py:106-133: the centers of the labels [label_begin,
    label_end) into ``ds_out[label_begin:label_end]`` ((n, 3) float32; a label
    without a voxel in its box, and ``ignore_label``, keep zeros).
    ``bb_start`` / ``bb_stop``: columns 5:8 / 8:11 of the morphology table, as
    the reference slices them: the stop is the table's inclusive maximum, so the
    last plane of every object on every axis is left out, as upstream
    (INTEGRATION.md)."""
    centers = np.zeros((label_end - label_begin, 3), dtype='float32')
    for label_id in range(label_begin, label_end):
        if ignore_label == label_id:
            continue
        bb = tuple(slice(int(start), int(stop)) for start, stop in zip(bb_start[label_id], bb_stop[label_id]))
        block = np.asarray(ds_in[bb])
        if block.size == 0:
            continue
        # the seeds are the voxels that are not the object: size - n_seeds object voxels
        _, info = rag.distance_transform(block, pitch=resolution, label=label_id, to_background=True)
        if info.n_seeds == block.size:           # the object has no voxel in its box (:121)
            continue
        # An object that fills its box has no background voxel.  scipy then measures to a phantom background
        # voxel at index (-1, 0, 0) of the box, and the arg-max of that is the box's last voxel: scipy's accident,
        # kept for parity.
        center = block.size - 1 if info.n_seeds == 0 else info.argmax
        center = np.unravel_index(center, block.shape)
        centers[label_id - label_begin] = [ce + b.start for ce, b in zip(center, bb)]
    ds_out[label_begin:label_end] = centers
