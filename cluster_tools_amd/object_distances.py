"""Object distances (distances/object_distances.py:109-195) around libctg.so:
per object, the distance from it to every other object within ``max_distance``.
The transform runs straight on the labels of the object's (enlarged) bounding
box (CTG_EDT_SRC_EQUAL), and the per-label minimum of the distances comes from
``rag.region_features_handle`` on the same device arrays: the distances do not
leave the GPU in between.  The six face minima and the box enlargement are the
host's, as in the reference.

The reference casts the labels to uint32 first (:110); here they keep their
width, so ids of 2^32 and above stay distinct.
"""
from __future__ import annotations

import numpy as np
import torch   # with the module: the arrays of this body live on the device between the two calls

from . import rag


def _labels_and_distances(ds, bb, resolution, label_id):
    """:109-113 -> (labels, distances), both on the device."""
    labels = np.ascontiguousarray(ds[bb])
    if labels.dtype not in (np.uint64, np.int64, np.uint32, np.int32):
        labels = labels.astype(np.uint64)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(labels.dtype)
    labels = torch.from_numpy(labels.view(signed) if signed else labels).cuda()
    distances, _ = rag.distance_transform(labels, pitch=resolution, label=label_id)
    return labels, distances


def _face_distances(distances):
    """:124-130: the smallest distance on each of the six faces (low z, high z,
    low y, ...), read back face by face."""
    faces = [np.s_[0, :, :], np.s_[-1, :, :], np.s_[:, 0, :], np.s_[:, -1, :], np.s_[:, :, 0], np.s_[:, :, -1]]
    return [float(distances[face].cpu().numpy().min()) for face in faces]


def _enlarge_bb(bb, face_distances, resolution, shape, max_distance):
    """:133-153: every side whose face is nearer than max_distance moves out by
    the missing distance, in voxels of that axis, clipped to the volume."""
    enlarged = []
    for dim, b in enumerate(bb):
        start, stop = b.start, b.stop
        low, high = face_distances[2 * dim], face_distances[2 * dim + 1]
        if low < max_distance:
            start = max(start - (max_distance - low) / resolution[dim], 0)
        if high < max_distance:
            stop = min(stop + (max_distance - high) / resolution[dim], shape[dim])
        enlarged.append(slice(int(start), int(stop)))
    return tuple(enlarged)


def object_distances(label_id, ds, bb_start, bb_stop, max_distance, resolution):
    """_object_distances (:156-180): {(label_id, other): distance} for every
    other object with a larger id whose nearest voxel lies closer than
    ``max_distance`` (float32 values).  ``bb_stop`` is exclusive (the
    morphology table's maximum + 1, :221)."""
    bb = tuple(slice(int(sta), int(sto)) for sta, sto in zip(bb_start[label_id], bb_stop[label_id]))
    labels, distances = _labels_and_distances(ds, bb, resolution, label_id)
    face_distances = _face_distances(distances)
    if min(face_distances) < max_distance:
        bb = _enlarge_bb(bb, face_distances, resolution, ds.shape, max_distance)
        labels, distances = _labels_and_distances(ds, bb, resolution, label_id)
    with rag.region_features_handle(labels, distances) as r:
        ids, minima = r.nodes(), r.region_moments()[2][:, 0]
    return {(label_id, int(obj)): np.float32(d) for obj, d in zip(ids, minima)
            if obj != 0 and label_id < obj and d < max_distance}


def distances_id_chunks(blocking, block_id, ds_in, bb_start, bb_stop, max_distance, resolution):
    """_distances_id_chunks (:183-195): the distances of the labels of one id
    chunk; label 0 is the ignore label."""
    block = blocking.getBlock(block_id)
    block_distances = {}
    for label_id in range(max(block.begin[0], 1), block.end[0]):
        block_distances.update(object_distances(label_id, ds_in, bb_start, bb_stop, max_distance, resolution))
    return block_distances
