"""Region features (RegionFeaturesWorkflow) around libctg.so: the array work of
the two job bodies of the reference's ``features`` package that are not
``nifty.distributed`` calls,

    computeAndSerializeRegionFeatures  _block_features, features/region_features.py:159-185
                                       (np.unique, the dict relabelling,
                                       vigra.analysis.extractRegionFeatures, write_chunk)
    mergeAndSerializeRegionFeatures    _extract_and_merge_region_features,
                                       features/merge_region_features.py:109-158

on the GPU (rag.region_features_handle, rag.merge_region_features_handle) with
the N5 I/O around them.

A block chunk (varlen float64, written by the first, read by the second) holds
the block's rows in the sum form

    id, count, sum, min, max

one after the other, ids ascending; the samples enter as they are (uint8 as its
integer value), and the dataset's attribute ``norm`` (255 for uint8 input, 1
otherwise: region_features.py:151-157) is applied once, after the merge.  The
reference's chunk is float32 ``id, count, mean``: it cannot hold an id or a
count above 2^24 and stores a mean where the merge needs a sum.  Both functions
that touch these chunks are mirrored here, so the layout is this library's
(DESIGN.md 4).  The merged dataset is the reference's: (n_labels, n_features)
float32, columns in ``feature_names`` order.
"""
from __future__ import annotations

import numpy as np

from . import rag
from .ndist import _grid_positions, _open

REGION_COLS = rag.REGION_COLS
FEATURE_NAMES = list(rag.REGION_FEATURE_NAMES)


def encode_region_chunk(rows):
    """(n, 5) float64 rows [id, count, sum, min, max] -> the chunk words above."""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.size % REGION_COLS or (rows.ndim == 2 and rows.size and rows.shape[1] != REGION_COLS):
        raise ValueError('region-feature rows have %d columns, got shape %s' % (REGION_COLS, rows.shape))
    return np.ascontiguousarray(rows).reshape(-1)


def decode_region_chunk(words):
    """Chunk words -> (n, 5) float64 rows in the chunk's order."""
    w = np.asarray(words, dtype=np.float64).reshape(-1)
    if w.size % REGION_COLS:
        raise RuntimeError('region-feature chunk: truncated row (%d words, not a multiple of %d)'
                           % (w.size, REGION_COLS))
    return w.reshape(-1, REGION_COLS)


def computeAndSerializeRegionFeatures(labels, data, outPath, outKey, chunkId, ignoreLabel=None):  # noqa: N802,N803
    """The region-feature rows of ``labels`` over ``data`` (one block of the
    segmentation and of the input map, float32 or uint8) as one varlen float64
    chunk of ``outKey`` at ``chunkId`` (region_features.py:159-185).  Voxels
    whose label equals ``ignoreLabel`` are not counted.  No chunk is written for
    an empty result; the dataset's ``feature_names`` and ``norm`` are set
    (region_features.py:230-232)."""
    norm = 255.0 if str(data.dtype).endswith('uint8') else 1.0
    r = rag.region_features_handle(labels, data, ignore_label=ignoreLabel)
    try:
        words = encode_region_chunk(r.region_rows('sums')) if r.n_nodes else None
    finally:
        r.free()
    with _open(outPath) as f:
        ds = f[outKey]
        if words is not None:
            ds.write_chunk([int(c) for c in chunkId], words, True)
        if ds.attrs.get('feature_names') != FEATURE_NAMES:   # (every block writes the same two values)
            ds.attrs['feature_names'] = FEATURE_NAMES
        if ds.attrs.get('norm') != norm:
            ds.attrs['norm'] = norm


def mergeAndSerializeRegionFeatures(inputPath, inputKey, outputPath, outputKey, labelBegin, labelEnd,  # noqa: N802,N803
                                    featureNames=('count', 'mean'), numberOfThreads=1):  # noqa: N803
    """Merge the block chunks of ``inputKey`` for the labels in [labelBegin,
    labelEnd) (merge_region_features.py:109-158) on the GPU -- counts and sums
    add, min and max fold, one division at the end -- and write
    ``out[labelBegin:labelEnd, :]`` as float32, one column per name of
    ``featureNames`` (of 'count', 'mean', 'minimum', 'maximum').  Labels without
    a row get a row of zeros (merge_region_features.py:157)."""
    begin, end = int(labelBegin), int(labelEnd)
    cols = []
    for name in featureNames:
        if name not in FEATURE_NAMES:
            raise ValueError('Invalid feature name %s' % name)   # merge_region_features.py:106
        cols.append(1 + FEATURE_NAMES.index(name))
    with _open(inputPath, 'r') as f:
        ds = f[inputKey]
        norm = float(ds.attrs['norm']) if 'norm' in ds.attrs else 1.0
        chunks = ds.read_chunks(_grid_positions(ds), numberOfThreads)
    parts = []
    for c in chunks:
        if c is None or not len(c):
            continue
        rows = decode_region_chunk(c)
        sel = (rows[:, 0] >= begin) & (rows[:, 0] < end)
        if sel.any():
            parts.append(rows[sel])
    rows = np.concatenate(parts) if parts else np.zeros((0, REGION_COLS), np.float64)
    r = rag.merge_region_features_handle(rows)
    try:
        out = rag.region_feature_rows(r, begin, end, 'features', norm)
    finally:
        r.free()
    with _open(outputPath) as f:
        f[outputKey][begin:end, :] = out[:, cols].astype(np.float32)
