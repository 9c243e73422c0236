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
from .ndist import _open, decode_row_chunk, encode_row_chunk, read_chunk_rows, write_block_chunk

REGION_COLS = rag.REGION_COLS
FEATURE_NAMES = list(rag.REGION_FEATURE_NAMES)


def encode_region_chunk(rows):
    """(n, 5) float64 rows [id, count, sum, min, max] -> the chunk words above."""
    return encode_row_chunk(rows, REGION_COLS, 'region-feature')


def decode_region_chunk(words):
    """Chunk words -> (n, 5) float64 rows in the chunk's order."""
    return decode_row_chunk(words, REGION_COLS, 'region-feature')


def computeAndSerializeRegionFeatures(labels, data, outPath, outKey, chunkId, ignoreLabel=None):  # noqa: N802,N803
    """The region-feature rows of ``labels`` over ``data`` (one block of the
    segmentation and of the input map, float32 or uint8) as one varlen float64
    chunk of ``outKey`` at ``chunkId`` (region_features.py:159-185).  Voxels
    whose label equals ``ignoreLabel`` are not counted.  No chunk is written for
    an empty result; the dataset's ``feature_names`` and ``norm`` are set
    (region_features.py:230-232)."""
    with rag.region_features_handle(labels, data, ignore_label=ignoreLabel) as r:
        words = encode_region_chunk(r.region_rows('sums')) if r.n_nodes else None
    write_block_chunk(outPath, outKey, chunkId, words,   # (every block writes the same two values)
                      (('feature_names', FEATURE_NAMES), ('norm', rag.region_norm(data))))


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
    (rows,), attrs = read_chunk_rows(inputPath, inputKey, lambda c: (decode_region_chunk(c),), begin, end,
                                     numberOfThreads, (np.zeros((0, REGION_COLS), np.float64),))
    with rag.merge_region_features_handle(rows) as r:
        out = rag.region_feature_rows(r, begin, end, 'features', float(attrs.get('norm', 1.0)))
    with _open(outputPath) as f:
        f[outputKey][begin:end, :] = out[:, cols].astype(np.float32)
