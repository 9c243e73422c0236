"""The seeded watershed around libctg.so (rag.seeded_watershed), with the
reference's spellings --

    watershed          elf.segmentation.watershed.watershed, imported as run_watershed at
                       watershed/watershed.py:16 (watershed_from_seeds.py:160 spells it
                       vu.watershed, which utils/volume_utils.py does not define)
    apply_size_filter  elf's size filter [UPSTREAM, unverified: restated in include/ctg.h]
    watershedsNew      vigra.analysis.watershedsNew(hmap, seeds=..., out=...) with seeds
    ws_block, ws_block_masked   _ws_block / _ws_block_masked, watershed_from_seeds.py:143-204,
                       over _read_data (:128-140)

-- and the N5 I/O of the two block bodies around it.  Labels are defined by the
rule of include/ctg.h, not by vigra's execution order: every voxel gets a label
of minimal pass height, and the two differ only where labels tie in it
(DESIGN.md 0 (m)).  Seeds may be 64-bit, so the reference's ``max_id < 2^32``
assertion (:159, :194) has nothing to guard.

Not mirrored: the size filter's ``exclude`` ids, vigra's own seed generation
(seeds are required), fit_to_hmap's erosion, the DT watershed's seed detection
and filling_size_filter's job body.
"""
from __future__ import annotations

import numpy as np

from . import rag

AGGLOMERATE = ('mean', 'max', 'min')


def watershed(input_, seeds, size_filter=0):
    """elf's watershed with seeds: flood ``input_`` (float32) from ``seeds``,
    drop the labels below ``size_filter`` voxels and flood again from the rest
    -> (ws, max_id)."""
    ws, info = rag.seeded_watershed(input_, seeds, size_filter=size_filter)
    return ws, info.max_id


def apply_size_filter(segmentation, input_, size_filter):
    """elf's apply_size_filter: the labels of ``segmentation`` with fewer than
    ``size_filter`` voxels become 0 and are flooded over from the others
    -> (segmentation, max_id).  A segmentation is its own seeds: with every
    voxel seeded the first flood changes nothing, the filter and the second
    flood are the call's."""
    ws, info = rag.seeded_watershed(input_, segmentation, size_filter=size_filter)
    return ws, info.max_id


def watershedsNew(hmap, seeds, out=None):
    """vigra.analysis.watershedsNew(hmap, seeds=seeds, out=out) -> (labels,
    max_id).  ``out`` may be ``seeds`` itself (64-bit): vigra's out=labels."""
    if seeds is None:
        raise ValueError('seeds are required: vigra\'s own seed generation is not built')
    labels, info = rag.seeded_watershed(hmap, seeds, out=out)
    return labels, info.max_id


def _normalize(x):
    """vu.normalize (utils/volume_utils.py:98-105) on the device, in its
    float32 operations: a subtraction and, where the maximum is positive, a true
    division (by a tensor: torch multiplies by the reciprocal of a host scalar)."""
    x = x - x.min()
    max_val = x.max()
    if float(max_val) > 0:
        x = x / max_val
    return x


def _read_data(ds_in, input_bb, config):
    """watershed_from_seeds.py:128-140 -> a float32 CUDA tensor: the box, or
    for a 4-D input the channels [channel_begin, channel_end) normalised over
    the slab read and folded by 'mean', 'max' or 'min'."""
    import torch
    if ds_in.ndim == 4:
        channel_begin = config.get('channel_begin', 0)
        channel_end = config.get('channel_end', None)
        input_bb = (slice(channel_begin, channel_end),) + tuple(input_bb)
    raw = np.ascontiguousarray(ds_in[tuple(input_bb)])
    x = _normalize(torch.from_numpy(raw).cuda().to(torch.float32))
    if ds_in.ndim != 4:
        return x
    agglomerate = config.get('agglomerate_channels', 'mean')
    assert agglomerate in AGGLOMERATE
    if agglomerate == 'max':
        return x.amax(dim=0)
    if agglomerate == 'min':
        return x.amin(dim=0)
    # np.mean over the first axis: the channels added one after the other in float32, then one division
    acc = x[0].clone()
    for c in range(1, x.shape[0]):
        acc += x[c]
    return acc / torch.full((), x.shape[0], dtype=torch.float32, device=x.device)


def _flood_block(input_, seeds, size_filter):
    import torch
    seeds = torch.from_numpy(np.ascontiguousarray(seeds).astype(np.uint64).view(np.int64)).cuda()
    ws, _ = rag.seeded_watershed(input_.contiguous(), seeds, size_filter=size_filter)
    return ws


def ws_block(ds_in, ds_seeds, ds_out, bb, config):
    """_ws_block (watershed_from_seeds.py:143-165): flood the box ``bb`` of
    ``ds_in`` from ``ds_seeds[bb]`` into ``ds_out[bb]`` (which may be the seeds'
    dataset)."""
    input_ = _read_data(ds_in, bb, config)
    ws = _flood_block(input_, ds_seeds[bb], config.get('size_filter', 0))
    ds_out[bb] = ws.cpu().numpy().view(np.uint64)


def ws_block_masked(ds_in, ds_seeds, ds_out, mask, bb, config):
    """_ws_block_masked (watershed_from_seeds.py:168-204), as the reference does
    it: nothing for a block outside the mask; else the heights outside the mask
    are set to 1, the block is flooded, and zeros are written back there.
    Returns whether the block was written."""
    import torch
    in_mask = np.asarray(mask[bb]).astype('bool')
    if np.sum(in_mask) == 0:
        return False
    input_ = _read_data(ds_in, bb, config)
    inv_mask = torch.from_numpy(np.logical_not(in_mask)).cuda()
    input_[inv_mask] = 1
    ws = _flood_block(input_, ds_seeds[bb], config.get('size_filter', 0))
    ws[inv_mask] = 0
    ds_out[bb] = ws.cpu().numpy().view(np.uint64)
    return True
