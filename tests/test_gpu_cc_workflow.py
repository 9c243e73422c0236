"""The thresholded-components workflow (harness/workflow.py:
thresholded_components_workflow, over cluster_tools_amd/thresholded_components.py)
end to end on a small N5 volume, against the oracle of tests/cc_cases.py: per
block labels, the offsets file, the face pairs, a dict union-find and the
written volume.  Integers only: every comparison is exact."""
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import n5
from cluster_tools_amd.blocking import blocking, blocks_in_volume
from cluster_tools_amd.thresholded_components import merge_offsets
from harness import workflow
from tests import cc_cases as C

pytestmark = pytest.mark.gpu

SHAPE, BLOCK = (20, 24, 70), (8, 16, 32)
ZERO_BLOCK = 4            # grid position (0, 1, 1): constant samples, no foreground above a threshold
MASK_BLOCK = 10           # grid position (1, 1, 1): the mask is empty there
U64 = np.uint64


def block_slices():
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK))
    return [tuple(slice(b, e) for b, e in zip(blk.getBlock(i).begin, blk.getBlock(i).end))
            for i in blocks_in_volume(SHAPE, BLOCK)]


@pytest.fixture(scope='module')
def volume():
    """A float32 map in steps of 1/16 (so `equal` finds voxels), one block
    constant; the mask with holes, empty over another block."""
    rng = np.random.default_rng(31)
    data = (np.round(rng.random(SHAPE) * 16) / 16).astype(np.float32)
    bbs = block_slices()
    data[bbs[ZERO_BLOCK]] = np.float32(0.25)
    mask = rng.random(SHAPE) < 0.85
    mask[bbs[MASK_BLOCK]] = False
    return data, mask


def expected(data, mask, threshold, mode, c):
    """The oracle's rendering of the workflow: per block the foreground of the
    block-normalised samples and its labels, the offsets, the pairs across the
    lower faces and the union-find -> (per-block n, offsets dict, table, volume,
    whole foreground)."""
    bbs = block_slices()
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK))
    local = np.zeros(SHAPE, dtype=U64)
    fg_all = np.zeros(SHAPE, dtype=bool)
    per_block = {}
    for b, bb in enumerate(bbs):
        if mask is not None and not mask[bb].any():
            per_block[b] = 0
            continue
        fg = C.foreground(data[bb], threshold, mode, True, None if mask is None else mask[bb])
        labels, n = C.oracle_label(fg, c)
        per_block[b] = n + 1 if n else 0
        local[bb] = labels
        fg_all[bb] = fg
    off = merge_offsets(per_block)
    glob = np.zeros(SHAPE, dtype=U64)
    for b, bb in enumerate(bbs):
        glob[bb] = np.where(local[bb] != 0, local[bb] + U64(off['offsets'][b]), U64(0))
    pairs = []
    for b in range(len(bbs)):
        for axis in range(3):
            ngb = blk.getNeighborId(b, axis, False)
            if ngb == -1:
                continue
            end = blk.getBlock(b).end[axis]
            lo = tuple(slice(end - 1, end) if d == axis else s for d, s in enumerate(bbs[b]))
            hi = tuple(slice(end, end + 1) if d == axis else s for d, s in enumerate(bbs[b]))
            a, bb_ = glob[lo].ravel(), glob[hi].ravel()
            both = (a != 0) & (bb_ != 0)
            pairs.extend(zip(a[both].tolist(), bb_[both].tolist()))
    table, _ = C.merge_table(np.array(pairs, dtype=np.int64).reshape(-1, 2), off['n_labels'])
    return per_block, off, table, table[glob], fg_all


def run(tmp_path, data, mask, threshold, mode, c, max_jobs=3, name='cc'):
    path, out = str(tmp_path / ('%s_in.n5' % name)), str(tmp_path / ('%s_out.n5' % name))
    with n5.File(path) as f:
        f.create_dataset('raw', shape=SHAPE, chunks=BLOCK, dtype=str(data.dtype), compression='gzip')[:] = data
        if mask is not None:
            f.create_dataset('mask', shape=SHAPE, chunks=BLOCK, dtype='uint8', compression='gzip')[:] = mask.astype(np.uint8)
    os.makedirs(str(tmp_path / name), exist_ok=True)
    workflow.thresholded_components_workflow(path, 'raw', out, 'cc', 'assignments', threshold, threshold_mode=mode,
                                             mask_path=path if mask is not None else None, mask_key='mask',
                                             block_shape=BLOCK, connectivity=c, max_jobs=max_jobs,
                                             tmp_folder=str(tmp_path / name))
    with open(str(tmp_path / name / 'cc_offsets.json')) as f:
        offsets = json.load(f)
    with n5.File(out, 'r') as f:
        return f['cc'][:], f['cc'], f['assignments'][:], offsets


def block_chunks_exist(ds, b):
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK)).getBlock(b)
    grid = [range(lo // ch, -(-hi // ch)) for lo, hi, ch in zip(blk.begin, blk.end, ds.chunks)]
    return [ds.chunk_exists([i, j, k]) for i in grid[0] for j in grid[1] for k in grid[2]]


def check_run(got, ds, table, offsets, want):
    per_block, off, want_table, want_vol, _ = want
    assert offsets == off                                        # cc_offsets.json = merge_offsets of the oracle's maxima
    # the reference's own property (test/thresholded_components.py:124-136): labels per block = offset differences
    steps = np.diff(np.array(off['offsets'] + [off['n_labels'] - 1]))
    assert_array_equal(steps, [per_block[b] for b in range(len(per_block))])
    assert_array_equal(table, want_table)                        # the consecutive table
    assert_array_equal(got, want_vol)
    # maxId is the table's largest entry: one id per component of the result, and one per
    # id of 1 .. n_labels - 1 that no block uses (each nonempty block leaves the one after its last)
    n_components = len(np.unique(got[got != 0]))
    unused = sum(1 for b in per_block if per_block[b])
    assert ds.attrs['maxId'] == int(table.max()) == n_components + unused
    for b in off['empty_blocks']:
        assert not any(block_chunks_exist(ds, b))                # no chunk is written for an empty block
    assert tuple(ds.chunks) == (4, 8, 16)                        # half a block (block_components.py:80)


def test_connectivity_1_equals_the_whole_volume_labelling(gpu, tmp_path, volume):
    """With c = 1 the face rule loses nothing: the result is the labelling of the
    whole foreground, exactly, once both are renumbered by first occurrence."""
    data, mask = volume
    want = expected(data, mask, 0.7, 'greater', 1)
    assert set(want[1]['empty_blocks']) == {ZERO_BLOCK, MASK_BLOCK}
    got, ds, table, offsets = run(tmp_path, data, mask, 0.7, 'greater', 1)
    check_run(got, ds, table, offsets, want)
    whole, n = C.oracle_label(want[4], 1)
    assert n >= 20
    assert_array_equal(C.first_occurrence(got), whole)
    assert len(np.unique(got[got != 0])) == n


def test_connectivity_3_equals_the_hybrid_labelling(gpu, tmp_path, volume):
    """With c = 3 blocks are 26-connected inside and joined through opposite face
    voxels only (the reference's rule): per-block labels, face pairs, union-find."""
    data, mask = volume
    want = expected(data, mask, 0.8, 'greater', 3)
    got, ds, table, offsets = run(tmp_path, data, mask, 0.8, 'greater', 3, max_jobs=2)
    check_run(got, ds, table, offsets, want)
    assert len(np.unique(got[got != 0])) >= 20
    # ... which is coarser than c = 1 and no coarser than the whole volume's 26-connected labelling
    whole, n = C.oracle_label(want[4], 3)
    assert len(np.unique(got[got != 0])) >= n
    ids = np.unique(np.stack([got[want[4]], whole[want[4]]], 1), axis=0)
    assert len(np.unique(ids[:, 0])) == len(ids)                 # every written component lies in one true component


@pytest.mark.parametrize('mode,threshold', [('less', 0.3), ('equal', 0.0)])
def test_modes(gpu, tmp_path, volume, mode, threshold):
    data, _ = volume
    want = expected(data, None, threshold, mode, 3)
    got, ds, table, offsets = run(tmp_path, data, None, threshold, mode, 3, max_jobs=1)
    check_run(got, ds, table, offsets, want)
    assert (got != 0).any()


def test_uint8_input_with_mask(gpu, tmp_path, volume):
    data, mask = volume
    data = np.round(data * 12).astype(np.uint8)
    want = expected(data, mask, 0.6, 'greater', 1)
    got, ds, table, offsets = run(tmp_path, data, mask, 0.6, 'greater', 1, max_jobs=4)
    check_run(got, ds, table, offsets, want)
    whole, n = C.oracle_label(want[4], 1)
    assert_array_equal(C.first_occurrence(got), whole)


def test_no_foreground_at_all(gpu, tmp_path):
    data = np.full(SHAPE, 0.5, dtype=np.float32)
    got, ds, table, offsets = run(tmp_path, data, None, 0.5, 'greater', 3)
    assert not got.any() and table.tolist() == [0] and ds.attrs['maxId'] == 0
    assert offsets == dict(offsets=[0] * 18, empty_blocks=list(range(18)), n_labels=1)
