"""The threshold-and-watershed workflow (harness/workflow.py:
threshold_and_watershed_workflow, over cluster_tools_amd/watershed.py) end to
end on a small N5 volume of several blocks: per block the written labels equal
the oracle of tests/ws_cases.py applied to the block-normalised input and the
seeds the thresholded-components stages wrote.  Every comparison is exact."""
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import n5
from cluster_tools_amd.blocking import blocking, blocks_in_volume
from harness import workflow
from tests import ws_cases as W

pytestmark = pytest.mark.gpu

# blocks larger than a 16 x 8 x 64 tile on every axis, the volume no multiple of the block
SHAPE, BLOCK = (30, 20, 100), (20, 12, 72)
MASK_BLOCK = 5            # grid position (1, 0, 1): the mask is empty there
U64 = np.uint64


def block_slices():
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK))
    return [tuple(slice(b, e) for b, e in zip(blk.getBlock(i).begin, blk.getBlock(i).end))
            for i in blocks_in_volume(SHAPE, BLOCK)]


def normalize(x):
    """vu.normalize (utils/volume_utils.py:98-105)."""
    x = x.astype('float32')
    x -= x.min()
    max_val = x.max()
    if max_val > 0:
        x /= max_val
    return x


@pytest.fixture(scope='module')
def volume():
    """Four channels of a float32 map with basins a threshold finds, and a mask
    with holes that is empty over one block."""
    rng = np.random.default_rng(77)
    data = rng.random((4,) + SHAPE).astype(np.float32)
    mask = rng.random(SHAPE) < 0.85
    mask[block_slices()[MASK_BLOCK]] = False
    return data, mask


def run(tmp_path, name, data, mask, both, **kw):
    """The seeds the first five stages write, and the workflow's volume."""
    path = str(tmp_path / ('%s_in.n5' % name))
    with n5.File(path) as f:
        chunks = BLOCK if data.ndim == 3 else (1,) + BLOCK
        f.create_dataset('raw', shape=data.shape, chunks=chunks, dtype='float32', compression='gzip')[:] = data
        if mask is not None:
            f.create_dataset('mask', shape=SHAPE, chunks=BLOCK, dtype='uint8', compression='gzip')[:] = mask.astype(np.uint8)
    out = []
    for stage, fn in (('seeds', workflow.thresholded_components_workflow), ('ws', workflow.threshold_and_watershed_workflow)):
        os.makedirs(str(tmp_path / name / stage), exist_ok=True)
        target = str(tmp_path / ('%s_%s.n5' % (name, stage)))
        extra = dict(both) if stage == 'seeds' else dict(both, **kw)
        fn(path, 'raw', target, 'seg', 'assignments', 0.12, threshold_mode='less',
           mask_path=path if mask is not None else None, mask_key='mask', block_shape=BLOCK, connectivity=1,
           max_jobs=3, tmp_folder=str(tmp_path / name / stage), **extra)
        with n5.File(target, 'r') as f:
            out.append(f['seg'][:])
    return out


def check_blocks(heights_of, seeds, got, mask=None):
    """heights_of(bb): the reference's input_ of a block, before the mask."""
    n_seeded = 0
    for b, bb in enumerate(block_slices()):
        if mask is not None and not mask[bb].any():
            assert_array_equal(got[bb], seeds[bb])            # not written: what the seeds' dataset held
            assert b == MASK_BLOCK
            continue
        h = heights_of(bb)
        if mask is not None:
            h[~mask[bb]] = 1
        want = W.oracle_fast(h, seeds[bb])
        if mask is not None:
            want[~mask[bb]] = 0
        assert_array_equal(got[bb], want, err_msg='block %d' % b)
        if seeds[bb].any():
            n_seeded += 1
            inside = got[bb] if mask is None else got[bb][mask[bb]]
            assert inside.all()                                # no 0 remains where the block holds a seed
        else:
            assert not got[bb].any()
    return n_seeded


def test_three_d_input(gpu, tmp_path, volume):
    data, _ = volume
    seeds, got = run(tmp_path, 'plain', data[0], None, {})
    assert W.n_segments(seeds) >= 50
    assert check_blocks(lambda bb: normalize(data[0][bb]), seeds, got) == 8
    assert (got != seeds).sum() > got.size // 2               # the flood moved


def test_with_a_mask(gpu, tmp_path, volume):
    data, mask = volume
    seeds, got = run(tmp_path, 'masked', data[0], mask, {})
    assert not seeds[~mask].any()
    assert check_blocks(lambda bb: normalize(data[0][bb]), seeds, got, mask) == 7
    assert not got[~mask].any()


@pytest.mark.parametrize('agglomerate', ['mean', 'max', 'min'])
def test_four_d_input_with_a_channel_range(gpu, tmp_path, volume, agglomerate):
    """The components come from one channel; the watershed reads the channels
    [1, 4), normalised over the slab, and folds them (watershed_from_seeds.py:130-137)."""
    data, _ = volume
    seeds, got = run(tmp_path, 'chan_' + agglomerate, data, None, dict(channel=1),
                     channel_begin=1, channel_end=4, agglomerate_channels=agglomerate)

    def heights_of(bb):
        return getattr(np, agglomerate)(normalize(data[(slice(1, 4),) + bb]), axis=0)
    assert check_blocks(heights_of, seeds, got) == 8


def test_size_filter_reaches_the_blocks(gpu, tmp_path, volume):
    data, _ = volume
    seeds, got = run(tmp_path, 'sized', data[0], None, {}, size_filter=40)
    dropped = 0
    for bb in block_slices():
        want, info = W.oracle(normalize(data[0][bb]), seeds[bb], 40)
        assert_array_equal(got[bb], want)
        dropped += info[2]
    assert dropped > 0
