"""The write and relabel workflows (harness/workflow.py: write_workflow,
relabel_workflow, over cluster_tools_amd/write.py) end to end on a small N5
volume, against numpy: the fragment volume mapped through the assignment, block
by block.  Integers only: every comparison is exact."""
import json
import pickle

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import n5
from cluster_tools_amd.blocking import blocking, blocks_in_volume
from harness import workflow

pytestmark = pytest.mark.gpu

SHAPE, BLOCK = (20, 24, 70), (8, 16, 32)
N_IDS = 400
ZERO_BLOCK = 4            # grid position (0, 1, 1): made all zero


@pytest.fixture(scope='module')
def volume():
    """Fragments in cells of 3 x 4 x 5 voxels with ids 1 .. N_IDS - 1, holes of
    zeros, one all-zero block; the dense table that merges about eight ids each."""
    z, y, x = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing='ij')
    cell = (z // 3) * 1000 + (y // 4) * 50 + x // 5
    seg = (cell * 7919 % (N_IDS - 1) + 1).astype(np.uint64)
    seg[(z + y + x) % 11 == 0] = 0
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK)).getBlock(ZERO_BLOCK)
    seg[tuple(slice(b, e) for b, e in zip(blk.begin, blk.end))] = 0
    table = (np.arange(N_IDS, dtype=np.uint64) * np.uint64(31) % np.uint64(50)) + np.uint64(1000)
    table[0] = 0
    return seg, table


def make_input(tmp_path, seg, name='in.n5'):
    path = str(tmp_path / name)
    with n5.File(path) as f:
        f.create_dataset('seg', shape=SHAPE, chunks=BLOCK, dtype='uint64', compression='gzip')[:] = seg
    return path


def read(path, key):
    with n5.File(path, 'r') as f:
        return f[key][:], f[key]


def zero_block_chunks(ds):
    """Whether any chunk file of the all-zero block exists."""
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK)).getBlock(ZERO_BLOCK)
    grid = [range(b // c, -(-e // c)) for b, e, c in zip(blk.begin, blk.end, ds.chunks)]
    return [ds.chunk_exists([i, j, k]) for i in grid[0] for j in grid[1] for k in grid[2]]


def test_write_dense(gpu, tmp_path, volume):
    seg, table = volume
    path, out = make_input(tmp_path, seg), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('table', shape=table.shape, chunks=(128,), dtype='uint64', compression='gzip')[:] = table
    workflow.write_workflow(path, 'seg', out, 'written', path, 'table', BLOCK, max_jobs=3)
    got, ds = read(out, 'written')
    assert_array_equal(got, table[seg])
    assert tuple(ds.chunks) == (4, 8, 16)                    # half a block (write.py:80-81)
    assert ds.attrs['maxId'] == int(table.max())
    assert not any(zero_block_chunks(ds))                    # the all-zero block wrote nothing


@pytest.mark.parametrize('form', ['pickle', 'n2', '2n'])
def test_write_sparse(gpu, tmp_path, volume, form):
    seg, table = volume
    path, out = make_input(tmp_path, seg), str(tmp_path / 'out.n5')
    keys = np.random.default_rng(1).permutation(N_IDS).astype(np.uint64)
    if form == 'pickle':
        apath, akey = str(tmp_path / 'assignment.pkl'), None
        with open(apath, 'wb') as f:
            pickle.dump({int(k): int(table[k]) for k in keys}, f)
    else:
        apath, akey = path, 'pairs'
        pairs = np.stack([keys, table[keys]], axis=1 if form == 'n2' else 0)
        with n5.File(path) as f:
            f.create_dataset(akey, shape=pairs.shape, chunks=pairs.shape, dtype='uint64', compression='gzip')[:] = pairs
    workflow.write_workflow(path, 'seg', out, 'written', apath, akey, BLOCK, max_jobs=2)
    got, ds = read(out, 'written')
    assert_array_equal(got, table[seg])
    assert ds.attrs['maxId'] == int(table.max())
    assert not any(zero_block_chunks(ds))


def test_write_with_offsets(gpu, tmp_path, volume):
    """Block-local ids plus the offsets JSON (offsets, empty_blocks): the table
    is indexed by id + offset of the block."""
    seg, _ = volume
    blk = blocking([0, 0, 0], list(SHAPE), list(BLOCK))
    n_blocks = len(blocks_in_volume(SHAPE, BLOCK))
    offsets = [int(b * N_IDS) for b in range(n_blocks)]
    table = (np.arange(n_blocks * N_IDS, dtype=np.uint64) * np.uint64(17)) % np.uint64(977) + np.uint64(5)
    table[0] = 0
    want = np.zeros(SHAPE, dtype=np.uint64)
    for b in range(n_blocks):
        bb = tuple(slice(x, y) for x, y in zip(blk.getBlock(b).begin, blk.getBlock(b).end))
        s = seg[bb]
        want[bb] = np.where(s != 0, table[np.where(s != 0, s + np.uint64(offsets[b]), 0)], 0)
    # a block named empty is skipped whatever it holds
    skipped = tuple(slice(x, y) for x, y in zip(blk.getBlock(1).begin, blk.getBlock(1).end))
    want[skipped] = 0
    path, out = make_input(tmp_path, seg), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('table', shape=table.shape, chunks=(4096,), dtype='uint64', compression='gzip')[:] = table
    opath = str(tmp_path / 'offsets.json')
    with open(opath, 'w') as f:
        json.dump({'offsets': offsets, 'empty_blocks': [1, ZERO_BLOCK]}, f)
    workflow.write_workflow(path, 'seg', out, 'written', path, 'table', BLOCK, offset_path=opath, max_jobs=2)
    got, _ = read(out, 'written')
    assert_array_equal(got, want)


def test_write_in_place(gpu, tmp_path, volume):
    seg, table = volume
    path, out = make_input(tmp_path, seg), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('table', shape=table.shape, chunks=(128,), dtype='uint64', compression='gzip')[:] = table
    workflow.write_workflow(path, 'seg', out, 'written', path, 'table', BLOCK)
    workflow.write_workflow(path, 'seg', path, 'seg', path, 'table', BLOCK)
    sep, _ = read(out, 'written')
    same, ds = read(path, 'seg')
    assert_array_equal(same, sep)
    assert_array_equal(same, table[seg])
    assert tuple(ds.chunks) == BLOCK and ds.attrs['maxId'] == int(table.max())     # the existing dataset's chunks


def test_write_missing_id(gpu, tmp_path, volume):
    seg, table = volume
    path, out = make_input(tmp_path, seg), str(tmp_path / 'out.n5')
    gone = int(seg[seg != 0].max())
    keys = np.array([k for k in range(N_IDS) if k != gone], dtype=np.uint64)
    apath = str(tmp_path / 'assignment.pkl')
    with open(apath, 'wb') as f:
        pickle.dump({int(k): int(table[k]) for k in keys}, f)
    with pytest.raises(KeyError, match='%d:' % gone):
        workflow.write_workflow(path, 'seg', out, 'written', apath, None, BLOCK)
    workflow.write_workflow(path, 'seg', out, 'kept', apath, None, BLOCK, allow_empty_assignments=True)
    got, _ = read(out, 'kept')
    assert_array_equal(got, np.where(seg == gone, np.uint64(gone), table[seg]))
    with n5.File(path) as f:                                 # a dense table that is too short
        f.create_dataset('short', shape=(gone,), chunks=(gone,), dtype='uint64', compression='gzip')[:] = table[:gone]
    with pytest.raises(IndexError, match='^%d:' % gone):
        workflow.write_workflow(path, 'seg', out, 'short', path, 'short', BLOCK)


@pytest.mark.parametrize('with_zero', [True, False])
def test_relabel(gpu, tmp_path, volume, with_zero):
    seg, _ = volume
    seg = seg * np.uint64(1 << 33) if with_zero else seg * np.uint64(1 << 33) + np.uint64(9)
    path = make_input(tmp_path, seg)
    workflow.relabel_workflow(path, 'seg', path, 'relabel_assignments', BLOCK, output_path=str(tmp_path / 'out.n5'),
                              output_key='relabeled', max_jobs=2)
    got, ds = read(str(tmp_path / 'out.n5'), 'relabeled')
    old = np.unique(seg)
    n = len(old) - 1 if with_zero else len(old)
    assert_array_equal(np.unique(got), np.arange(0 if with_zero else 1, n + 1, dtype=np.uint64))   # exactly 1 .. N, 0 kept
    assert_array_equal(got == 0, seg == 0)
    # the partition is the input's: old id -> new id is one to one and monotone
    assert_array_equal(got, (np.searchsorted(old, seg) + (0 if with_zero else 1)).astype(np.uint64))
    assert ds.attrs['maxId'] == n
    table, _ = read(path, 'relabel_assignments')
    assert_array_equal(table[:, 0], old)
