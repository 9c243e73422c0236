"""Label overlaps on the GPU (ctg_label_overlaps, ctg_merge_overlaps,
ctg_max_overlaps and their ndist mirror) against the numpy oracle of
tests/test_overlaps_host.py.  Everything is integers: every comparison is
exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cluster_tools_amd import _lib, n5, ndist, rag
from cluster_tools_amd import synthetic as S
from harness import workflow

from test_overlaps_host import max_overlap, overlap_table, table_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.uint64(1) << np.uint64(40)
TOP = np.uint64(1) << np.uint64(63)


def two_labellings(shape, seed=0, cell=5, coarse=11):
    """Voronoi supervoxels and a second, coarser labelling of the same box."""
    a = S.generate(shape, cell=cell, seed=seed, with_boundary=False)[0]
    b = S.generate(shape, cell=coarse, seed=seed + 100, with_boundary=False)[0]
    return a, b


def check_table(out, a, b, ignore_label=None):
    pairs, counts = overlap_table(a, b, ignore_label)
    np.testing.assert_array_equal(out['pairs'], pairs)
    np.testing.assert_array_equal(out['counts'], counts)
    np.testing.assert_array_equal(out['nodes'], np.unique(pairs[:, 0]))
    assert out['pairs'].dtype == out['counts'].dtype == out['nodes'].dtype == np.uint64
    return pairs, counts


# ------------------------------------------------------------------ the scan
def test_hand_computed_case(gpu):
    """tests/golden/overlaps_kat.json: table, arg-max, the tie of node 1 and the
    chunk words, all written by hand."""
    import json
    with open(os.path.join(ROOT, 'tests', 'golden', 'overlaps_kat.json')) as fh:
        kat = json.load(fh)
    a, b = np.array(kat['labels'], np.uint64), np.array(kat['values'], np.uint64)
    out = rag.label_overlaps(a, b)
    np.testing.assert_array_equal(out['pairs'], kat['pairs'])
    np.testing.assert_array_equal(out['counts'], kat['counts'])
    np.testing.assert_array_equal(out['nodes'], kat['nodes'])
    lab, cnt = rag.max_overlaps(out, *kat['label_range'])
    np.testing.assert_array_equal(lab, kat['max_labels'])
    np.testing.assert_array_equal(cnt, kat['max_counts'])
    np.testing.assert_array_equal(ndist.encode_overlap_chunk(out['pairs'], out['counts']), kat['chunk'])
    out = rag.label_overlaps(a, b, ignore_label=kat['ignore_label'])
    np.testing.assert_array_equal(out['pairs'], kat['pairs_ignore'])
    np.testing.assert_array_equal(out['counts'], kat['counts_ignore'])


@pytest.mark.parametrize('shape', [(5, 7, 67), (17, 9, 130), (1, 1, 1)])
def test_shapes_off_the_tile_grid(gpu, shape):
    """Off the 64 x 8 x 16 tile grid in every axis, crossing a wave in x."""
    a, b = two_labellings(shape, seed=3)
    check_table(rag.label_overlaps(a, b), a, b)


def test_sub_box(gpu):
    a, b = two_labellings((20, 21, 150), seed=4)
    begin, end = (3, 2, 5), (19, 17, 139)
    sl = tuple(slice(x, y) for x, y in zip(begin, end))
    check_table(rag.label_overlaps(a, b, begin, end), a[sl], b[sl])
    check_table(rag.label_overlaps(a, b, begin=begin), a[3:, 2:, 5:], b[3:, 2:, 5:])
    out = rag.label_overlaps(a, b, (4, 4, 4), (4, 9, 9))      # empty box
    assert out['pairs'].shape == (0, 2) and out['counts'].shape == (0,) and out['nodes'].shape == (0,)
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.label_overlaps(a, b, (0, 0, 0), (21, 21, 150))
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.label_overlaps(a, b, (5, 0, 0), (4, 21, 150))


def test_run_collapse(gpu):
    """One pair over the whole volume (every wave row is one run: count == V)
    and a pair that changes at every voxel along x (every lane a head)."""
    shape = (18, 10, 131)
    V = int(np.prod(shape))
    a = np.full(shape, 7, np.uint64)
    b = np.full(shape, 9, np.uint64)
    out = rag.label_overlaps(a, b)
    np.testing.assert_array_equal(out['pairs'], [[7, 9]])
    np.testing.assert_array_equal(out['counts'], [V])
    x = np.arange(shape[2], dtype=np.uint64)
    a2 = np.broadcast_to(x % np.uint64(2), shape).copy()
    b2 = np.broadcast_to(x % np.uint64(3), shape).copy()
    check_table(rag.label_overlaps(a2, b2), a2, b2)
    # runs of every length in one row, cut by skipped voxels
    rng = np.random.default_rng(5)
    a3 = np.repeat(rng.integers(1, 4, size=(6, 9, 40)), 4, axis=2)[:, :, :131].astype(np.uint64)
    b3 = np.repeat(rng.integers(0, 3, size=(6, 9, 70)), 2, axis=2)[:, :, :131].astype(np.uint64)
    check_table(rag.label_overlaps(a3, b3), a3, b3)
    check_table(rag.label_overlaps(a3, b3, ignore_label=0), a3, b3, 0)


PRESSURE_SHAPE = (16, 16, 128)


def test_table_pressure(gpu):
    """A distinct pair at every voxel: each 64 x 8 x 16 tile meets 8192 keys,
    2048 per step, against a 2048-entry LDS table -- the table fills (heads
    that find no slot write direct records) and is flushed after every step.
    With values = arange every voxel is its own pair, so the scan writes
    exactly one record per unique pair: records cannot exceed unique pairs for
    this input, and the two paths are asserted through their own counters.
    The excess of records over unique pairs is asserted on the periodic
    variant below, where every tile meets the same keys again after a flush."""
    V = int(np.prod(PRESSURE_SHAPE))
    a = two_labellings(PRESSURE_SHAPE, seed=6)[0]
    b = np.arange(V, dtype=np.uint64).reshape(PRESSURE_SHAPE)
    out = rag.label_overlaps(a, b)
    check_table(out, a, b)
    assert out['pairs'].shape[0] == V and out['n_records'] == V
    assert 0 < out['n_direct'] < out['n_records']          # direct records and flushed entries
    # the same 2048 keys in every step of a tile: flushed, then met again
    b = (np.arange(V, dtype=np.uint64) % np.uint64(8192)).reshape(PRESSURE_SHAPE)
    a = np.ones(PRESSURE_SHAPE, np.uint64)
    out = rag.label_overlaps(a, b)
    check_table(out, a, b)
    assert out['n_records'] > out['pairs'].shape[0] and out['n_direct'] > 0


def test_first_record_buffer_too_small():
    """A fresh process: a tiny call, then the table-pressure call, whose V
    records do not fit the first attempt's buffer (max(4096, V / 16) records);
    the scan runs again with the counted size and the table is exact."""
    code = (
        "import numpy as np\n"
        "from cluster_tools_amd import rag\n"
        "t = rag.label_overlaps(np.ones((1, 1, 2), np.uint64), np.ones((1, 1, 2), np.uint64))\n"
        "assert t['pairs'].tolist() == [[1, 1]] and t['counts'].tolist() == [2]\n"
        "shape = %r\n"
        "V = int(np.prod(shape))\n"
        "assert V > max(4096, V // 16)\n"
        "a = (np.arange(V, dtype=np.uint64) // np.uint64(37)).reshape(shape)\n"
        "b = np.arange(V, dtype=np.uint64).reshape(shape)\n"
        "out = rag.label_overlaps(a, b)\n"
        "assert (out['pairs'] == np.stack([a.ravel(), b.ravel()], 1)).all()\n"
        "assert (out['counts'] == 1).all() and out['counts'].shape == (V,)\n"
        "assert (out['nodes'] == np.unique(a)).all()\n"
        "assert out['n_records'] == V\n"
        "print('RETRY_OK')\n") % (PRESSURE_SHAPE,)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and 'RETRY_OK' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------ label ranges
@pytest.mark.parametrize('side', ['labels', 'values', 'both'])
def test_labels_above_2_32(gpu, side):
    """Labels >= 2^32 (one of them >= 2^63) take the dense relabelling of the
    side(s) that hold them; the tables come back in the original labels."""
    a, b = two_labellings((9, 11, 70), seed=7)
    if side in ('labels', 'both'):
        a = a * np.uint64(977) + BIG
        a[a == a.max()] = TOP + np.uint64(5)
    if side in ('values', 'both'):
        b = b * np.uint64(31) + BIG * np.uint64(3)
        b[b == b.min()] = TOP + np.uint64(9)
    pairs, _ = check_table(rag.label_overlaps(a, b), a, b)
    assert pairs.max() >= TOP
    # a sub-box, and an ignore label that is itself >= 2^32 (values) or absent
    ign = int(b[4, 5, 6])
    sl = (slice(1, 8), slice(2, 11), slice(3, 69))
    check_table(rag.label_overlaps(a, b, (1, 2, 3), (8, 11, 69), ignore_label=ign), a[sl], b[sl], ign)
    check_table(rag.label_overlaps(a, b, ignore_label=12345), a, b, 12345)


def test_uint32_inputs(gpu):
    a, b = two_labellings((7, 9, 80), seed=8)
    a32, b32 = a.astype(np.uint32), b.astype(np.uint32)
    for x, y in ((a32, b), (a, b32), (a32, b32)):
        check_table(rag.label_overlaps(x, y), a, b)
    # 32-bit labels with a 64-bit side past 2^32
    check_table(rag.label_overlaps(a32, b + BIG), a, b + BIG)
    # the largest 32-bit pair has the bit pattern of a free table slot
    a32[2, 3, 10:20] = 0xFFFFFFFF
    b32[2, 3, 12:30] = 0xFFFFFFFF
    pairs, _ = check_table(rag.label_overlaps(a32, b32), a32, b32)
    assert (pairs == 0xFFFFFFFF).all(axis=1).any()
    check_table(rag.label_overlaps(a32, b32, ignore_label=0xFFFFFFFF), a32, b32, 0xFFFFFFFF)
    # signed views of the same bits
    check_table(rag.label_overlaps(a.view(np.int64), b32.view(np.int32)), a, b32)


def test_ignore_label(gpu, tmp_path):
    a, b = two_labellings((10, 12, 90), seed=9)
    b[2:7, :, 20:61] = 0
    assert (b == 0).any()
    pairs, _ = check_table(rag.label_overlaps(a, b, ignore_label=0), a, b, 0)
    assert not (pairs[:, 1] == 0).any()
    pairs, _ = check_table(rag.label_overlaps(a, b), a, b)       # None: zeros are counted
    assert (pairs[:, 1] == 0).any()
    other = int(b[9, 11, 89])
    assert other != 0
    check_table(rag.label_overlaps(a, b, ignore_label=other), a, b, other)
    # the ignore label applies to the values, not to the labels
    a0 = a.copy()
    a0[:3] = 0
    pairs, _ = check_table(rag.label_overlaps(a0, b, ignore_label=0), a0, b, 0)
    assert (pairs[:, 0] == 0).any()
    # every voxel ignored: an empty table, and the mirror writes no chunk
    out = rag.label_overlaps(a, np.zeros_like(b), ignore_label=0)
    assert out['pairs'].shape == (0, 2) and out['counts'].shape == (0,) and out['nodes'].shape == (0,)
    path = str(tmp_path / 'ol.n5')
    with n5.file_reader(path) as f:
        f.require_dataset('ol', shape=a.shape, chunks=a.shape, dtype='uint64', compression='gzip')
    ndist.computeAndSerializeLabelOverlaps(a, np.zeros_like(b), path, 'ol', (0, 0, 0), withIgnoreLabel=True,
                                           ignoreLabel=0)
    with n5.file_reader(path, 'r') as f:
        assert not f['ol'].chunk_exists((0, 0, 0))
    assert ndist.deserializeOverlapChunk(path, 'ol', (0, 0, 0)) == ({}, 0)
    ndist.computeAndSerializeLabelOverlaps(a, b, path, 'ol', (0, 0, 0), withIgnoreLabel=True, ignoreLabel=0)
    got, max_node = ndist.deserializeOverlapChunk(path, 'ol', (0, 0, 0))
    assert got == table_dict(*overlap_table(a, b, 0)) and max_node == int(overlap_table(a, b, 0)[0][:, 0].max())
    # withIgnoreLabel=False: ignoreLabel has no effect
    ndist.computeAndSerializeLabelOverlaps(a, b, path, 'ol', (0, 0, 0), ignoreLabel=0)
    assert ndist.deserializeOverlapChunk(path, 'ol', (0, 0, 0))[0] == table_dict(*overlap_table(a, b))


# ------------------------------------------------------------------- merge
def test_merge_partial_tables(gpu):
    a, b = two_labellings((21, 13, 70), seed=10)
    parts = [rag.label_overlaps(a[z0:z1], b[z0:z1]) for z0, z1 in ((0, 6), (6, 15), (15, 21))]
    out = rag.merge_overlaps(np.concatenate([p['pairs'] for p in parts]),
                             np.concatenate([p['counts'] for p in parts]))
    check_table(out, a, b)
    # rows in any order
    rng = np.random.default_rng(11)
    perm = rng.permutation(sum(p['counts'].shape[0] for p in parts))
    out = rag.merge_overlaps(np.concatenate([p['pairs'] for p in parts])[perm],
                             np.concatenate([p['counts'] for p in parts])[perm])
    check_table(out, a, b)
    out = rag.merge_overlaps(np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64))
    assert out['pairs'].shape == (0, 2) and out['counts'].shape == (0,) and out['nodes'].shape == (0,)


def test_merge_counts_pass_2_32(gpu):
    pairs = np.array([[4, 2], [1, 1], [4, 2], [4, 3]], np.uint64)
    counts = np.array([3 * 10 ** 9, 5, 3 * 10 ** 9, 7], np.uint64)
    out = rag.merge_overlaps(pairs, counts)
    np.testing.assert_array_equal(out['pairs'], [[1, 1], [4, 2], [4, 3]])
    np.testing.assert_array_equal(out['counts'], [5, 6 * 10 ** 9, 7])
    np.testing.assert_array_equal(out['nodes'], [1, 4])


def test_merge_keys_above_2_32(gpu):
    big, top = int(BIG), int(TOP)
    pairs = np.array([[big + 1, 3], [2, big], [big + 1, 3], [top + 4, top + 1], [2, big], [2, 1],
                      [top + 4, top + 1], [big + 1, top]], np.uint64)
    counts = np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint64)
    out = rag.merge_overlaps(pairs, counts)
    np.testing.assert_array_equal(out['pairs'], np.array([[2, 1], [2, big], [big + 1, 3], [big + 1, top],
                                                          [top + 4, top + 1]], np.uint64))
    np.testing.assert_array_equal(out['counts'], [6, 7, 4, 8, 11])
    np.testing.assert_array_equal(out['nodes'], np.array([2, big + 1, top + 4], np.uint64))
    lab, cnt = rag.max_overlaps(out, big, big + 3)
    np.testing.assert_array_equal(lab, np.array([0, top, 0], np.uint64))
    np.testing.assert_array_equal(cnt, [0, 8, 0])


# ----------------------------------------------------------------- arg-max
def test_max_overlaps(gpu):
    # node 3 ties between 9 and 4 (the smaller wins), node 5 between three
    pairs = np.array([[1, 8], [3, 9], [3, 4], [3, 6], [5, 2], [5, 7], [5, 1], [9, 9]], np.uint64)
    counts = np.array([2, 5, 5, 1, 3, 3, 3, 1], np.uint64)
    tables = dict(pairs=pairs, counts=counts)
    lab, cnt = rag.max_overlaps(tables, 0, 12)                  # gaps: 0, 2, 4, 6-8, 10, 11
    np.testing.assert_array_equal(lab, [0, 8, 0, 4, 0, 1, 0, 0, 0, 9, 0, 0])
    np.testing.assert_array_equal(cnt, [0, 2, 0, 5, 0, 3, 0, 0, 0, 1, 0, 0])
    m = rag.merge_overlaps(pairs, counts)
    ref = max_overlap(m['pairs'], m['counts'], 0, 12)
    np.testing.assert_array_equal(lab, ref[0])
    np.testing.assert_array_equal(cnt, ref[1])
    assert ref[2][3] and ref[2][5]
    lab, cnt = rag.max_overlaps(tables, 3, 10)                  # a range that starts above 0
    np.testing.assert_array_equal(lab, [4, 0, 1, 0, 0, 0, 9])
    np.testing.assert_array_equal(cnt, [5, 0, 3, 0, 0, 0, 1])
    lab, cnt = rag.max_overlaps(tables, 6, 6)
    assert lab.shape == (0,) and cnt.shape == (0,)
    # on a scanned table
    a, b = two_labellings((12, 14, 75), seed=12)
    r = rag.label_overlaps_handle(a, b)
    p, c = overlap_table(a, b)
    for lb, le in ((0, int(a.max()) + 3), (7, 40)):
        lab, cnt = rag.max_overlaps(r, lb, le)
        ref = max_overlap(p, c, lb, le)
        np.testing.assert_array_equal(lab, ref[0])
        np.testing.assert_array_equal(cnt, ref[1])
    r.free()
    with pytest.raises(_lib.CtgError, match='not an overlaps result'):
        g = rag.rag_features_handle(a)
        try:
            rag.max_overlaps(g, 0, 4)
        finally:
            g.free()


def test_torch_tensors_and_handles(gpu):
    import torch
    a, b = two_labellings((11, 10, 100), seed=13)
    p, c = overlap_table(a, b, 0)
    at = torch.from_numpy(a.view(np.int64)).cuda()
    bt = torch.from_numpy(b.astype(np.uint32).view(np.int32)).cuda()
    out = rag.label_overlaps(at, bt, ignore_label=0)
    np.testing.assert_array_equal(out['pairs'], p)
    np.testing.assert_array_equal(out['counts'], c)
    r = rag.label_overlaps_handle(at, bt, ignore_label=0)
    assert r.n_edges == p.shape[0] and r.n_nodes == np.unique(p[:, 0]).shape[0]
    n_rec, n_direct = r.info()
    assert n_rec >= r.n_edges and n_direct == 0
    pt, ct = r.edges_torch_i64(), r.counts_torch()
    assert pt.is_cuda and ct.is_cuda
    np.testing.assert_array_equal(pt.cpu().numpy().view(np.uint64), p)
    np.testing.assert_array_equal(ct.cpu().numpy().view(np.uint64), c)
    # device tables in, a handle out
    m = rag.merge_overlaps_handle(torch.cat([pt, pt]), torch.cat([ct, ct]))
    np.testing.assert_array_equal(m.edges(), p)
    np.testing.assert_array_equal(m.counts(), c * np.uint64(2))
    ref = max_overlap(p, c, 0, 50)
    for h in (r, m):
        lab, cnt = rag.max_overlaps(h, 0, 50)
        np.testing.assert_array_equal(lab, ref[0])
        np.testing.assert_array_equal(cnt, ref[1] * np.uint64(1 if h is r else 2))
    r.free()
    m.free()
    with pytest.raises(ValueError, match='both'):
        rag.label_overlaps(at, b)


def test_deferred_stats_survive_an_overlaps_call(gpu):
    """A CTG_DEFER_STATS table still packs after overlaps calls on its device:
    they keep their records in buffers of their own.  The exchange simulation
    of tests/exchange_sim.py with 2 slabs (one slab moves no rows, so nothing
    would be packed) and an overlaps, a merge and an arg-max call right before
    every pack."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    a, b = two_labellings((16, 16, 128), seed=14)
    p, c = overlap_table(a, b)
    calls = []

    def overlaps_between():
        out = rag.label_overlaps(a, b)
        np.testing.assert_array_equal(out['pairs'], p)
        m = rag.merge_overlaps(out['pairs'], out['counts'])
        np.testing.assert_array_equal(m['counts'], c)
        rag.max_overlaps(m, 0, 10)
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=overlaps_between)
    assert calls
    np.testing.assert_array_equal(np.concatenate([x.edges() for x in shards]),
                                  np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 1, before_pack=overlaps_between)
    assert shards[0].n_edges == sum(x.n_edges for x in eager)


# ---------------------------------------------------------------- workflow
def test_node_label_workflow(gpu, tmp_path):
    """NodeLabelWorkflow through the harness job bodies on a 40 x 60 x 70
    volume with 32^3 blocks and two node ranges: every block chunk equals the
    oracle on that block (test_node_labels.py test_subresults), the merged
    max-overlap vector equals the oracle with the smallest-label tie rule
    (hence wherever there is no tie, test_max_overlap), and the
    max_overlap=False chunks hold the whole-volume table (test_overlaps)."""
    shape, block = (40, 60, 70), (32, 32, 32)
    ws, lab = two_labellings(shape, seed=15, cell=6, coarse=14)
    lab[30:, 40:, :] = 0
    max_id = int(ws.max())
    node_chunk = (max_id + 2) // 2
    assert node_chunk < max_id + 1 <= 2 * node_chunk              # two node ranges
    path, out = str(tmp_path / 'in.n5'), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('ws', shape=shape, chunks=block, dtype='uint64', compression='gzip')[:] = ws
        f.create_dataset('gt', shape=shape, chunks=block, dtype='uint64', compression='gzip')[:] = lab
    p, c = overlap_table(ws, lab)
    workflow.node_label_workflow(path, 'ws', path, 'gt', out, 'labels', block, max_id, node_chunk=node_chunk,
                                 max_jobs=2)
    # block chunks
    blk = workflow.blocking([0, 0, 0], list(shape), list(block))
    assert blk.numberOfBlocks == 2 * 2 * 3
    for bid in range(blk.numberOfBlocks):
        bb = blk.getBlock(bid)
        sl = tuple(slice(x, y) for x, y in zip(bb.begin, bb.end))
        chunk_id = tuple(x // s for x, s in zip(bb.begin, block))
        got, max_node = ndist.deserializeOverlapChunk(out, 'label_overlaps_', chunk_id)
        assert got == table_dict(*overlap_table(ws[sl], lab[sl]))
        assert max_node == int(ws[sl].max())
    # merged arg-max
    ref_lab, ref_cnt, tie = max_overlap(p, c, 0, max_id + 1)
    with n5.File(out, 'r') as f:
        assert f['labels'].shape == (max_id + 1,) and f['label_overlaps_'].attrs['maxId'] == max_id
        got = f['labels'][:]
    assert tie.any() and not tie.all()
    np.testing.assert_array_equal(got[~tie], ref_lab[~tie])
    np.testing.assert_array_equal(got, ref_lab)
    # with counts
    workflow.node_label_workflow(path, 'ws', path, 'gt', out, 'labels_counts', block, max_id,
                                 node_chunk=node_chunk, serialize_counts=True, prefix='c')
    with n5.File(out, 'r') as f:
        got = f['labels_counts'][:]
    np.testing.assert_array_equal(got, np.stack([ref_lab, ref_cnt], axis=1))
    # all overlaps: one chunk per node range
    workflow.node_label_workflow(path, 'ws', path, 'gt', out, 'overlaps', block, max_id, node_chunk=node_chunk,
                                 max_overlap=False, prefix='all')
    lo, _ = ndist.deserializeOverlapChunk(out, 'overlaps', (0,))
    hi, _ = ndist.deserializeOverlapChunk(os.path.join(out, 'overlaps'), (1,))
    assert lo and hi and max(lo) < node_chunk <= min(hi)
    assert {**lo, **hi} == table_dict(p, c)
    # an ignore label: the rows of label 0 are gone, and blocks that hold nothing else write no chunk
    workflow.node_label_workflow(path, 'ws', path, 'gt', out, 'overlaps_ign', block, max_id,
                                 node_chunk=max_id + 1, max_overlap=False, ignore_label=0, prefix='ign')
    got, _ = ndist.deserializeOverlapChunk(out, 'overlaps_ign', (0,))
    assert got == table_dict(*overlap_table(ws, lab, 0))
