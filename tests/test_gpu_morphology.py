"""Segment morphology on the GPU (ctg_morphology, ctg_merge_morphology,
ctg_morphology_rows and their ndist mirror) against the numpy oracle of
tests/test_morphology_host.py.  Everything is integers until one division of
the same integers the oracle divides: every comparison is exact, the float64
rows included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cluster_tools_amd import _lib, n5, ndist, rag
from cluster_tools_amd import synthetic as S
from harness import workflow

from test_morphology_host import dense_rows, morph_rows, morph_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.uint64(1) << np.uint64(40)
TOP = np.uint64(1) << np.uint64(63)


def supervoxels(shape, seed=0, cell=5):
    return S.generate(shape, cell=cell, seed=seed, with_boundary=False)[0]


def check_table(out, labels, origin=(0, 0, 0)):
    """out (nodes, moments, rows) == the oracle's table of ``labels`` whose
    first voxel sits at ``origin``."""
    nodes, mom = morph_table(labels, origin)
    np.testing.assert_array_equal(out['nodes'], nodes)
    np.testing.assert_array_equal(out['moments'], mom)
    np.testing.assert_array_equal(out['rows'], morph_rows(nodes, mom))
    assert out['nodes'].dtype == out['moments'].dtype == np.uint64 and out['rows'].dtype == np.float64
    assert out['moments'].shape == (nodes.shape[0], 10) and out['rows'].shape == (nodes.shape[0], 11)
    return nodes, mom


# ------------------------------------------------------------------ the scan
def test_hand_computed_case(gpu):
    """tests/golden/morphology_kat.json: moments, rows, the dense rows of a label
    range and the chunk words, all written by hand."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'morphology_kat.json')) as fh:
        kat = json.load(fh)
    labels = np.array(kat['labels'], np.uint64)
    out = rag.morphology(labels)
    np.testing.assert_array_equal(out['nodes'], np.array(kat['nodes'], np.uint64))
    np.testing.assert_array_equal(out['moments'], np.array(kat['moments'], np.uint64))
    np.testing.assert_array_equal(out['rows'], np.array(kat['rows'], np.float64))
    np.testing.assert_array_equal(ndist.encode_morphology_chunk(out['rows']), np.array(kat['chunk'], np.float64))
    np.testing.assert_array_equal(rag.morphology_rows(out, *kat['label_range']),
                                  np.array(kat['dense_rows'], np.float64))
    out = rag.morphology(labels, origin=kat['origin'])
    np.testing.assert_array_equal(out['moments'], np.array(kat['moments_at_origin'], np.uint64))


@pytest.mark.parametrize('shape', [(5, 7, 67), (17, 9, 130), (1, 1, 1)])
def test_shapes_off_the_tile_grid(gpu, shape):
    """Off the 64 x 8 x 16 tile grid in every axis, crossing a wave in x."""
    a = supervoxels(shape, seed=3)
    check_table(rag.morphology(a), a)


def test_sub_box_and_origin(gpu):
    """The coordinate of the voxel at array index p is p + origin, so the box
    (3,2,5)-(19,17,139) at origin (100,200,300) is the oracle's table of that
    sub-array with its first voxel at begin + origin."""
    a = supervoxels((20, 21, 150), seed=4)
    begin, end, origin = (3, 2, 5), (19, 17, 139), (100, 200, 300)
    sl = tuple(slice(x, y) for x, y in zip(begin, end))
    check_table(rag.morphology(a, begin, end, origin), a[sl], tuple(b + o for b, o in zip(begin, origin)))
    check_table(rag.morphology(a, begin=begin), a[3:, 2:, 5:], begin)
    check_table(rag.morphology(a, origin=origin), a, origin)
    out = rag.morphology(a, (4, 4, 4), (4, 9, 9), origin)      # empty box
    assert out['nodes'].shape == (0,) and out['moments'].shape == (0, 10) and out['rows'].shape == (0, 11)
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.morphology(a, (0, 0, 0), (21, 21, 150))
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.morphology(a, (5, 0, 0), (4, 21, 150))
    # origin + end must stay below 2^31: the largest origin that does, and one more
    far = (1 << 31) - 1 - 20
    check_table(rag.morphology(a, origin=(far, 0, 0)), a, (far, 0, 0))
    for bad in ((far + 1, 0, 0), (0, 0, (1 << 31) - 150), (0, -1, 0)):
        with pytest.raises(_lib.CtgError, match='origin'):
            rag.morphology(a, origin=bad)


def test_run_collapse(gpu):
    """One label over the whole volume (every wave row is one run), a label
    that changes at every voxel along x (every lane a head), and runs of every
    length in one row."""
    shape = (18, 10, 131)
    Z, Y, X = shape
    V = Z * Y * X
    out = rag.morphology(np.full(shape, 7, np.uint64))
    np.testing.assert_array_equal(out['nodes'], [7])
    np.testing.assert_array_equal(out['moments'], [[V, V * (Z - 1) // 2, V * (Y - 1) // 2, V * (X - 1) // 2,
                                                    0, 0, 0, Z - 1, Y - 1, X - 1]])
    np.testing.assert_array_equal(out['rows'], [[7, V, (Z - 1) / 2, (Y - 1) / 2, (X - 1) / 2,
                                                 0, 0, 0, Z - 1, Y - 1, X - 1]])
    x = np.arange(X, dtype=np.uint64)
    a2 = np.broadcast_to(x % np.uint64(2), shape).copy()
    check_table(rag.morphology(a2), a2)
    rng = np.random.default_rng(5)
    a3 = np.repeat(rng.integers(1, 4, size=(18, 10, 40)), 4, axis=2)[:, :, :131].astype(np.uint64)
    check_table(rag.morphology(a3), a3)
    reps = np.tile(np.arange(1, 16), 2)                           # runs of 1 .. 15 voxels, twice: 240 >= 131
    row = np.repeat(np.arange(reps.size, dtype=np.uint64) % np.uint64(3), reps)[:131]
    a4 = np.broadcast_to(row, shape).copy()
    check_table(rag.morphology(a4), a4)


@pytest.mark.parametrize('axis,width', [(0, 5), (1, 3), (2, 70)])
def test_segments_larger_than_a_tile(gpu, axis, width):
    """Slabs of 5 planes, 3 rows, 70 columns on (33,17,200): every segment
    spans several tiles and z steps, so its box and sums come together only in
    the back half."""
    shape = (33, 17, 200)
    idx = np.arange(shape[axis], dtype=np.uint64) // np.uint64(width)
    a = np.broadcast_to(idx.reshape([-1 if k == axis else 1 for k in range(3)]), shape).copy()
    nodes, mom = check_table(rag.morphology(a), a)
    assert nodes.shape[0] == -(-shape[axis] // width)


PRESSURE_SHAPE = (16, 16, 128)


def test_table_pressure(gpu):
    """A distinct label at every voxel: each 64 x 8 x 16 tile meets 8192 keys,
    2048 per z step (4 planes x 8 rows x 64), against a 512-entry LDS table
    with 32 probes -- the table fills (heads that find no slot write direct
    records) and is flushed after every step.  Every voxel is its own label, so
    the scan writes exactly one record per label.  With labels = arange % 8192
    a tile's 4 steps each meet the same 2048 labels (z * 2048 + y * 128 + x mod
    8192 repeats every 4 planes): flushed, then met again, so records exceed
    labels."""
    V = int(np.prod(PRESSURE_SHAPE))
    a = np.arange(V, dtype=np.uint64).reshape(PRESSURE_SHAPE) + np.uint64(1)
    out = rag.morphology(a)
    nodes, mom = check_table(out, a)
    assert nodes.shape[0] == V and out['n_records'] == V
    assert 0 < out['n_direct'] < out['n_records']          # direct records and flushed entries
    z, y, x = np.unravel_index(np.arange(V), PRESSURE_SHAPE)
    assert (mom[:, 0] == 1).all()
    for c, g in enumerate((z, y, x)):                      # com == min == max == the coordinate
        np.testing.assert_array_equal(out['rows'][:, 2 + c], g)
        np.testing.assert_array_equal(out['rows'][:, 5 + c], g)
        np.testing.assert_array_equal(out['rows'][:, 8 + c], g)
    a = (np.arange(V, dtype=np.uint64) % np.uint64(8192)).reshape(PRESSURE_SHAPE)
    out = rag.morphology(a)
    nodes, _ = check_table(out, a)
    assert out['n_records'] > nodes.shape[0] and out['n_direct'] > 0


def test_first_record_buffer_too_small():
    """A fresh process: a tiny call, then the table-pressure call, whose V
    records do not fit the first attempt's buffer (max(4096, V / 16) records);
    the scan runs again with the counted size and the table is exact."""
    code = (
        "import numpy as np\n"
        "from cluster_tools_amd import rag\n"
        "t = rag.morphology(np.ones((1, 1, 2), np.uint64))\n"
        "assert t['nodes'].tolist() == [1] and t['moments'].tolist() == [[2, 0, 0, 1, 0, 0, 0, 0, 0, 1]]\n"
        "shape = %r\n"
        "V = int(np.prod(shape))\n"
        "assert V > max(4096, V // 16)\n"
        "a = np.arange(V, dtype=np.uint64).reshape(shape)\n"
        "out = rag.morphology(a)\n"
        "z, y, x = np.unravel_index(np.arange(V), shape)\n"
        "assert (out['nodes'] == np.arange(V)).all() and out['n_records'] == V\n"
        "m = out['moments']\n"
        "assert (m[:, 0] == 1).all()\n"
        "for c, g in enumerate((z, y, x)):\n"
        "    assert (m[:, 1 + c] == g).all() and (m[:, 4 + c] == g).all() and (m[:, 7 + c] == g).all()\n"
        "print('RETRY_OK')\n") % (PRESSURE_SHAPE,)
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and 'RETRY_OK' in r.stdout, r.stderr[-2000:]


# ------------------------------------------------------------ label ranges
def test_labels_above_2_32(gpu):
    """Labels >= 2^32 take the monotone dense relabelling; nodes and moments
    come back in the original labels.  A label >= 2^53 does not fit the rows' id
    column: the rows are refused, the moments table holds it."""
    a = supervoxels((9, 11, 70), seed=7) * np.uint64(977) + BIG
    check_table(rag.morphology(a), a)
    sl = (slice(1, 8), slice(2, 11), slice(3, 69))
    check_table(rag.morphology(a, (1, 2, 3), (8, 11, 69), (5, 6, 7)), a[sl], (6, 8, 10))
    a[a == a.max()] = TOP + np.uint64(5)
    nodes, mom = morph_table(a)
    assert nodes[-1] >= TOP
    r = rag.morphology_handle(a)
    try:
        np.testing.assert_array_equal(r.nodes(), nodes)
        np.testing.assert_array_equal(r.moments(), mom)
        with pytest.raises(_lib.CtgError, match=r'2\^53'):
            r.morph_rows()
        with pytest.raises(_lib.CtgError, match=r'2\^53'):
            rag.morphology_rows(r, 0, 10)
    finally:
        r.free()
    with pytest.raises(_lib.CtgError, match=r'2\^53'):
        rag.morphology(a)


def test_uint32_inputs(gpu):
    a = supervoxels((7, 9, 80), seed=8)
    a32 = a.astype(np.uint32)
    out64, out32 = rag.morphology(a), rag.morphology(a32)
    check_table(out32, a)
    for k in ('nodes', 'moments', 'rows'):
        np.testing.assert_array_equal(out32[k], out64[k])
    # the largest 32-bit label has the bit pattern of a free table slot
    a32[2, 3, 10:20] = 0xFFFFFFFF
    nodes, _ = check_table(rag.morphology(a32), a32)
    assert nodes[-1] == 0xFFFFFFFF
    # signed views of the same bits
    check_table(rag.morphology(a.view(np.int64)), a)
    check_table(rag.morphology(a32.view(np.int32)), a32)


# ------------------------------------------------------------------- merge
MERGE_SHAPE, MERGE_BLOCK = (24, 40, 72), (12, 20, 24)


@pytest.fixture(scope='module')
def merge_case():
    a = supervoxels(MERGE_SHAPE, seed=10, cell=6)
    a[1:3, 2:5, 3:9] = 10 ** 6                                    # a label of one block only
    return a, morph_table(a)


def block_rows(a):
    parts = []
    for z in range(0, MERGE_SHAPE[0], MERGE_BLOCK[0]):
        for y in range(0, MERGE_SHAPE[1], MERGE_BLOCK[1]):
            for x in range(0, MERGE_SHAPE[2], MERGE_BLOCK[2]):
                blk = a[z:z + MERGE_BLOCK[0], y:y + MERGE_BLOCK[1], x:x + MERGE_BLOCK[2]]
                parts.append(rag.morphology(blk, origin=(z, y, x))['rows'])
    return parts


def test_merge_equals_one_whole_volume_call(gpu, merge_case):
    """12 blocks of (12,20,24), each called with its origin; their rows in a
    shuffled order merge to the whole-volume table bit for bit."""
    a, (nodes, mom) = merge_case
    parts = block_rows(a)
    assert len(parts) == 12
    assert sum(int((p[:, 0] == 10 ** 6).sum()) for p in parts) == 1
    rows = np.concatenate(parts)
    assert rows.shape[0] > nodes.shape[0]                         # labels that span blocks
    whole = rag.morphology(a)
    check_table(whole, a)
    rng = np.random.default_rng(11)
    out = rag.merge_morphology(rows[rng.permutation(rows.shape[0])])
    for k in ('nodes', 'moments', 'rows'):
        np.testing.assert_array_equal(out[k], whole[k])
    check_table(out, a)
    out = rag.merge_morphology(np.zeros((0, 11)))
    assert out['nodes'].shape == (0,) and out['moments'].shape == (0, 10) and out['rows'].shape == (0, 11)
    with pytest.raises(_lib.CtgError, match='id'):
        rag.merge_morphology(np.array([[1.5, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]]))
    with pytest.raises(_lib.CtgError, match='id'):
        rag.merge_morphology(np.array([[1, 1, 0, np.nan, 0, 0, 0, 0, 0, 0, 0]]))


def test_dense_rows_over_a_label_range(gpu, merge_case):
    """A label range that cuts the table and contains absent labels: their
    rows are all zeros."""
    a, (nodes, mom) = merge_case
    a = a.copy()
    gone = [int(nodes[5]), int(nodes[6]), int(nodes[20])]
    for g in gone:
        a[a == g] = nodes[4]
    nodes, mom = morph_table(a)
    rows = morph_rows(nodes, mom)
    lb, le = int(nodes[3]), int(nodes[-2])                        # cuts both ends (and the one-block label)
    assert lb > 0 and all(lb <= g < le for g in gone)
    r = rag.morphology_handle(a)
    try:
        got = rag.morphology_rows(r, lb, le)
        empty = rag.morphology_rows(r, 7, 7)
        past = rag.morphology_rows(r, 2 * 10 ** 6, 2 * 10 ** 6 + 3)
    finally:
        r.free()
    np.testing.assert_array_equal(got, dense_rows(rows, lb, le))
    for g in gone:
        assert not got[g - lb].any()
    assert got[int(nodes[7]) - lb, 1] > 0
    assert empty.shape == (0, 11) and past.shape == (3, 11) and not past.any()
    # from a dict of rows (merged first)
    np.testing.assert_array_equal(rag.morphology_rows(dict(rows=rows), lb, le), got)
    with pytest.raises(_lib.CtgError, match='not a morphology result'):
        g = rag.rag_features_handle(a)
        try:
            rag.morphology_rows(g, 0, 4)
        finally:
            g.free()


def test_torch_tensors_and_handles(gpu):
    import torch
    a = supervoxels((11, 10, 100), seed=13)
    nodes, mom = morph_table(a, (1, 2, 3))
    rows = morph_rows(nodes, mom)
    at = torch.from_numpy(a.view(np.int64)).cuda()
    check_table(rag.morphology(at, origin=(1, 2, 3)), a, (1, 2, 3))
    a32 = torch.from_numpy(a.astype(np.uint32).view(np.int32)).cuda()
    check_table(rag.morphology(a32), a)
    r = rag.morphology_handle(at, origin=(1, 2, 3))
    assert r.n_nodes == nodes.shape[0]
    n_rec, n_direct = r.info()
    assert n_rec >= r.n_nodes and n_direct == 0
    mt, rt, nt = r.moments_torch(), r.morph_rows_torch(), r.nodes_torch()
    assert mt.is_cuda and rt.is_cuda and nt.is_cuda
    np.testing.assert_array_equal(mt.cpu().numpy().view(np.uint64), mom)
    np.testing.assert_array_equal(rt.cpu().numpy(), rows)
    np.testing.assert_array_equal(nt.cpu().numpy().view(np.uint64), nodes)
    # device rows in, a handle out: twice the rows are twice the voxels at the same centre
    m = rag.merge_morphology_handle(torch.cat([rt, rt]))
    np.testing.assert_array_equal(m.nodes(), nodes)
    mom2 = mom.copy()
    mom2[:, :4] *= np.uint64(2)
    np.testing.assert_array_equal(m.moments(), mom2)
    np.testing.assert_array_equal(m.morph_rows()[:, 2:], rows[:, 2:])
    np.testing.assert_array_equal(rag.morphology_rows(m, 0, 50)[:, 2:], dense_rows(rows, 0, 50)[:, 2:])
    r.free()
    m.free()
    r.free()
    m.free()
    with pytest.raises(ValueError, match='float64'):
        rag.merge_morphology_handle(mt)


def test_deferred_stats_survive_a_morphology_call(gpu, merge_case):
    """A CTG_DEFER_STATS table still packs after morphology calls on its
    device: they keep their records in buffers of their own.  The exchange
    simulation of tests/exchange_sim.py with 2 slabs and a morphology, a merge
    and a rows call right before every pack."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    a, (nodes, mom) = merge_case
    calls = []

    def morphology_between():
        out = rag.morphology(a)
        np.testing.assert_array_equal(out['moments'], mom)
        m = rag.merge_morphology(out['rows'])
        np.testing.assert_array_equal(m['moments'], mom)
        rag.morphology_rows(m, 0, 10)
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=morphology_between)
    assert calls
    np.testing.assert_array_equal(np.concatenate([x.edges() for x in shards]),
                                  np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 1, before_pack=morphology_between)
    assert shards[0].n_edges == sum(x.n_edges for x in eager)


# ---------------------------------------------------------------- workflow
def test_morphology_workflow(gpu, tmp_path):
    """MorphologyWorkflow through the harness job bodies on a 24 x 40 x 72
    volume with (10,16,32) blocks -- off the grid in every axis -- one block
    zeroed (skipped: block_morphology.py:120) and three label ranges.  The
    assertions of the reference's test_morphology.py:36-61 against the numpy
    oracle of the whole volume, the centre of mass exact instead of allclose:
    the dataset equals morphology_rows of one whole-volume call."""
    shape, block = (24, 40, 72), (10, 16, 32)
    seg = supervoxels(shape, seed=15, cell=6)
    seg[10:20, 16:32, 32:64] = 0                                  # block (1, 1, 1): nothing but label 0
    seg[seg == 50] = 49                                           # an absent label
    max_id = int(seg.max())
    node_chunk = (max_id + 3) // 3
    assert 2 * node_chunk < max_id + 1 <= 3 * node_chunk          # three merge jobs
    path, out = str(tmp_path / 'in.n5'), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('seg', shape=shape, chunks=block, dtype='uint64', compression='gzip')[:] = seg
    workflow.morphology_workflow(path, 'seg', out, 'morphology', block, max_id, node_chunk=node_chunk, max_jobs=2)
    with n5.File(out, 'r') as f:
        ds_tmp = f['morphology_']
        assert ds_tmp.dtype == np.float64 and tuple(ds_tmp.chunks) == block
        assert not ds_tmp.chunk_exists((1, 1, 1)) and ds_tmp.chunk_exists((0, 0, 0))
        chunk = ndist.decode_morphology_chunk(ds_tmp.read_chunk((2, 2, 2)))
        assert f['morphology'].shape == (max_id + 1, 11) and tuple(f['morphology'].chunks) == (node_chunk, 11)
        res = f['morphology'][:]
    # a block chunk: the block's table in volume coordinates
    nodes_b, mom_b = morph_table(seg[20:24, 32:40, 64:72], (20, 32, 64))
    np.testing.assert_array_equal(chunk, morph_rows(nodes_b, mom_b))
    nodes, mom = morph_table(seg)
    assert nodes[0] == 0 and nodes.shape[0] < max_id + 1          # label 0, and absent labels
    # label 0 lives in the skipped block alone: no row (the reference's test strips it, :32-34)
    assert not res[0].any()
    res, nodes, mom = res[1:], nodes[1:], mom[1:]
    present = res[:, 1] > 0
    ids = np.flatnonzero(present) + 1
    np.testing.assert_array_equal(res[present, 0].astype(np.uint64), ids)              # ids == the row index
    np.testing.assert_array_equal(ids.astype(np.uint64), nodes)
    np.testing.assert_array_equal(res[present, 1].astype(np.uint64), mom[:, 0])        # counts
    np.testing.assert_array_equal(res[present, 5:8].astype(np.uint64), mom[:, 4:7])    # bb_min
    np.testing.assert_array_equal(res[present, 8:].astype(np.uint64), mom[:, 7:])      # bb_max (inclusive)
    np.testing.assert_array_equal(res[present, 2:5], morph_rows(nodes, mom)[:, 2:5])   # centre of mass, exact
    assert not res[~present].any() and (~present).any()
    r = rag.morphology_handle(seg)
    try:
        whole = rag.morphology_rows(r, 0, max_id + 1)
    finally:
        r.free()
    np.testing.assert_array_equal(res, whole[1:])
