"""Region features on the GPU (ctg_region_features, ctg_merge_region_features,
ctg_region_rows, cluster_tools_amd.features and the harness workflow) against
the numpy oracle of tests/test_region_features_host.py.  "Exact" is
assert_array_equal on nodes, counts, sums, min / max and both row forms: the
float32 data is drawn as k / 256, k in [0, 256], whose partial sums are all
representable, so every order of the adds gives the same bits.  Data that is
not exactly summable is compared within 2 (n - 1) 2^-53 sum|x|."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import _lib, features, n5, rag
from cluster_tools_amd import synthetic as S
from harness import workflow

from test_region_features_host import (check_against_kat, dense_rows, feature_rows, kat_inputs, region_table,
                                       sum_bound, sum_rows)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = np.uint64(1) << np.uint64(40)
TOP = np.uint64(1) << np.uint64(63)


def supervoxels(shape, seed=0, cell=5):
    return S.generate(shape, cell=cell, seed=seed, with_boundary=False)[0]


def grid_data(shape, seed):
    """float32 k / 256, k in [0, 256]: exactly summable."""
    return (np.random.default_rng(seed).integers(0, 257, size=shape) / 256.0).astype(np.float32)


def distinct_data(shape):
    """A different exactly summable value at every voxel of a row and of its
    neighbours: (index mod 4093) / 4096."""
    return ((np.arange(int(np.prod(shape))) % 4093) / 4096.0).astype(np.float32).reshape(shape)


def check_exact(out, labels, data, ignore_label=None, norm=None):
    """out == the oracle's table of (labels, data), every array and both row forms."""
    t = region_table(labels, data, ignore_label)
    norm = (255.0 if data.dtype == np.uint8 else 1.0) if norm is None else norm
    np.testing.assert_array_equal(out['nodes'], t['nodes'])
    np.testing.assert_array_equal(out['counts'], t['counts'])
    np.testing.assert_array_equal(out['sums'], t['sums'])
    np.testing.assert_array_equal(out['minmax'], t['minmax'])
    np.testing.assert_array_equal(out['rows'], sum_rows(t))
    np.testing.assert_array_equal(out['features'], feature_rows(t, norm))
    n = t['nodes'].shape[0]
    assert out['nodes'].dtype == out['counts'].dtype == np.uint64 and out['sums'].dtype == np.float64
    assert out['minmax'].dtype == np.float32 and out['minmax'].shape == (n, 2)
    assert out['rows'].shape == out['features'].shape == (n, 5) and out['rows'].dtype == np.float64
    return t


# ------------------------------------------------------------------ the scan
@pytest.mark.parametrize('variant', ['f32', 'f32_ignore', 'u8', 'u8_ignore'])
def test_hand_computed_case(gpu, variant):
    """tests/golden/region_features_kat.json: moments, both row forms, the dense
    rows of a label range and the chunk words, all written by hand."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'region_features_kat.json')) as fh:
        kat = json.load(fh)
    labels, data, ignore = kat_inputs(kat, variant)
    want = kat[variant]
    out = rag.region_features(labels, data, ignore_label=ignore)
    check_against_kat(out, out['rows'], out['features'], want)
    if variant.startswith('f32'):
        np.testing.assert_array_equal(rag.region_feature_rows(out, *kat['label_range']),
                                      np.array(kat['dense_features_' + variant], np.float64))
    if variant in ('f32', 'u8_ignore'):
        np.testing.assert_array_equal(features.encode_region_chunk(out['rows']),
                                      np.array(kat['chunk_' + variant], np.float64))


@pytest.mark.parametrize('shape', [(5, 7, 67), (17, 9, 130), (1, 1, 1)])
def test_shapes_off_the_tile_grid(gpu, shape):
    """Off the 64 x 8 x 16 tile grid in every axis, crossing a wave in x."""
    a = supervoxels(shape, seed=3)
    d = grid_data(shape, 4)
    check_exact(rag.region_features(a, d), a, d)


RUN_SHAPE = (18, 10, 131)


def test_runs(gpu):
    """One label everywhere (every wave row is one run of 64, then 64, then 3),
    a label that changes at every voxel (every lane a head, nothing folds), and
    runs of 1 .. 15 voxels in one row -- with data that differs at every voxel,
    so a fold that leaks past a head, or stops short of its run's end, changes
    a sum."""
    d = distinct_data(RUN_SHAPE)
    one = np.full(RUN_SHAPE, 7, np.uint64)
    t = check_exact(rag.region_features(one, d), one, d)
    assert t['nodes'].tolist() == [7] and t['counts'][0] == one.size
    x = np.arange(RUN_SHAPE[2], dtype=np.uint64)
    alt = np.broadcast_to(x % np.uint64(2), RUN_SHAPE).copy()
    check_exact(rag.region_features(alt, d), alt, d)
    reps = np.tile(np.arange(1, 16), 2)                           # runs of 1 .. 15 voxels, twice: 240 >= 131
    row = np.repeat(np.arange(reps.size, dtype=np.uint64), reps)[:131]    # a label of its own per run
    runs = np.broadcast_to(row, RUN_SHAPE).copy()
    runs += (np.arange(RUN_SHAPE[0], dtype=np.uint64) % np.uint64(2))[:, None, None] * np.uint64(100)
    t = check_exact(rag.region_features(runs, d), runs, d)
    assert t['nodes'].shape[0] == 2 * (int(row.max()) + 1)
    same = np.broadcast_to(np.repeat(np.arange(reps.size, dtype=np.uint64) % np.uint64(3), reps)[:131],
                           RUN_SHAPE).copy()                              # the same three labels, run after run
    check_exact(rag.region_features(same, d), same, d)


def test_holes(gpu):
    """A row a a I a a b I I b ...: I is the ignore label and the I voxels
    carry data of their own.  The two a runs on either side of a hole do not
    exchange samples and the I samples appear nowhere: the table is the
    oracle's of the voxels that are left."""
    IGN = 9
    pat = np.array([1, 1, IGN, 1, 1, 2, IGN, IGN, 2, 2, 2, IGN, 1, IGN, IGN, IGN, 2, 1, 1, 1, 1, 1, IGN], np.uint64)
    row = np.tile(pat, 6)[:131]
    a = np.broadcast_to(row, RUN_SHAPE).copy()
    a[:, 1::2, :] = np.roll(a[:, 1::2, :], 5, axis=2)              # holes at other lanes in every other row
    d = distinct_data(RUN_SHAPE)
    d[a == IGN] += np.float32(64.0)                               # nothing else reaches 64
    out = rag.region_features(a, d, ignore_label=IGN)
    t = check_exact(out, a, d, ignore_label=IGN)
    assert t['nodes'].tolist() == [1, 2] and out['minmax'].max() < 64
    assert int(out['counts'].sum()) == int((a != IGN).sum())
    # a box of only I: an empty result
    only = np.full((3, 4, 70), IGN, np.uint64)
    out = rag.region_features(only, distinct_data(only.shape), ignore_label=IGN)
    assert out['nodes'].shape == (0,) and out['rows'].shape == (0, 5) and out['minmax'].shape == (0, 2)
    assert out['n_records'] == 0
    out = rag.region_features(a, d, (0, 0, 2), (18, 1, 3), ignore_label=IGN)     # a sub-box of only I
    assert out['nodes'].shape == (0,) and out['features'].shape == (0, 5)
    # the ignore label absent from the box: as without one
    check_exact(rag.region_features(a, d, ignore_label=77), a, d)
    # ignore_label = 0 against no ignore label
    z = a.copy()
    z[z == IGN] = 0
    t0 = check_exact(rag.region_features(z, d, ignore_label=0), z, d, ignore_label=0)
    tn = check_exact(rag.region_features(z, d), z, d)
    assert t0['nodes'].tolist() == [1, 2] and tn['nodes'].tolist() == [0, 1, 2]


@pytest.mark.parametrize('axis,width', [(0, 5), (1, 3), (2, 70)])
def test_segments_larger_than_a_tile(gpu, axis, width):
    """Slabs of 5 planes, 3 rows, 70 columns on (33,17,200): every segment
    spans several tiles and z steps, so its moments come together only in the
    back half."""
    shape = (33, 17, 200)
    idx = np.arange(shape[axis], dtype=np.uint64) // np.uint64(width)
    a = np.broadcast_to(idx.reshape([-1 if k == axis else 1 for k in range(3)]), shape).copy()
    d = grid_data(shape, 6)
    t = check_exact(rag.region_features(a, d), a, d)
    assert t['nodes'].shape[0] == -(-shape[axis] // width)


PRESSURE_SHAPE = (16, 16, 128)


def test_table_pressure(gpu):
    """A distinct label per voxel: 2048 keys per z step against 512 entries
    with 32 probes, so heads go direct and the table is flushed at every step.
    A distinct label per voxel pair along x: 1024 keys per step, direct records
    with run = 2 that carry their pair's folded samples.  arange % 8192: a
    tile's steps meet the same labels again after a flush, so records exceed
    labels."""
    V = int(np.prod(PRESSURE_SHAPE))
    d = distinct_data(PRESSURE_SHAPE)
    a = np.arange(V, dtype=np.uint64).reshape(PRESSURE_SHAPE) + np.uint64(1)
    out = rag.region_features(a, d)
    t = check_exact(out, a, d)
    assert t['nodes'].shape[0] == V and out['n_records'] == V and 0 < out['n_direct'] < V
    np.testing.assert_array_equal(out['sums'], d.ravel().astype(np.float64))
    a = (np.arange(V, dtype=np.uint64) // np.uint64(2)).reshape(PRESSURE_SHAPE)
    out = rag.region_features(a, d)
    t = check_exact(out, a, d)
    assert t['nodes'].shape[0] == V // 2 and (t['counts'] == 2).all() and out['n_direct'] > 0
    a = (np.arange(V, dtype=np.uint64) % np.uint64(8192)).reshape(PRESSURE_SHAPE)
    out = rag.region_features(a, d)
    t = check_exact(out, a, d)
    assert out['n_records'] > t['nodes'].shape[0] and out['n_direct'] > 0


# ------------------------------------------------------------ label ranges
def test_uint32_labels(gpu):
    shape = (7, 9, 80)
    a = supervoxels(shape, seed=8)
    d = grid_data(shape, 9)
    a32 = a.astype(np.uint32)
    out64, out32 = rag.region_features(a, d), rag.region_features(a32, d)
    check_exact(out32, a, d)
    for k in ('nodes', 'counts', 'sums', 'minmax', 'rows', 'features'):
        np.testing.assert_array_equal(out32[k], out64[k])
    a32[2, 3, 10:20] = 0xFFFFFFFF                                  # the bit pattern of a free table slot
    t = check_exact(rag.region_features(a32, d), a32, d)
    assert t['nodes'][-1] == 0xFFFFFFFF
    check_exact(rag.region_features(a32, d, ignore_label=0xFFFFFFFF), a32, d, ignore_label=0xFFFFFFFF)


@pytest.mark.parametrize('ignore', [None, int(BIG) + 3])
def test_labels_above_2_32(gpu, ignore):
    """Labels offset by 2^40 take the monotone dense relabelling, the ignore
    label with them; nodes come back in the original labels.  One label at
    2^63: the moments hold it, the float64 id column does not."""
    shape = (9, 11, 70)
    a = supervoxels(shape, seed=7) % np.uint64(40) + BIG
    assert (a == BIG + np.uint64(3)).any()
    d = grid_data(shape, 10)
    t = check_exact(rag.region_features(a, d, ignore_label=ignore), a, d, ignore_label=ignore)
    assert (int(BIG) + 3 in t['nodes'].tolist()) == (ignore is None)
    sl = (slice(1, 8), slice(2, 11), slice(3, 69))
    check_exact(rag.region_features(a, d, (1, 2, 3), (8, 11, 69), ignore_label=ignore), a[sl], d[sl],
                ignore_label=ignore)
    a[a == a.max()] = TOP
    t = region_table(a, d, ignore)
    assert t['nodes'][-1] == TOP
    r = rag.region_features_handle(a, d, ignore_label=ignore)
    try:
        np.testing.assert_array_equal(r.nodes(), t['nodes'])
        counts, sums, minmax = r.region_moments()
        np.testing.assert_array_equal(counts, t['counts'])
        np.testing.assert_array_equal(sums, t['sums'])
        np.testing.assert_array_equal(minmax, t['minmax'])
        with pytest.raises(_lib.CtgError, match=r'2\^53'):
            r.region_rows()
        with pytest.raises(_lib.CtgError, match=r'2\^53'):
            rag.region_feature_rows(r, 0, 10)
    finally:
        r.free()


# ------------------------------------------------------------------- data
def test_uint8_data(gpu):
    shape = (11, 10, 100)
    a = supervoxels(shape, seed=12)
    d = np.random.default_rng(13).integers(0, 256, size=shape).astype(np.uint8)
    out = rag.region_features(a, d)
    t = check_exact(out, a, d, norm=255.0)
    assert out['features'][:, 2].max() <= 1.0 and out['sums'].max() > 255.0
    np.testing.assert_array_equal(out['sums'], np.rint(out['sums']))
    np.testing.assert_array_equal(rag.region_features(a, d, norm=1.0)['features'], feature_rows(t, 1.0))


def test_noise_within_the_summation_bound(gpu):
    """float32 noise that is not exactly summable (fourth powers of uniform
    draws: exponents far apart): counts and min / max exact, every sum within
    2 (n - 1) 2^-53 sum|x| of the oracle's, sum|x| from the oracle."""
    shape = (20, 21, 150)
    a = supervoxels(shape, seed=14, cell=8)
    d = (np.random.default_rng(15).random(shape) ** 4).astype(np.float32)
    out = rag.region_features(a, d)
    t = region_table(a, d)
    np.testing.assert_array_equal(out['nodes'], t['nodes'])
    np.testing.assert_array_equal(out['counts'], t['counts'])
    np.testing.assert_array_equal(out['minmax'], t['minmax'])
    err, bound = np.abs(out['sums'] - t['sums']), sum_bound(t['counts'], t['abs_sums'])
    print('largest |sum - oracle| / bound: %.3g over %d labels' % (float((err / np.maximum(bound, 1e-300)).max()),
                                                                 t['nodes'].shape[0]))
    assert (err <= bound).all()
    np.testing.assert_array_equal(out['rows'][:, 2], out['sums'])
    np.testing.assert_array_equal(out['features'][:, 2], out['sums'] / out['counts'].astype(np.float64))


# --------------------------------------------------------- boxes and errors
def test_sub_box_and_error_paths(gpu):
    shape = (20, 21, 150)
    a = supervoxels(shape, seed=4)
    d = grid_data(shape, 5)
    begin, end = (3, 2, 5), (19, 17, 139)
    sl = tuple(slice(x, y) for x, y in zip(begin, end))
    check_exact(rag.region_features(a, d, begin, end), a[sl], d[sl])
    check_exact(rag.region_features(a, d, begin=begin), a[3:, 2:, 5:], d[3:, 2:, 5:])
    check_exact(rag.region_features(a, d, begin, end, ignore_label=int(a[5, 5, 50])), a[sl], d[sl],
                ignore_label=int(a[5, 5, 50]))
    out = rag.region_features(a, d, (4, 4, 4), (4, 9, 9))          # empty box
    assert out['nodes'].shape == (0,) and out['counts'].shape == (0,) and out['minmax'].shape == (0, 2)
    assert out['rows'].shape == (0, 5) and out['features'].shape == (0, 5)
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.region_features(a, d, (0, 0, 0), (21, 21, 150))
    with pytest.raises(_lib.CtgError, match='outside'):
        rag.region_features(a, d, (5, 0, 0), (4, 21, 150))
    r = rag.region_features_handle(a, d)
    g = rag.rag_features_handle(a)
    try:
        lib = _lib.load()
        buf = np.zeros((r.n_nodes, 5))
        for form, norm, text in ((2, 1.0, 'form'), (1, 0.0, 'norm'), (1, float('nan'), 'norm')):
            rc = lib.ctg_region_rows(r.handle, 0, 0, form, norm, None, buf.ctypes.data_as(_lib.c_vp), 0, None)
            assert rc == -1 and text in lib.ctg_last_error().decode()
        assert not buf.any()
        with pytest.raises(_lib.CtgError, match='not a region-features result'):
            rag.region_feature_rows(g, 0, 4)
        with pytest.raises(_lib.CtgError, match='no region moments'):
            g.region_moments()
        with pytest.raises(_lib.CtgError, match='not a morphology result'):
            rag.morphology_rows(r, 0, 4)
    finally:
        r.free()
        g.free()


# ------------------------------------------------------------------- merge
MERGE_SHAPE = (20, 21, 150)


@pytest.fixture(scope='module')
def merge_case():
    a = supervoxels(MERGE_SHAPE, seed=10, cell=6)
    a[1:3, 2:5, 3:9] = 10 ** 6                                    # a label of one block only
    return a, grid_data(MERGE_SHAPE, 11)


def test_merge_equals_one_whole_volume_call(gpu, merge_case):
    """The block tables of a 2 x 2 x 2 blocking, in a shuffled row order, merge
    to the whole-volume table bit for bit; rows of count 0 add nothing; a bad id
    or count is CTG_ERR_ARG."""
    a, d = merge_case
    parts = []
    for z in (0, 10):
        for y in (0, 11):
            for x in (0, 75):
                sl = (slice(z, z + 10), slice(y, y + 11 if y == 0 else 21), slice(x, x + 75))
                parts.append(rag.region_features(a[sl], d[sl])['rows'])
    assert len(parts) == 8 and sum(int((p[:, 0] == 10 ** 6).sum()) for p in parts) == 1
    rows = np.concatenate(parts)
    whole = rag.region_features(a, d)
    t = check_exact(whole, a, d)
    assert rows.shape[0] > t['nodes'].shape[0]                            # labels that span blocks
    rng = np.random.default_rng(12)
    out = rag.merge_region_features(rows[rng.permutation(rows.shape[0])])
    for k in ('nodes', 'counts', 'sums', 'minmax', 'rows', 'features'):
        np.testing.assert_array_equal(out[k], whole[k])
    # zero-count rows add nothing: not to a label with voxels (whatever their other columns say) ...
    absent = float(t['nodes'].max() + 5)
    zero = np.array([[rows[0, 0], 0, 123.0, -5.0, 99.0], [absent, 0, 0, 0, 0], [rows[3, 0], 0, 7.0, 0.0, 500.0]])
    out = rag.merge_region_features(np.concatenate([zero[:2], rows, zero[2:]]))
    np.testing.assert_array_equal(out['nodes'], np.append(whole['nodes'], np.uint64(absent)))
    for k in ('counts', 'sums', 'minmax', 'rows', 'features'):
        np.testing.assert_array_equal(out[k][:-1], whole[k])
    # ... and a label with nothing else is a row of zeros after its id
    assert out['counts'][-1] == 0 and not out['rows'][-1, 1:].any() and not out['features'][-1, 1:].any()
    dense = rag.region_feature_rows(dict(rows=np.concatenate([rows, zero])), int(absent) - 2, int(absent) + 2)
    assert not dense.any()
    # dense rows over a range that cuts the table
    lb, le = int(t['nodes'][3]), int(t['nodes'][-2])
    np.testing.assert_array_equal(rag.region_feature_rows(dict(rows=rows), lb, le),
                                  dense_rows(feature_rows(t, 1.0), lb, le))
    np.testing.assert_array_equal(rag.region_feature_rows(dict(rows=rows), lb, le, 'sums'),
                                  dense_rows(sum_rows(t), lb, le))
    out = rag.merge_region_features(np.zeros((0, 5)))
    assert out['nodes'].shape == (0,) and out['rows'].shape == (0, 5)
    for bad in ([1.5, 1, 0, 0, 0], [-1, 1, 0, 0, 0], [2.0 ** 53, 1, 0, 0, 0], [np.nan, 1, 0, 0, 0],
                [1, -1, 0, 0, 0], [1, np.inf, 0, 0, 0], [1, np.nan, 0, 0, 0]):
        with pytest.raises(_lib.CtgError, match='status -1.*id'):
            rag.merge_region_features(np.array([rows[0], bad]))


def test_torch_tensors_and_handles(gpu, merge_case):
    import torch
    a, d = merge_case
    t = region_table(a, d, 10 ** 6)
    at, dt = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(d).cuda()
    check_exact(rag.region_features(at, dt, ignore_label=10 ** 6), a, d, ignore_label=10 ** 6)
    d8 = (d * 255).astype(np.uint8)
    check_exact(rag.region_features(torch.from_numpy(a.astype(np.uint32).view(np.int32)).cuda(),
                                    torch.from_numpy(d8).cuda()), a, d8)
    r = rag.region_features_handle(at, dt, ignore_label=10 ** 6)
    n_rec, n_direct = r.info()
    assert r.n_nodes == t['nodes'].shape[0] and n_rec >= r.n_nodes and n_direct == 0
    rt = r.region_rows_torch()
    assert rt.is_cuda
    np.testing.assert_array_equal(rt.cpu().numpy(), sum_rows(t))
    m = rag.merge_region_features_handle(torch.cat([rt, rt]))      # twice the rows: twice the voxels, the same mean
    counts, sums, minmax = m.region_moments()
    np.testing.assert_array_equal(counts, t['counts'] * np.uint64(2))
    np.testing.assert_array_equal(sums, t['sums'] * 2)
    np.testing.assert_array_equal(minmax, t['minmax'])
    np.testing.assert_array_equal(m.region_rows('features')[:, 2:], feature_rows(t, 1.0)[:, 2:])
    r.free()
    m.free()
    r.free()
    with pytest.raises(ValueError, match='both'):
        rag.region_features(at, d)


def test_deferred_stats_survive_a_region_features_call(gpu, merge_case):
    """A CTG_DEFER_STATS table still packs after region-features calls on its
    device: they keep their records in buffers of their own."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    a, d = merge_case
    want = region_table(a, d)
    calls = []

    def region_between():
        out = rag.region_features(a, d)
        np.testing.assert_array_equal(out['sums'], want['sums'])
        m = rag.merge_region_features(out['rows'])
        np.testing.assert_array_equal(m['counts'], want['counts'])
        rag.region_feature_rows(m, 0, 10)
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=region_between)
    assert calls
    np.testing.assert_array_equal(np.concatenate([x.edges() for x in shards]),
                                  np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------- workflow
@pytest.mark.parametrize('label_dtype', ['uint64', 'uint32'])
def test_region_features_workflow(gpu, tmp_path, label_dtype):
    """RegionFeaturesWorkflow through the harness job bodies on a (40,48,140)
    volume with (16,24,70) blocks, uint8 input, ignore_label 0, in threads
    mode: every block chunk equals the oracle's rows of that block
    (test/features/test_region_features.py:52-93), the merged float32 table
    equals float32(oracle) exactly (:33-50), labels absent from the volume have
    zero rows."""
    shape, block = (40, 48, 140), (16, 24, 70)
    seg = supervoxels(shape, seed=16, cell=7)
    seg[:16, :24, :70] = 0                                        # block (0, 0, 0): nothing but the ignore label
    seg[20:30, 30:40, 80:120] = 0                                 # and some of it elsewhere
    seg[seg == 50] = 49                                           # an absent label
    n_labels = int(seg.max()) + 4                                 # and three past the largest
    node_chunk = (n_labels + 2) // 3
    assert 2 * node_chunk < n_labels <= 3 * node_chunk            # three label ranges
    raw = np.random.default_rng(17).integers(0, 256, size=shape).astype(np.uint8)
    path, tmp, out = str(tmp_path / 'in.n5'), str(tmp_path / 'tmp.n5'), str(tmp_path / 'out.n5')
    with n5.File(path) as f:
        f.create_dataset('seg', shape=shape, chunks=block, dtype=label_dtype, compression='gzip')[:] = \
            seg.astype(label_dtype)
        f.create_dataset('raw', shape=shape, chunks=block, dtype='uint8', compression='gzip')[:] = raw
    names = ('count', 'mean', 'minimum', 'maximum')
    workflow.region_features_workflow(path, 'raw', path, 'seg', out, 'feats', tmp, block, n_labels, ignore_label=0,
                                      feature_names=names, node_chunk=node_chunk, max_jobs=2, mode='threads')
    blk_ids = [(z, y, x) for z in range(3) for y in range(2) for x in range(2)]
    with n5.File(tmp, 'r') as f:
        ds = f['block_feats']
        assert ds.dtype == np.float64 and tuple(ds.chunks) == block
        assert ds.attrs['feature_names'] == list(names) and ds.attrs['norm'] == 255.0
        assert not ds.chunk_exists((0, 0, 0))
        for cz, cy, cx in blk_ids[1:]:
            sl = (slice(cz * 16, cz * 16 + 16), slice(cy * 24, cy * 24 + 24), slice(cx * 70, cx * 70 + 70))
            got = features.decode_region_chunk(ds.read_chunk((cz, cy, cx)))
            np.testing.assert_array_equal(got, sum_rows(region_table(seg[sl], raw[sl], 0)))
    with n5.File(out, 'r') as f:
        assert f['feats'].dtype == np.float32 and f['feats'].shape == (n_labels, 4)
        assert tuple(f['feats'].chunks) == (node_chunk, 1)
        res = f['feats'][:]
    t = region_table(seg, raw, 0)
    want = dense_rows(feature_rows(t, 255.0), 0, n_labels)[:, 1:].astype(np.float32)
    np.testing.assert_array_equal(res, want)
    present = np.zeros(n_labels, bool)
    present[t['nodes'].astype(np.int64)] = True
    assert not present[0] and not present[50] and not present[-3:].any() and not res[~present].any()
    assert (res[present, 0] > 0).all() and res[:, 1].max() <= 1.0
    # the default columns (region_features.py:211) into a second dataset, from the same chunks
    workflow.region_features_workflow(path, 'raw', path, 'seg', out, 'feats2', tmp, block, n_labels, ignore_label=0,
                                      node_chunk=node_chunk)
    with n5.File(out, 'r') as f:
        assert f['feats2'].shape == (n_labels, 2)
        np.testing.assert_array_equal(f['feats2'][:], want[:, :2])
