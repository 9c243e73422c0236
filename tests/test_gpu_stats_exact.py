"""The mergeable statistics rows (keep_stats: 42 histogram slots, count | ADJ,
ordered min / max, pivot, and the shifted sums S1 / S2) against the oracle's
statistics, word by word, on every path that writes or combines them: the
FAST40 and the general binning of the scan, uint8 maps, the affinity forms,
samples on and next to the bin edges, the statistics merge, and the
packed-histogram reduce on both sides of its 2^16 count threshold (the batched
blocks: test_gpu_blocks.py::test_blocks_boundary_features, with check_stats).

Nothing in these rows is approximate except the two f64 sums: the scan bins
with the oracle's f64 rule (oracle.rag_oracle.histogram_slots), counts are
integers, min / max are float32 samples.  Every case also runs without
keep_stats -- the packed-histogram reduce, another kernel -- through
check_features, whose quantile bar (QTOL) only an exact histogram meets.
"""
import numpy as np
import pytest

from cluster_tools_amd import rag
from cluster_tools_amd import synthetic as S
from oracle import rag_oracle as O

from test_gpu_parity import check_features
from tests.dist_helpers import decode_stats, f2ord

pytestmark = pytest.mark.gpu


def check_stats(out, stats):
    """out: a keep_stats result (sums (E, 2) f64, records (E, 48) u32);
    stats: the oracle's return_stats dictionary for the same edge rows.
    Histogram, count, min and max bit-exact; the mean decoded from
    (pivot, S1) within rtol 1e-12 and m2 / count from (S1, S2) within rtol
    1e-5, the bars of test_variance_constant_and_near_constant_edges and
    check_features.  Rows without samples are all zero up to their min / max /
    pivot words, which no consumer reads."""
    rec, sums = out['records'], out['sums']
    count = stats['count']
    n = count.shape[0]
    assert rec.shape == (n, 48) and rec.dtype == np.uint32 and sums.shape == (n, 2)
    np.testing.assert_array_equal(rec[:, :42], stats['hist'])
    np.testing.assert_array_equal(rec[:, 42] & np.uint32(0x7FFFFFFF), count)
    np.testing.assert_array_equal(rec[:, :42].sum(axis=1, dtype=np.int64), count)
    ne = count > 0
    np.testing.assert_array_equal(rec[ne, 43], f2ord(stats['min'][ne]))
    np.testing.assert_array_equal(rec[ne, 44], f2ord(stats['max'][ne]))
    piv = rec[:, 45].view(np.float32).astype(np.float64)
    assert np.all((piv[ne] >= stats['min'][ne]) & (piv[ne] <= stats['max'][ne]))
    np.testing.assert_array_equal(rec[:, 46:48], 0)
    d = decode_stats(sums, rec)
    np.testing.assert_allclose(d['mean'], stats['mean'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d['m2'] / np.maximum(count, 1), stats['var'], rtol=1e-5, atol=0)


def _both_reduces(lab, data, ref, lo=0.0, hi=1.0, **kw):
    """One input through the statistics-writing reduce (keep_stats) and the
    packed-histogram reduce, each against the oracle's (edges, features, stats)."""
    e_ref, f_ref, stats = ref
    out = rag.rag_features(lab, data, hist_range=(lo, hi), keep_stats=True, **kw)
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_stats(out, stats)
    check_features(out['features'], f_ref, lo, hi)
    out = rag.rag_features(lab, data, hist_range=(lo, hi), **kw)
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_features(out['features'], f_ref, lo, hi)
    return stats


# ------------------------------------------------ boundary maps, both binnings
@pytest.fixture(scope='module')
def wide_volume():
    lab, bnd = S.generate((16, 30, 34), cell=5, seed=2)
    return lab, bnd, (bnd * 3.0 - 1.0).astype(np.float32)      # [-1, 2]: both outlier slots fill


@pytest.mark.parametrize('lo,hi', [(0.0, 1.0), (-1.0, 2.0)])
def test_boundary_f32_stats(gpu, wide_volume, lo, hi):
    """[0, 1] takes the scan's FAST40 binning, [-1, 2] the general one."""
    lab, _, data = wide_volume
    stats = _both_reduces(lab, data, O.boundary_features(lab, data, lo=lo, hi=hi, return_stats=True), lo, hi)
    if (lo, hi) == (0.0, 1.0):
        assert stats['hist'][:, 0].sum() > 0 and stats['hist'][:, 41].sum() > 0


def test_boundary_u8_stats(gpu, wide_volume):
    lab, bnd, _ = wide_volume
    data = np.round(bnd * 255).astype(np.uint8)
    _both_reduces(lab, data, O.boundary_features(lab, data, return_stats=True))


@pytest.mark.parametrize('offsets', [S.NN_OFFSETS, S.LR_OFFSETS], ids=['nn', 'long_range'])
def test_affinity_stats(gpu, offsets):
    lab, bnd = S.generate((12, 40, 33), cell=5, seed=4)
    affs = S.affinities_from_boundary(bnd, offsets)
    _both_reduces(lab, affs, O.affinity_features(lab, affs, offsets, return_stats=True), offsets=offsets)


# ------------------------------------------------------------------ bin edges
def _bin_edge_volume():
    """Samples k/40 (k = 0 .. 40, 1.0 included: bin 39), a third of them one
    float up and a third one float down (1.0's upper neighbour is a right
    outlier, 0.0's lower neighbour truncates into bin 0), a sprinkle in
    (-1/40, 0), which truncation toward zero keeps in bin 0; salt-and-pepper
    labels, so each of the ~435 edges gets many samples."""
    rng = np.random.default_rng(40)
    lab = rng.integers(0, 30, (8, 24, 40)).astype(np.uint64)
    x = (rng.integers(0, 41, lab.shape) / 40.0).astype(np.float32)
    side = rng.integers(0, 3, lab.shape)
    x = np.where(side == 1, np.nextafter(x, np.float32(np.inf)), x)
    x = np.where(side == 2, np.nextafter(x, np.float32(-np.inf)), x)
    neg = rng.random(lab.shape) < 0.03
    x = np.where(neg, -(rng.random(lab.shape) * 0.0248 + 1e-4), x).astype(np.float32)
    return lab, x


@pytest.mark.parametrize('lo,hi', [(0.0, 1.0), (-1.0, 2.0)])
def test_bin_edge_samples(gpu, lo, hi):
    lab, x = _bin_edge_volume()
    data = x if lo == 0.0 else (np.float32(3.0) * x - np.float32(1.0)).astype(np.float32)
    ref = O.boundary_features(lab, data, lo=lo, hi=hi, return_stats=True)
    stats = _both_reduces(lab, data, ref, lo, hi)
    if lo == 0.0:     # the volume holds what it claims: both outlier slots, and negatives inside bin 0
        slots = O.histogram_slots(x, 0.0, 1.0)
        assert (slots[x < 0] == 1).sum() > 100 and (slots == 41).sum() > 20 and (slots[x == 1.0] == 40).sum() > 20
        assert not (slots == 0).any() and stats['hist'][:, 41].sum() > 0 and stats['count'].min() > 30


# ---------------------------------------------------------------------- merge
@pytest.mark.parametrize('outliers', [False, True])
def test_merged_slabs_stats(gpu, outliers):
    """ctg_merge_stats over two z-slabs' rows: the merged rows are the
    whole volume's statistics -- on a [0, 1] map, and on one stretched to
    [-1, 2] so that both outlier slots of the merged rows fill."""
    lab, bnd = S.generate((30, 40, 44), cell=5, seed=14)
    if outliers:
        bnd = (bnd * 3.0 - 1.0).astype(np.float32)
    e_ref, f_ref, stats = O.boundary_features(lab, bnd, return_stats=True)
    assert not outliers or (stats['hist'][:, 0].sum() > 0 and stats['hist'][:, 41].sum() > 0)
    a = rag.rag_features(lab[:13], bnd[:13], keep_stats=True)
    b = rag.rag_features(lab[12:], bnd[12:], own_begin=(1, 0, 0), keep_stats=True)
    m = rag.merge_stats(np.concatenate([a['edges'], b['edges']]), np.concatenate([a['sums'], b['sums']]),
                        np.concatenate([a['records'], b['records']]), keep_stats=True)
    np.testing.assert_array_equal(m['edges'], e_ref)
    check_stats(m, stats)
    check_features(m['features'], f_ref)
    # the slabs' own rows, against the oracle's statistics of their owned faces
    e_a, _, st_a = O.boundary_features(lab[:13], bnd[:13], return_stats=True)
    np.testing.assert_array_equal(a['edges'], e_a)
    check_stats(a, st_a)
    e_b, _, st_b = O.boundary_features(lab[12:], bnd[12:], own_begin=(1, 0, 0), return_stats=True)
    np.testing.assert_array_equal(b['edges'], e_b)
    check_stats(b, st_b)


@pytest.mark.parametrize('defer', [False, True])
def test_exchange_merge_with_outliers(gpu, defer):
    """The multi-GPU merge (ctg_mgpu_merge over exchanged rows, two z-slabs
    on one GPU: tests/exchange_sim.py) on a map stretched to [-1, 2]: rows
    written by the local calls, and rows rebuilt from the records
    (CTG_DEFER_STATS), keep both outlier slots -- the oracle's features of the
    whole volume."""
    import torch
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = S.generate((20, 40, 44), cell=5, seed=24)
    data = (bnd * 3.0 - 1.0).astype(np.float32)
    e_ref, f_ref, stats = O.boundary_features(lab, data, return_stats=True)
    assert stats['hist'][:, 0].sum() > 0 and stats['hist'][:, 41].sum() > 0
    lab_t, data_t = torch.from_numpy(lab.view(np.int64)).cuda(), torch.from_numpy(data).cuda()
    shards = simulate(cdist.HipBackend(defer_stats=defer), lab_t, data_t, 2, fresh=defer)
    np.testing.assert_array_equal(np.concatenate([x.edges() for x in shards]), e_ref)
    check_features(np.concatenate([x.features() for x in shards]), f_ref)


# ------------------------------------------- the packed reduce's 2^16 threshold
def _threshold_values(n, values):
    """n samples.  'mixed': 0.33 (slot 14, the low half of its packed word),
    ~1 % of them 0.36 (slot 15, the high half of the same word), three each of
    -0.5 and 1.5 (the outlier slots).  'one_slot': every sample 0.33 -- with
    2^16 samples the low half is exactly full + 1, so an edge wrongly kept in
    u16 halves reads slot 14 = 0 and slot 15 = 1."""
    v = np.full(n, 0.33, np.float32)
    if values == 'mixed':
        rng = np.random.default_rng(n)
        v[rng.random(n) < 0.01] = 0.36
        out = rng.choice(n, 6, replace=False)
        v[out[:3]] = -0.5
        v[out[3:]] = 1.5
    return v


def _check_one_edge(lab, data, ref, n, **kw):
    e_ref, f_ref, stats = ref
    assert e_ref.tolist() == [[1, 2]] and stats['count'].tolist() == [n]
    assert stats['hist'][0, 14] >= 0.98 * n and stats['hist'][0].sum() == n
    out = rag.rag_features(lab, data, **kw)                      # packed-histogram reduce (+ its heavy redo)
    np.testing.assert_array_equal(out['edges'], e_ref)
    assert out['features'][0, 9] == n
    check_features(out['features'], f_ref)
    out = rag.rag_features(lab, data, keep_stats=True, **kw)     # wide reduce, statistics row
    np.testing.assert_array_equal(out['edges'], e_ref)
    assert out['features'][0, 9] == n
    check_features(out['features'], f_ref)
    check_stats(out, stats)


@pytest.mark.parametrize('tile_z', [None, '64'])
@pytest.mark.parametrize('values', ['mixed', 'one_slot'])
@pytest.mark.parametrize('shape', [(2, 255, 257), (2, 256, 256), (2, 257, 256)])
def test_one_edge_at_the_u16_threshold_affinity(gpu, monkeypatch, shape, values, tile_z):
    """One z-offset channel over two planes of two labels: a single edge of
    Y * X samples -- 65 535 (the largest edge the packed-histogram reduce keeps
    in u16 halves), 65 536 (the smallest it hands to the wide redo), 65 792 --
    (nearly) all in slot 14, whose carry would land in slot 15.  A threshold
    one off or a carry between the halves moves the quantiles by a visible
    part of a bin."""
    if tile_z:
        monkeypatch.setenv('CTG_TILE_Z', tile_z)
    n = shape[1] * shape[2]
    lab = np.ones(shape, np.uint64)
    lab[1] = 2
    offsets = [[-1, 0, 0]]
    affs = np.full((1,) + shape, 0.33, np.float32)
    affs[0, 1] = _threshold_values(n, values).reshape(shape[1:])
    _check_one_edge(lab, affs, O.affinity_features(lab, affs, offsets, return_stats=True), n, offsets=offsets)


@pytest.mark.parametrize('tile_z', [None, '64'])
@pytest.mark.parametrize('values', ['mixed', 'one_slot'])
def test_one_edge_at_the_u16_threshold_boundary(gpu, monkeypatch, values, tile_z):
    """The same with a boundary map: 128 x 256 z faces at two samples a face,
    65 536 samples."""
    if tile_z:
        monkeypatch.setenv('CTG_TILE_Z', tile_z)
    shape = (2, 128, 256)
    n = 2 * shape[1] * shape[2]
    assert n == 65536
    lab = np.ones(shape, np.uint64)
    lab[1] = 2
    bnd = _threshold_values(n, values).reshape(shape)
    _check_one_edge(lab, bnd, O.boundary_features(lab, bnd, return_stats=True), n)

