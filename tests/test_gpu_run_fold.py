"""The record back half of label overlaps, segment morphology and region
features (ctg_run_fold.h: run_fold and its three policies) on segments that
start and end at lanes 0, 62, 63 and 64 of a wave, straddle one, two and eight
waves and cross workgroup boundaries -- the existing suites' labels own a
handful of records each and hardly get there.

Through the merge entries the sorted position of every row is known from its
id: rows of one id are contiguous after the sort, in input order (the sort is
stable), so the multiplicities below place the segments.  Through the scan
entries a volume of 300 tiles of one or two labels gives 300 records of one or
two keys.  Every comparison is exact, against integer or exactly representable
float sums computed here with numpy."""
import numpy as np
import pytest

from cluster_tools_amd import rag

pytestmark = pytest.mark.gpu

# rows per id, ids ascending: the segments start at sorted positions 0, 1, 63, 64, 128, 193, 256, 511, 512, 768, 1025
MULT = np.array([1, 62, 1, 64, 65, 63, 255, 1, 256, 257, 513])
IDS = np.array([3, 7, 8, 20, 21, 50, 51, 60, 61, 1000, 5000], dtype=np.uint64)
TILE = (16, 8, 64)   # a tile of the scans (z, y, x)
NT = 300


def layout(mult, ids, seed=11):
    """(id of every row, its rank among the rows of its id), the rows in a shuffled order."""
    idx = np.repeat(np.arange(len(mult)), mult)
    idx = idx[np.random.default_rng(seed).permutation(idx.shape[0])]
    rank = np.zeros(idx.shape[0], dtype=np.int64)
    for j in range(len(mult)):
        rank[idx == j] = np.arange(mult[j])
    return idx, rank, ids[idx]


# (case, with a row of count 0 in the middle of its longest segment)
ZERO_CASES = [('wave_edges', False), ('wave_edges', True), ('one_row', False), ('one_id_300', False), ('one_id_300', True)]
CASES = {
    'wave_edges': (MULT, IDS),
    'one_row': (np.array([1]), np.array([9], dtype=np.uint64)),
    'one_id_300': (np.array([300]), np.array([4], dtype=np.uint64)),
}


def f2ord(x):
    """The order-preserving u32 word of a float32 (-0.0 below +0.0)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ the merge entries
@pytest.mark.parametrize('case', sorted(CASES))
def test_merge_overlaps_segments(case):
    mult, ids = CASES[case]
    idx, _, _ = layout(mult, ids)
    # several rows share a node: a = id // 10, b = id, so the node table and the row offsets fold too
    a, b = ids // np.uint64(10), ids
    rng = np.random.default_rng(5)
    # counts near 2^31: a segment of 65 rows, which crosses a wave, sums past 2^32
    counts = rng.integers(1 << 30, 1 << 31, size=idx.shape[0]).astype(np.uint64)
    out = rag.merge_overlaps(np.stack([a[idx], b[idx]], 1), counts)
    want = np.zeros(len(mult), dtype=np.uint64)
    np.add.at(want, idx, counts)
    np.testing.assert_array_equal(out['pairs'], np.stack([a, b], 1))
    np.testing.assert_array_equal(out['counts'], want)
    np.testing.assert_array_equal(out['nodes'], np.unique(a))
    if case == 'wave_edges':
        assert int(want[4]) > 1 << 32
    # the row offsets, through the arg-max: per node the row with the largest sum, ties to the smallest b
    top = int(a.max()) + 2
    best_l, best_c = rag.max_overlaps(dict(pairs=out['pairs'], counts=out['counts']), 0, top)
    for node in range(top):
        rows = np.flatnonzero(a == np.uint64(node))
        if rows.size == 0:
            assert best_l[node] == 0 and best_c[node] == 0
        else:
            k = rows[np.argmax(want[rows])]
            assert best_l[node] == b[k] and best_c[node] == want[k]


def morph_rows(mult, ids, zero_row):
    """Partial morphology rows and the moments they merge to.  The first row of
    a segment holds its smallest box corner and the last its largest, so where a
    segment crosses a wave the minimum and the maximum sit in different waves."""
    idx, rank, rid = layout(mult, ids)
    n = idx.shape[0]
    rng = np.random.default_rng(6)
    size = rng.integers(1, 50, size=n)
    sums = rng.integers(0, 1 << 20, size=(n, 3)) * size[:, None]   # com = sum / size: an integer, exact
    lo = rng.integers(100, 200, size=(n, 3))
    hi = lo + rng.integers(0, 50, size=(n, 3))
    lo[rank == 0] = 5
    hi[rank == mult[idx] - 1] = 900
    if zero_row:   # a row without voxels in the middle of the longest segment: its box must not count
        z = np.flatnonzero((idx == np.argmax(mult)) & (rank == mult.max() // 2))[0]
        size[z], sums[z], lo[z], hi[z] = 0, 0, 0, 1 << 20
    rows = np.zeros((n, 11), dtype=np.float64)
    rows[:, 0], rows[:, 1] = rid, size
    rows[:, 2:5] = sums / np.maximum(size, 1)[:, None]
    rows[:, 5:8], rows[:, 8:11] = lo, hi
    live = size > 0
    want = np.zeros((len(mult), 10), dtype=np.uint64)
    np.add.at(want[:, 0], idx, size.astype(np.uint64))
    for c in range(3):
        np.add.at(want[:, 1 + c], idx, sums[:, c].astype(np.uint64))
        mn = np.full(len(mult), np.iinfo(np.int64).max)
        mx = np.zeros(len(mult), dtype=np.int64)
        np.minimum.at(mn, idx[live], lo[live, c])
        np.maximum.at(mx, idx[live], hi[live, c])
        want[:, 4 + c], want[:, 7 + c] = mn, mx
    return rows, want


@pytest.mark.parametrize('case,zero_row', ZERO_CASES)
def test_merge_morphology_segments(case, zero_row):
    mult, ids = CASES[case]
    rows, want = morph_rows(mult, ids, zero_row)
    out = rag.merge_morphology(rows)
    np.testing.assert_array_equal(out['nodes'], ids)
    np.testing.assert_array_equal(out['moments'], want)
    np.testing.assert_array_equal(out['rows'][:, 1], want[:, 0].astype(np.float64))
    np.testing.assert_array_equal(out['rows'][:, 2:5], want[:, 1:4].astype(np.float64) / want[:, :1].astype(np.float64))
    if case == 'wave_edges':
        assert (want[:, 4:7] == 5).all() and (want[:, 7:10] == 900).all()


def region_rows(mult, ids, zero_row):
    """Partial region rows [id, count, sum, min, max] on the k / 256 grid, |x| <
    2^10 -- every partial sum is exact in any order -- with negative values, and
    with both zeros where they decide the ordered minimum / maximum."""
    idx, rank, rid = layout(mult, ids)
    n = idx.shape[0]
    rng = np.random.default_rng(7)
    count = rng.integers(1, 100, size=n)
    total = rng.integers(-(1 << 18) + 1, 1 << 18, size=n) / 256.0
    lo = (rng.integers(-(1 << 18) + 1, 0, size=n) / 256.0).astype(np.float32)
    hi = (rng.integers(1, 1 << 18, size=n) / 256.0).astype(np.float32)
    if len(mult) > 5:
        # segment 4 (65 rows: crosses a wave): minima +0.0 but one -0.0 at its far end -> -0.0
        lo[idx == 4] = 0.0
        lo[(idx == 4) & (rank == mult[4] - 1)] = -0.0
        # segment 5: maxima -0.0 but one +0.0 at its start -> +0.0
        hi[idx == 5] = -0.0
        hi[(idx == 5) & (rank == 0)] = 0.0
    if zero_row:   # a row without voxels in the middle of the longest segment: nothing of it counts
        z = np.flatnonzero((idx == np.argmax(mult)) & (rank == mult.max() // 2))[0]
        count[z], total[z], lo[z], hi[z] = 0, 0.0, -2000.0, 2000.0
    rows = np.stack([rid.astype(np.float64), count.astype(np.float64), total, lo.astype(np.float64),
                     hi.astype(np.float64)], 1)
    live = count > 0
    want_n = np.zeros(len(mult), dtype=np.uint64)
    want_s = np.zeros(len(mult), dtype=np.float64)
    np.add.at(want_n, idx, count.astype(np.uint64))
    np.add.at(want_s, idx, total)   # (exact: multiples of 2^-8 below 2^29)
    mn = np.full(len(mult), 0xFFFFFFFF, dtype=np.uint32)
    mx = np.zeros(len(mult), dtype=np.uint32)
    np.minimum.at(mn, idx[live], f2ord(lo[live]))
    np.maximum.at(mx, idx[live], f2ord(hi[live]))
    return rows, want_n, want_s, mn, mx


@pytest.mark.parametrize('case,zero_row', ZERO_CASES)
def test_merge_region_features_segments(case, zero_row):
    mult, ids = CASES[case]
    rows, want_n, want_s, mn, mx = region_rows(mult, ids, zero_row)
    out = rag.merge_region_features(rows)
    np.testing.assert_array_equal(out['nodes'], ids)
    np.testing.assert_array_equal(out['counts'], want_n)
    np.testing.assert_array_equal(out['sums'], want_s)
    np.testing.assert_array_equal(f2ord(out['minmax'][:, 0]), mn)
    np.testing.assert_array_equal(f2ord(out['minmax'][:, 1]), mx)
    if case == 'wave_edges':   # the signs of the zeros
        assert bits(out['minmax'][4, 0]) == 0x80000000 and bits(out['minmax'][5, 1]) == 0


# ------------------------------------------------------------------ the scan entries
def tile_labels(kind):
    """(16, 8, 64 * 300) uint32: one label, two labels alternating per tile, or
    those with every fifth tile holding label 0."""
    t = np.arange(NT)
    per_tile = {'one': np.full(NT, 7), 'two': 5 + 6 * (t % 2), 'holes': np.where(t % 5 == 0, 0, 5 + 6 * (t % 2))}[kind]
    return np.ascontiguousarray(np.broadcast_to(np.repeat(per_tile, TILE[2]).astype(np.uint32),
                                                TILE[:2] + (NT * TILE[2],)))


@pytest.mark.parametrize('kind', ['one', 'two'])
def test_scan_overlaps_long_segments(kind):
    labels = tile_labels(kind)
    values = np.full(labels.shape, 3, dtype=np.uint32)
    out = rag.label_overlaps(labels, values)
    ids, tiles = np.unique(labels[0, 0, ::TILE[2]], return_counts=True)
    np.testing.assert_array_equal(out['pairs'], np.stack([ids, np.full_like(ids, 3)], 1).astype(np.uint64))
    np.testing.assert_array_equal(out['counts'], (tiles * int(np.prod(TILE))).astype(np.uint64))
    np.testing.assert_array_equal(out['nodes'], ids.astype(np.uint64))
    assert out['n_records'] == NT   # one record per tile: segments of 300, or two of 150


@pytest.mark.parametrize('kind', ['one', 'two'])
def test_scan_morphology_long_segments(kind):
    labels = tile_labels(kind)
    out = rag.morphology(labels)
    Z, Y, X = labels.shape
    row = labels[0, 0].astype(np.int64)
    ids = np.unique(row)
    want = np.zeros((ids.shape[0], 10), dtype=np.uint64)
    for j, a in enumerate(ids):   # the labels depend on x alone
        xs = np.flatnonzero(row == a)
        want[j] = [Z * Y * xs.size, Y * xs.size * np.arange(Z).sum(), Z * xs.size * np.arange(Y).sum(), Z * Y * xs.sum(),
                   0, 0, xs.min(), Z - 1, Y - 1, xs.max()]
    np.testing.assert_array_equal(out['nodes'], ids.astype(np.uint64))
    np.testing.assert_array_equal(out['moments'], want)
    assert out['n_records'] == NT


@pytest.mark.parametrize('kind', ['one', 'two', 'holes'])
def test_scan_region_features_long_segments(kind):
    labels = tile_labels(kind)
    data = (np.random.default_rng(8).integers(-(1 << 10), (1 << 10) + 1, size=labels.shape) / 256.0).astype(np.float32)
    ignore = 0 if kind == 'holes' else None
    out = rag.region_features(labels, data, ignore_label=ignore)
    ids = np.unique(labels[0, 0])
    ids = ids[ids != 0] if kind == 'holes' else ids
    np.testing.assert_array_equal(out['nodes'], ids.astype(np.uint64))
    for j, a in enumerate(ids):
        x = data[labels == a]
        assert out['counts'][j] == x.size
        assert out['sums'][j] == x.astype(np.float64).sum()   # (exact: multiples of 2^-8 below 2^24)
        assert out['minmax'][j, 0] == x.min() and out['minmax'][j, 1] == x.max()
    assert out['n_records'] == NT - (NT // 5 if kind == 'holes' else 0)
