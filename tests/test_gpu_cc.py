"""rag.threshold_components and rag.merge_assignments on the GPU (csrc/ctg_cc.hip)
against the oracle of tests/cc_cases.py, a dict union-find and the golden
fixture.  Every comparison is exact: the labels with their numbering and the
component count."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import _lib, rag
from tests import cc_cases as C

pytestmark = pytest.mark.gpu

U64 = np.uint64
SHAPES = [(1, 1, 1), (1, 1, 130), (16, 8, 64), (17, 9, 65), (33, 17, 129)]


def as_data(fg):
    """A float32 map whose samples above 0.5 are the foreground (no normalisation needed)."""
    return np.where(fg, np.float32(0.75), np.float32(0.25))


def label(fg, c, **kw):
    return rag.threshold_components(as_data(fg), 0.5, connectivity=c, normalize=False, **kw)


def check(fg, c, **kw):
    want, n = C.oracle_label(fg, c)
    got, m = label(fg, c, **kw)
    assert got.dtype == U64 and got.shape == fg.shape
    assert m == n
    assert_array_equal(got, want)
    return n


# --------------------------------------------------------------------------- shapes and densities
@pytest.mark.parametrize('c', [1, 2, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_shapes(gpu, shape, c):
    """One voxel past a tile edge on every axis, exactly one tile, and the degenerate shapes."""
    for p in (0.3, 0.6):
        check(C.random_fg(shape, p, seed=shape[2] + c), c)


@pytest.mark.parametrize('c,p', [(1, 0.25), (1, 0.45), (2, 0.08), (2, 0.15), (3, 0.08), (3, 0.15)])
@pytest.mark.parametrize('shape', [(17, 9, 65), (33, 17, 129)])
def test_random_maps(gpu, shape, c, p):
    """Densities at which the oracle alone yields many components (above about
    0.5 with c >= 2 the volume is one component, which tests nothing)."""
    assert check(C.random_fg(shape, p, seed=shape[0] + c), c) >= 20


@pytest.mark.parametrize('c', [1, 2, 3])
def test_all_foreground_and_all_background(gpu, c):
    for shape in SHAPES:
        got, n = label(np.ones(shape, dtype=bool), c)
        assert n == 1 and (got == 1).all()
        got, n = label(np.zeros(shape, dtype=bool), c)
        assert n == 0 and not got.any()


def test_checkerboard(gpu):
    shape = (18, 10, 66)
    fg = C.checkerboard(shape)
    got, n = label(fg, 1)
    assert n == np.prod(shape) // 2                       # every foreground voxel alone
    assert_array_equal(got[fg], np.arange(1, n + 1, dtype=U64))
    assert check(fg, 2) == 1 and check(fg, 3) == 1


@pytest.mark.parametrize('c', [1, 2, 3])
def test_serpentine(gpu, c):
    """One one-voxel path through (3, 16, 130): chains of hundreds of nodes
    across dozens of seam crossings."""
    fg = C.serpentine()
    assert check(fg, c) == 1
    # the same path cut once: two components, the second numbered from its first voxel
    fg[0, 6, 70] = False
    assert check(fg, 1) == 2


@pytest.mark.parametrize('c', [1, 2, 3])
def test_root_moves_across_the_seams(gpu, c):
    """The 'U': its first raster voxel lies in the last x tile and the arm in the
    first tile learns of it only through the seam pass."""
    fg = C.u_shape()
    assert check(fg, c) == 1
    fg[3, 2, 5] = True                                    # and a later component keeps its number
    assert check(fg, c) == 2


@pytest.mark.parametrize('c', [1, 2, 3])
def test_two_runs_joined_by_the_row_below(gpu, c):
    fg = np.zeros((2, 3, 70), dtype=bool)
    fg[0, 0, 2:9] = fg[0, 0, 20:66] = True
    fg[0, 1, 8:21] = True
    assert check(fg, c) == 1
    fg[0, 1, 14] = False                                  # the bridge cut: the two runs part again
    assert check(fg, c) == 2


def test_corner_and_edge_contacts_across_tile_borders(gpu):
    corner = np.zeros((17, 9, 66), dtype=bool)
    corner[15, 7, 63] = corner[16, 8, 64] = True          # a corner contact across the z, y and x borders at once
    assert check(corner, 1) == 2 and check(corner, 2) == 2 and check(corner, 3) == 1
    for a, b in (((15, 7, 10), (16, 8, 10)), ((15, 3, 63), (16, 3, 64)), ((4, 7, 63), (4, 8, 64)),
                 ((15, 8, 64), (16, 7, 64)), ((4, 7, 64), (4, 8, 63))):
        edge = np.zeros((17, 9, 66), dtype=bool)          # an edge contact across two borders
        edge[a] = edge[b] = True
        assert check(edge, 1) == 2 and check(edge, 2) == 1 and check(edge, 3) == 1
    for a, b in (((15, 8, 64), (16, 7, 63)), ((15, 7, 64), (16, 8, 63)), ((15, 8, 63), (16, 7, 64))):
        corner = np.zeros((17, 9, 66), dtype=bool)        # the other corner directions
        corner[a] = corner[b] = True
        assert check(corner, 2) == 2 and check(corner, 3) == 1


# --------------------------------------------------------------------------- inputs, modes, normalisation
@pytest.fixture(scope='module')
def noise():
    return np.random.default_rng(3).random((19, 11, 70)).astype(np.float32)


@pytest.mark.parametrize('mode', ['greater', 'less', 'equal'])
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_modes_and_types(gpu, noise, mode, normalize, dtype):
    data = (noise * 6).astype(np.uint8) if dtype == np.uint8 else np.round(noise * 8) / np.float32(8) + np.float32(2)
    data = data.astype(dtype)
    # a threshold that some normalised / raw samples equal
    t = float(C.normalize(data).ravel()[5]) if normalize else float(data.ravel()[5])
    fg = C.foreground(data, t, mode, normalize)
    assert 0 < fg.sum() < fg.size
    for c in (1, 3):
        want, n = C.oracle_label(fg, c)
        got, m = rag.threshold_components(data, t, mode=mode, normalize=normalize, connectivity=c)
        assert m == n
        assert_array_equal(got, want)


def test_golden(gpu):
    g = C.golden()
    for case in g['cases']:
        got, n = rag.threshold_components(g['values'], case['threshold'], mode=case['mode'],
                                          mask=g['mask'] if case['mask'] else None, normalize=case['normalize'],
                                          connectivity=case['connectivity'])
        assert n == case['n'], case
        assert_array_equal(got, case['labels'])
    # ... and as uint8 samples
    got, n = rag.threshold_components(g['values'].astype(np.uint8), 0.4, connectivity=2)
    assert n == 2
    assert_array_equal(got, g['cases'][1]['labels'])


def test_sub_box(gpu, noise):
    b, e = (2, 3, 5), (19, 10, 70)
    bb = tuple(slice(x, y) for x, y in zip(b, e))
    mask = np.random.default_rng(8).random(noise.shape) < 0.9
    for normalize in (True, False):
        t = 0.6
        fg = C.foreground(noise[bb], t, 'greater', normalize, mask[bb])      # normalised over the box alone
        want, n = C.oracle_label(fg, 1)
        got, m = rag.threshold_components(noise, t, mask=mask, normalize=normalize, connectivity=1, begin=b, end=e)
        assert got.shape == want.shape and m == n
        assert_array_equal(got, want)
    got, m = rag.threshold_components(noise, 0.5, begin=(3, 3, 3), end=(3, 9, 9))
    assert got.shape == (0, 6, 6) and m == 0


def test_mask(gpu, noise):
    mask = np.ones(noise.shape, dtype=bool)
    mask[3:9, 2:7, 10:66] = False                         # a hole
    mask[::3, ::2, ::5] = False                           # and pinholes
    fg = C.foreground(noise, 0.4, 'greater', True, mask)
    for m in (mask, mask.astype(np.uint8) * 7):
        want, n = C.oracle_label(fg, 3)
        got, k = rag.threshold_components(noise, 0.4, mask=m, connectivity=3)
        assert k == n
        assert_array_equal(got, want)
    got, k = rag.threshold_components(noise, 0.4, mask=np.zeros(noise.shape, dtype=bool))
    assert k == 0 and not got.any()


def test_device_inputs_and_outputs(gpu, noise):
    import torch
    mask = np.random.default_rng(9).random(noise.shape) < 0.8
    fg = C.foreground(noise, 0.55, 'greater', True, mask)
    want, n = C.oracle_label(fg, 2)
    d, m = torch.from_numpy(noise).cuda(), torch.from_numpy(mask).cuda()
    got, k = rag.threshold_components(d, 0.55, mask=m, connectivity=2)
    assert got.is_cuda and got.dtype == torch.int64 and k == n
    assert_array_equal(got.cpu().numpy().view(U64), want)
    out = torch.full(noise.shape, -1, dtype=torch.int64, device='cuda')
    got, k = rag.threshold_components(d, 0.55, mask=m, connectivity=2, out=out)
    assert got is out and k == n
    assert_array_equal(out.cpu().numpy().view(U64), want)
    host_out = np.full(noise.shape, 9, dtype=U64)
    got, k = rag.threshold_components(noise, 0.55, mask=mask, connectivity=2, out=host_out)
    assert got is host_out
    assert_array_equal(host_out, want)
    # an output that is only 8-byte aligned takes the narrow stores
    flat = torch.full((noise.size + 1,), -1, dtype=torch.int64, device='cuda')
    odd = flat[1:].view(noise.shape)
    rag.threshold_components(d, 0.55, mask=m, connectivity=2, out=odd)
    assert_array_equal(odd.cpu().numpy().view(U64), want)
    assert int(flat[0]) == -1


def test_normalised_samples_one_ulp_around_the_threshold(gpu):
    """Samples whose normalised value is a threshold and its two float32
    neighbours, for eight thresholds: the expected values come from numpy's
    float32 -= and /=.  A reciprocal multiply in the kernel moves some of them to
    the other side -- the test checks on the CPU that it would notice."""
    rng = np.random.default_rng(17)
    # minimum 2^-6 and range 3: x - mn in [1.5, 2) steps by 2^-23, so the quotients step by less than the float32
    # spacing of [0.5, 2/3) and each of a threshold's neighbours has a preimage
    mn, mx = np.float32(2.0 ** -6), np.float32(3.0)
    x = (rng.random((9, 10, 66)).astype(np.float32) * np.float32(2.9) + np.float32(0.05)).astype(np.float32)
    x.ravel()[0], x.ravel()[1] = mn, mn + mx               # the box's range
    thresholds, k = [], 100
    for y in np.linspace(1.55, 1.95, 8, dtype=np.float32):
        t = np.float32(y / mx)
        near = {np.nextafter(t, np.float32(0)), t, np.nextafter(t, np.float32(1))}
        cand, seen = np.float32(t * mx + mn), set()
        for _ in range(8):
            cand = np.nextafter(cand, np.float32(0))
        for _ in range(16):                                # the float32 neighbourhood of the preimage
            r = np.float32(np.float32(cand - mn) / mx)
            if r in near:
                x.ravel()[k] = cand
                seen.add(r)
                k += 7
            cand = np.nextafter(cand, np.float32(4))
        assert seen == near, 'a neighbour of the threshold has no preimage'
        thresholds.append(t)
    assert x.min() == mn and np.float32(x.max() - mn) == mx
    wrong = np.float32(x - mn) * np.float32(np.float32(1) / mx)        # what a reciprocal multiply would compute
    assert any(((wrong > t) != (C.normalize(x) > t)).any() for t in thresholds)
    for t in thresholds:
        for mode in ('greater', 'less', 'equal'):
            fg = C.foreground(x, t, mode, True)
            want, n = C.oracle_label(fg, 1)
            got, m = rag.threshold_components(x, float(t), mode=mode, connectivity=1)
            assert_array_equal(got != 0, fg)
            assert m == n
            assert_array_equal(got, want)


def test_nan_in_a_normalised_box_gives_the_empty_result(gpu, noise):
    x = noise.copy()
    x[7, 3, 40] = np.nan
    for mode in ('greater', 'less', 'equal'):
        got, n = rag.threshold_components(x, 0.5, mode=mode)
        assert n == 0 and not got.any()
    # without normalisation the NaN voxel alone is background
    for mode in ('greater', 'less'):
        fg = C.foreground(x, 0.5, mode, False)
        assert not fg[7, 3, 40]
        want, n = C.oracle_label(fg, 1)
        got, m = rag.threshold_components(x, 0.5, mode=mode, normalize=False, connectivity=1)
        assert m == n
        assert_array_equal(got, want)
    # a box that leaves the NaN out is labelled as usual
    got, n = rag.threshold_components(x, 0.5, begin=(8, 0, 0), end=(19, 11, 70), connectivity=1)
    want, m = C.oracle_label(C.foreground(x[8:], 0.5, 'greater', True), 1)
    assert n == m
    assert_array_equal(got, want)


# --------------------------------------------------------------------------- merge_assignments
@pytest.fixture(scope='module')
def merge_cases():
    rng = np.random.default_rng(23)
    n = 100000
    chain = rng.permutation(np.stack([np.arange(1, 10000), np.arange(2, 10001)], 1))
    star = np.stack([np.full(5000, 77), rng.permutation(np.arange(100, 5100))], 1)
    return n, dict(random=rng.integers(1, n, size=(60000, 2)),
                   chain=chain,
                   star=star,
                   repeats=np.array([[5, 9], [9, 5], [5, 9], [9, 11], [11, 5], [n - 1, 9], [n - 1, n - 1]]),
                   mixed=np.concatenate([chain[:3000] + 20000, star + 40000, rng.integers(70000, n, size=(9000, 2))]))


@pytest.mark.parametrize('name', ['random', 'chain', 'star', 'repeats', 'mixed'])
def test_merge_assignments(gpu, merge_cases, name):
    n, cases = merge_cases
    pairs = cases[name].astype(U64)
    want, max_id = C.merge_table(pairs, n)
    fast, fast_max = C.merge_table_fast(pairs, n)          # the oracle of the cases past one scan step
    assert fast_max == max_id
    assert_array_equal(fast, want)
    got, m = rag.merge_assignments(pairs, n)
    assert got.dtype == U64 and m == max_id
    assert_array_equal(got, want)
    assert got[0] == 0 and (got[1:] != 0).all()
    # ids that appear in no pair keep their rank order
    free = np.setdiff1d(np.arange(1, n, dtype=np.int64), pairs.ravel().astype(np.int64))
    assert (np.diff(got[free].astype(np.int64)) > 0).all()


def test_merge_assignments_edges(gpu):
    got, m = rag.merge_assignments(np.zeros((0, 2), dtype=U64), 1000)
    assert m == 999
    assert_array_equal(got, np.arange(1000, dtype=U64))                      # no pairs: the identity
    got, m = rag.merge_assignments(np.zeros((0, 2), dtype=U64), 1)
    assert m == 0 and got.tolist() == [0]
    got, m = rag.merge_assignments(np.array([[1, 2]], dtype=U64), 3)
    assert m == 1 and got.tolist() == [0, 1, 1]
    got, m = rag.merge_assignments(np.array([[1, 2049], [4097, 2]], dtype=np.int64), 5000)       # across numbering segments
    want, k = C.merge_table([[1, 2049], [4097, 2]], 5000)
    assert m == k
    assert_array_equal(got, want)


def test_merge_assignments_device(gpu, merge_cases):
    import torch
    n, cases = merge_cases
    pairs = cases['mixed'].astype(np.int64)
    want, max_id = C.merge_table(pairs, n)
    got, m = rag.merge_assignments(torch.from_numpy(pairs).cuda(), n)
    assert got.is_cuda and got.dtype == torch.int64 and m == max_id
    assert_array_equal(got.cpu().numpy().view(U64), want)


# --------------------------------------------------------------------------- past one scan step, one range turn
def scipy_label(fg, c):
    from scipy import ndimage as ndi
    lab, n = ndi.label(fg, structure=ndi.generate_binary_structure(3, c))
    return lab.astype(U64), int(n)


def label_dev(data, threshold, c, normalize, mode='greater'):
    """threshold_components of a device volume into a device ``out`` prefilled
    with -1 (no voxel may keep what an earlier call left in a pooled buffer)."""
    import torch
    out = torch.full(tuple(data.shape), -1, dtype=torch.int64, device='cuda')
    got, n = rag.threshold_components(torch.from_numpy(data).cuda(), threshold, mode=mode, normalize=normalize,
                                      connectivity=c, out=out)
    assert got is out
    return out.cpu().numpy().view(U64), n


def big_box_asserted():
    """C.BIG takes k_uf_scan past one step and k_cc_range past two turns
    (tests/test_cc_host.py pins the mirrors these come from)."""
    assert C.scan_steps(int(np.prod(C.BIG))) >= 2 and C.BIG[0] * C.BIG[1] > 2 * C.RANGE_ROWS


def merge_pair_sets(n):
    """name -> pairs over the ids 1 .. n - 1, n >= 2^21: nothing; 10^6 random
    pairs; chains (k, k + 2^21) and (k, k + 2048) across the scan step's and the
    segments' borders; the first id with the last."""
    rng = np.random.default_rng(n)
    step = C.SEG * C.SCAN_STEP
    far = np.arange(1, max(n - step, 1), 3)
    near = np.arange(1, n - C.SEG, 5)
    near = near[(near // 7) % 3 != 0]                      # (chains of a few links, broken here and there)
    return dict(none=np.zeros((0, 2), dtype=np.int64),
                random=rng.integers(1, n, size=(10 ** 6, 2)),
                chains=rng.permutation(np.concatenate([np.stack([far, far + step], 1),
                                                       np.stack([near, near + C.SEG], 1)])),
                ends=np.array([[1, n - 1]]))


@pytest.mark.parametrize('n', [1 << 21, (1 << 21) + 1, (1 << 21) + 2049, 3 * (1 << 21) + 5])
def test_merge_assignments_past_one_scan_step(gpu, n):
    """k_uf_scan (csrc/ctg_cc.hip) past its first step of 1024 numbering
    segments of CC_SEG = 2048 ids: `carry` and the reuse of `wsum`.  Without
    pairs every segment holds 2048 roots and the table is the identity, so a slip
    of the carry shifts everything behind it; the chains tie ids across the
    step's and the segments' borders.  Host and device pairs, the device table
    written over -1."""
    import torch
    assert C.scan_steps(n + 1) >= 2                        # (2^21 ids fill the first step to its last entry)
    for name, pairs in merge_pair_sets(n).items():
        want, max_id = C.merge_table_fast(pairs, n)
        if name == 'none':
            assert_array_equal(want, np.arange(n, dtype=U64))
        if name == 'ends':
            assert want[n - 1] == 1 and max_id == n - 2
        got, m = rag.merge_assignments(pairs.astype(U64), n, out=np.full(n, (1 << 64) - 1, dtype=U64))
        assert m == max_id, name
        assert_array_equal(got, want)
        out = torch.full((n,), -1, dtype=torch.int64, device='cuda')
        got, m = rag.merge_assignments(torch.from_numpy(pairs.astype(np.int64)).cuda(), n, out=out)
        assert got is out and m == max_id, name
        assert_array_equal(out.cpu().numpy().view(U64), want)


BIG_DENSITIES = {1: (0.2, 0.31, 0.5), 2: (0.08, 0.14, 0.3), 3: (0.05, 0.1, 0.2)}   # below, near, above percolation


@pytest.mark.parametrize('c', [1, 2, 3])
def test_big_box_random_maps(gpu, c):
    """(129,128,128): 288 tiles, about a thousand seam workgroups on every XCD
    uniting concurrently (k_cc_seams; the agent-scope argument of ctg_uf.h),
    1032 numbering segments (k_uf_flatten, k_uf_scan's second step).  Densities
    below, near and above the site-percolation point of each connectivity
    (0.3116, 0.137, 0.0976): thousands of components at each, and above it one
    that spans the box -- chains across hundreds of tile borders.  scipy's
    numbering exactly (tests/test_cc_host.py judges scipy by oracle_label)."""
    big_box_asserted()
    for k, p in enumerate(BIG_DENSITIES[c]):
        fg = C.random_fg(C.BIG, p, seed=c)
        want, n = scipy_label(fg, c)
        assert n > 1000
        if k == 2:
            assert np.bincount(want.ravel().astype(np.int64))[1:].max() > 0.1 * fg.sum()
        got, m = label_dev(as_data(fg), 0.5, c, False)
        assert m == n
        assert_array_equal(got, want)


@pytest.mark.parametrize('c', [1, 2, 3])
def test_big_box_comb(gpu, c):
    """One path through every tile border of (129,128,128), then cut once."""
    big_box_asserted()
    fg = C.comb()
    for cut in (None, (64, 64, 64)):
        if cut:
            fg[cut] = False
        want, n = scipy_label(fg, c)
        assert n == (2 if cut else 1)
        got, m = label_dev(as_data(fg), 0.5, c, False)
        assert m == n
        assert_array_equal(got, want)


@pytest.mark.parametrize('dtype', [np.float32, np.uint8])
def test_big_box_range_past_one_turn(gpu, dtype):
    """k_cc_range (csrc/ctg_cc.hip) past its first turn of 2048 x 4 = 8192 rows:
    the box's minimum only in row 0 and its maximum only in the last row, row
    16511, of the third turn; then swapped; then a NaN in the last row alone,
    which must give the empty result.  A missed extreme changes the normalised
    values, and with them the foreground."""
    big_box_asserted()
    rng = np.random.default_rng(31)
    if dtype == np.uint8:
        base, lo, hi = rng.integers(60, 200, size=C.BIG).astype(np.uint8), 0, 255
    else:
        base, lo, hi = (rng.random(C.BIG, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)), -1.0, 2.0
    for first, last in ((lo, hi), (hi, lo)):
        data = base.copy()
        data[0, 0, 77], data[-1, -1, 5] = first, last
        assert (data == lo).sum() == 1 and (data == hi).sum() == 1
        fg = C.foreground(data, 0.45, 'greater', True)
        missed = C.foreground(np.clip(data, base.min(), base.max()), 0.45, 'greater', True)
        assert (fg != missed).sum() > 1000                  # the extremes matter at this threshold
        want, n = scipy_label(fg, 1)
        got, m = label_dev(data, 0.45, 1, True)
        assert_array_equal(got != 0, fg)
        assert m == n
        assert_array_equal(got, want)
    if dtype == np.float32:
        data = base.copy()
        data[-1, -1, 100] = np.nan
        for mode in ('greater', 'less'):
            got, m = label_dev(data, 0.45, 3, True, mode=mode)
            assert m == 0 and not got.any()


def test_merge_assignments_refuses_bad_members(gpu):
    import ctypes
    lib = _lib.load()
    for bad in ([[1, 10]], [[10, 1]], [[0, 3]], [[3, 0]], [[2, 3], [4, 1 << 40]]):
        with pytest.raises(_lib.CtgError, match='status -1'):
            rag.merge_assignments(np.array(bad, dtype=U64), 10)
        # the table is untouched
        pairs = np.array(bad, dtype=U64)
        table = np.full(10, 12345, dtype=U64)
        max_id = ctypes.c_uint64(7)
        rc = lib.ctg_merge_assignments(pairs.ctypes.data, len(pairs), 10, table.ctypes.data, _lib.CTG_MEM_HOST, None,
                                       ctypes.byref(max_id))
        assert rc == -1 and (table == 12345).all()
    table = np.zeros(4, dtype=U64)
    rc = lib.ctg_merge_assignments(None, 0, 1 << 32, table.ctypes.data, _lib.CTG_MEM_HOST, None,
                                   ctypes.byref(ctypes.c_uint64(0)))
    assert rc == -4                                                          # CTG_ERR_UNSUPPORTED


def test_c_abi_argument_statuses(gpu):
    import ctypes
    lib = _lib.load()
    vol = np.zeros((2, 3, 4), dtype=np.float32)
    out = np.zeros((2, 3, 4), dtype=U64)
    n = ctypes.c_uint64(0)
    shape = (ctypes.c_int64 * 3)(2, 3, 4)

    def call(kind=_lib.CTG_DATA_F32, mode=0, conn=3, end=None):
        return lib.ctg_threshold_components(vol.ctypes.data, kind, None, shape, None, end, 0.5, mode, 1, conn,
                                            out.ctypes.data, _lib.CTG_MEM_HOST, None, ctypes.byref(n))
    assert call() == 0
    assert call(kind=_lib.CTG_DATA_NONE) == -1 and call(mode=3) == -1 and call(conn=0) == -1 and call(conn=4) == -1
    assert call(end=(ctypes.c_int64 * 3)(2, 3, 5)) == -1


# --------------------------------------------------------------------------- no workspace state
def test_deferred_stats_survive_the_calls(gpu, noise):
    """A CTG_DEFER_STATS table still packs after labelling and merge calls on its
    device: they use call-sized buffers only (the exchange simulation of
    tests/exchange_sim.py, as tests/test_gpu_take.py runs it for the apply call)."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    calls = []

    def between():
        rag.threshold_components(noise, 0.5, connectivity=3)
        rag.merge_assignments(np.array([[1, 2], [2, 900]], dtype=U64), 1000)
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=between)
    assert calls
    assert_array_equal(np.concatenate([x.edges() for x in shards]), np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)
