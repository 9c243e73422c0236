"""rag.seeded_watershed on the GPU (csrc/ctg_ws.hip) against the oracles of
tests/ws_cases.py and the golden fixture.  Every comparison is exact: the labels
and the call's info (largest label, voxels left 0, labels dropped); the rounds
are held to their bound."""
import functools
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import _lib, rag
from tests import ws_cases as W

pytestmark = pytest.mark.gpu

U64 = np.uint64
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ws_kat.json')


@functools.lru_cache(maxsize=None)
def case(hk, sk, shape, two_d=False, limit=0):
    """(heights, seeds, labels, info) of a generated case; computed once, never written to."""
    h, s = W.heights(hk, shape, seed=shape[2]), W.seeds(sk, shape, seed=shape[0])
    want, info = W.oracle(h, s, limit, two_d)
    for a in (h, s, want):
        a.setflags(write=False)
    return h, s, want, info


def check(h, s, want, info, two_d=False, limit=0, **kw):
    got, gi = rag.seeded_watershed(h, s, size_filter=limit, two_d=two_d, **kw)
    assert got.dtype == U64 and got.shape == want.shape
    assert_array_equal(got, want)
    assert (gi.max_id, gi.n_zero, gi.n_dropped) == info
    assert gi.rounds <= W.round_bound(s)
    return got, gi


# --------------------------------------------------------------------------- fixture, shapes, maps, seeds
def test_kats(gpu):
    for c in W.load_kats(KATS):
        got, _ = rag.seeded_watershed(c['hmap'], c['seeds'], two_d=c['two_d'])
        assert_array_equal(got, c['labels'], err_msg=c['name'])


@pytest.mark.parametrize('hk', W.HEIGHTS)
@pytest.mark.parametrize('shape', W.SHAPES)
def test_maps_and_seeds(gpu, shape, hk):
    """Every height map with every seed layout on the shapes that cross the tile
    by one voxel on each axis, and the degenerate ones."""
    for sk in W.SEEDS:
        check(*case(hk, sk, shape))


@pytest.mark.parametrize('hk', ['distinct', 'levels8', 'serpentine'])
@pytest.mark.parametrize('shape', [(17, 9, 65), (33, 17, 129)])
def test_many_segments(gpu, shape, hk):
    """Seed densities at which the oracle alone yields many segments."""
    h, s, want, info = case(hk, 'scattered', shape)
    assert W.n_segments(want) >= 50
    check(h, s, want, info)
    # the oracle's labels differ from a copy of the seeds: the flood moved
    assert (want != s).sum() > want.size // 2


@pytest.mark.parametrize('hk', ['distinct', 'levels2', 'constant', 'special'])
@pytest.mark.parametrize('shape', W.SHAPES)
def test_two_d(gpu, shape, hk):
    """Every slice on its own; seeds in every other slice only, so the rest stay 0."""
    h = W.heights(hk, shape, seed=3)
    s = W.seeds('scattered', shape, seed=4).copy()
    s[1::2] = 0
    want, info = W.oracle(h, s, 0, True)
    check(h, s, want, info, two_d=True)
    assert not want[1::2].any()
    if shape[0] > 1:
        assert not np.array_equal(want, W.oracle(h, s, 0, False)[0])


@pytest.mark.parametrize('dtype', [np.uint32, np.int32, np.uint64, np.int64])
def test_seed_widths(gpu, dtype):
    h, s, want, info = case('levels8', 'scattered', (17, 9, 65))
    check(h, s.astype(dtype), want, info)


def test_labels_above_2_32(gpu):
    h, s, want, info = case('levels256', 'big', (17, 9, 65))
    assert info[0] > 1 << 32
    check(h, s, want, info)


def test_disconnected_blobs_share_a_label(gpu):
    h, s, want, info = case('distinct', 'blobs', (33, 17, 129))
    from scipy.ndimage import label
    lab = int(s.max())
    assert label(s == lab)[1] == 2
    check(h, s, want, info)


def test_past_the_first_grid_turn(gpu):
    """More voxels than one turn of the capped grid takes (ws_cases.GRID_TURN):
    every kernel's stride loop runs a second, ragged turn, in both floods."""
    assert W.GRID_TURN < int(np.prod(W.BIG)) < 2 * W.GRID_TURN
    h, s, want, info = case('levels8', 'scattered', W.BIG)
    assert W.n_segments(want) >= 1000
    check(h, s, want, info)
    kept, dropped = W.size_filter(want, h, 30)      # (from the flood above: one oracle run less)
    assert 0 < dropped < W.n_segments(want)
    check(h, s, kept, (int(kept.max()), int((kept == 0).sum()), dropped), limit=30)


# --------------------------------------------------------------------------- call forms
def test_sub_box(gpu):
    shape = (20, 21, 140)
    h, s = W.heights('levels8', shape, seed=5), W.seeds('scattered', shape, seed=6)
    b, e = (2, 3, 5), (19, 12, 70)
    sl = tuple(slice(lo, hi) for lo, hi in zip(b, e))
    for two_d in (False, True):
        want, info = W.oracle(np.ascontiguousarray(h[sl]), np.ascontiguousarray(s[sl]), 0, two_d)
        check(h, s, want, info, two_d=two_d, begin=b, end=e)
    for limit in (4,):
        want, info = W.oracle(np.ascontiguousarray(h[sl]), np.ascontiguousarray(s[sl]), limit, False)
        assert info[2] > 0
        check(h, s, want, info, limit=limit, begin=b, end=e)


def test_in_place(gpu):
    h, s, want, info = case('levels8', 'scattered', (17, 9, 65))
    for limit in (0, 30):
        want, info = W.oracle(h, s, limit)
        buf = s.copy()
        got, gi = rag.seeded_watershed(h, buf, size_filter=limit, out=buf)
        assert got is buf
        assert_array_equal(buf, want)
        assert (gi.max_id, gi.n_zero, gi.n_dropped) == info


def test_tensors_on_a_side_stream(gpu):
    import torch
    h, s, want, info = case('distinct', 'scattered', (33, 17, 129))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        th = torch.from_numpy(h.copy()).cuda()
        ts = torch.from_numpy(s.astype(np.int64)).cuda()
        got, gi = rag.seeded_watershed(th, ts)
        assert got.dtype == torch.int64 and got.is_cuda
        assert_array_equal(got.cpu().numpy().view(U64), want)
        assert (gi.max_id, gi.n_zero, gi.n_dropped) == info
        # in place on the device, 32-bit seeds into a given tensor
        got32, _ = rag.seeded_watershed(th, ts.to(torch.int32), out=torch.empty_like(ts))
        assert_array_equal(got32.cpu().numpy().view(U64), want)
        out, _ = rag.seeded_watershed(th, ts, out=ts)
        assert out is ts
        assert_array_equal(ts.cpu().numpy().view(U64), want)
    side.synchronize()


# --------------------------------------------------------------------------- size filter
@pytest.mark.parametrize('two_d', [False, True])
def test_size_filter(gpu, two_d):
    shape = (17, 9, 65)
    h, s, flood, _ = case('levels8', 'scattered', shape, two_d)
    sizes = np.concatenate([np.unique(p[p != 0], return_counts=True)[1] for p in (flood if two_d else [flood])])
    distinct = np.unique(sizes)
    assert distinct.size >= 3
    mid = int(distinct[distinct.size // 2])
    n_below = {limit: int((sizes < limit).sum()) for limit in (mid, mid + 1)}
    # a size equal to the limit is kept: one voxel more in the limit drops those labels too
    assert 0 < n_below[mid] < n_below[mid + 1] < sizes.size
    for limit, dropped in ((1, 0), (int(sizes.min()), 0), (mid, n_below[mid]), (mid + 1, n_below[mid + 1]),
                           (int(sizes.max()) + 1, sizes.size)):
        want, info = W.oracle(h, s, limit, two_d)
        assert info[2] == dropped
        got, _ = check(h, s, want, info, two_d=two_d, limit=limit)
        if dropped == sizes.size:
            assert not got.any()


def test_size_filter_counts_a_label_over_its_pieces(gpu):
    """A label whose two disconnected pieces reach the limit only together stays."""
    from scipy.ndimage import label
    x = np.arange(70)
    hx = np.minimum(np.minimum(abs(x - 0), 0.5 * abs(x - 35)), abs(x - 69)).astype(np.float32)
    h = np.broadcast_to(hx, (3, 4, 70)).copy()    # three valleys along x: label 5 in the outer two, 9 between
    s = np.zeros(h.shape, dtype=U64)
    s[0, 0, 0] = s[0, 0, 69] = 5
    s[0, 0, 35] = 9
    flood, _ = W.oracle(h, s, 0)
    n5 = int((flood == 5).sum())
    pieces, n_pieces = label(flood == 5)
    assert n_pieces == 2 and max((pieces == 1).sum(), (pieces == 2).sum()) < n5 < (flood == 9).sum()
    for limit, kept in ((n5, True), (n5 + 1, False)):
        want, info = W.oracle(h, s, limit)
        assert bool((want == 5).any()) == kept and info[2] == (0 if kept else 1)
        check(h, s, want, info, limit=limit)


# --------------------------------------------------------------------------- across runs, errors
def test_two_runs_agree(gpu):
    h, s, want, info = case('levels2', 'scattered', (33, 17, 129))
    a, ia = check(h, s, want, info)
    b, ib = check(h, s, want, info)
    assert_array_equal(a, b)
    assert ia == ib


def test_round_bound_is_tight_enough(gpu):
    """No seed near: a ramp floods from its low end in rounds, not in steps."""
    h, s, want, info = case('ramp', 'one', (1, 1, 130))
    _, gi = check(h, s, want, info)
    assert 1 <= gi.rounds <= W.round_bound(s) == 9


def test_nan_raises_and_writes_nothing(gpu):
    import torch
    h, s, _, _ = case('distinct', 'scattered', (17, 9, 65))
    bad = h.copy()
    bad[16, 8, 64] = np.nan
    out = np.full(h.shape, 77, dtype=U64)
    with pytest.raises(ValueError, match='NaN'):
        rag.seeded_watershed(bad, s, out=out)
    assert (out == 77).all()
    # a tensor's NaN is found by the library, before anything is written
    tout = torch.full(h.shape, 77, dtype=torch.int64, device='cuda')
    with pytest.raises(_lib.CtgError, match='NaN'):
        rag.seeded_watershed(torch.from_numpy(bad).cuda(), torch.from_numpy(s.astype(np.int64)).cuda(), out=tout)
    assert bool((tout == 77).all())
    # outside the box it does not count
    got, _ = rag.seeded_watershed(bad, s, end=(16, 9, 65))
    assert_array_equal(got, W.oracle(np.ascontiguousarray(bad[:16]), np.ascontiguousarray(s[:16]))[0])


def test_library_argument_errors(gpu):
    import ctypes
    lib = _lib.load()
    h = np.zeros((2, 2, 2), dtype=np.float32)
    s = np.zeros((2, 2, 2), dtype=U64)
    out = np.zeros((2, 2, 2), dtype=U64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    sh = (ctypes.c_int64 * 3)(2, 2, 2)
    big = (ctypes.c_int64 * 3)(1025, 1024, 1024)
    assert lib.ctg_seeded_watershed(p(h), p(s), 16, sh, None, None, 0, 0, p(out), 0, None, None) == -1
    assert lib.ctg_seeded_watershed(p(h), p(s), 64, sh, None, None, 2, 0, p(out), 0, None, None) == -1
    assert lib.ctg_seeded_watershed(None, p(s), 64, sh, None, None, 0, 0, p(out), 0, None, None) == -1
    assert lib.ctg_seeded_watershed(p(h), p(s), 64, big, None, None, 0, 0, p(out), 0, None, None) == -1
    assert b'2^30' in lib.ctg_last_error()
    s32 = np.zeros((2, 2, 2), dtype=np.uint32)
    assert lib.ctg_seeded_watershed(p(h), p(s32), 32, sh, None, None, 0, 0, p(s32), 0, None, None) == -1
