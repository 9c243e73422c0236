"""ctg_distance_transform on the GPU against the oracles of tests/edt_cases.py:
bit-exact with integer pitches -- every term of D2 is then exact in float64,
so the result does not depend on which of several equally near seeds a pass
picks -- and within 1 float32 ulp with other pitches, where a different choice
among near-equal seeds changes D2 by a few units of 2^-53 relative, which the
square root and the rounding to float32 turn into at most one unit in the last
place.  ``info`` entry for entry."""
import ctypes

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import _lib, distance, rag
from tests import edt_cases as E

pytestmark = pytest.mark.gpu


def run(seeds, pitch=None, two_d=False, **kw):
    dist, info = rag.distance_transform(np.asarray(seeds).astype(np.uint8), pitch=pitch, two_d=two_d, **kw)
    return dist, tuple(info)


# --------------------------------------------------------------------------- shapes x patterns x pitches
@pytest.mark.parametrize('shape', E.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_shapes_patterns_pitches(gpu, shape):
    for name in E.pattern_names(shape):
        for pitch in E.PITCHES:
            seeds, d2 = E.case(shape, name, pitch)
            dist, info = run(seeds, pitch)
            try:
                E.check(dist, info, seeds, pitch, False, d2)
            except AssertionError as err:
                raise AssertionError('%s pitch %s: %s' % (name, pitch, err)) from None


def test_corner_seeds_pin_the_square_root(gpu):
    """A single seed at each corner of (33,17,129) with unit pitch: D2 runs over
    sums of three squares, and every one of them must come out as
    float32(sqrt(float64(n)))."""
    shape = (33, 17, 129)
    g = np.indices(shape)
    seen = set()
    for z in (0, shape[0] - 1):
        for y in (0, shape[1] - 1):
            for x in (0, shape[2] - 1):
                seeds = np.zeros(shape, dtype=bool)
                seeds[z, y, x] = True
                n = (g[0] - z) ** 2 + (g[1] - y) ** 2 + (g[2] - x) ** 2
                dist, info = run(seeds)
                assert_array_equal(dist.view(np.uint32), np.sqrt(n.astype(np.float64)).astype(np.float32).view(np.uint32))
                assert info == (1, 0, int(np.argmax(n)), float(n.max()))
                seen |= set(np.unique(n).tolist())
    assert len(seen) > 5000


# --------------------------------------------------------------------------- past the first grid turn
def run_dev(seeds, pitch=None, two_d=False, squared=False):
    """The transform of a device source into a device ``out`` prefilled with -1:
    a voxel that no turn writes stays negative, whatever an earlier call left in
    the pool's buffers."""
    import torch
    src = torch.from_numpy(np.array(seeds, dtype=np.uint8)).cuda()
    out = torch.full(tuple(seeds.shape), -1.0, dtype=torch.float64 if squared else torch.float32, device='cuda')
    got, info = rag.distance_transform(src, pitch=pitch, two_d=two_d, squared=squared, out=out)
    assert got is out
    return out.cpu().numpy(), tuple(info)


def turns_asserted(shape, two_d):
    """What the box takes past a first turn, from the mirrors of tests/edt_cases.py
    (tests/test_edt_host.py pins them against the plan functions)."""
    y, z = E.line_pass(shape, 1, two_d), E.line_pass(shape, 0, two_d)
    if shape in ((8193, 33, 3), (33, 8193, 3)):
        rows = shape[0] * shape[1]                               # k_edt_x: 8.25 turns, one live wave in the last group
        assert E.x_turns(shape) >= 2 and rows % E.X_WAVES == 1 and rows > 2 * E.X_WAVES * E.X_MAX_GRID
    if shape == (8193, 33, 3):                                   # y pass: buffer stacks, 8193 groups on 8192 workgroups
        assert y[0] and not y[1] and y[2] > y[3] == E.LINE_MAX_GRID
    if shape == (33, 8193, 3) and not two_d:                     # z pass: the same along z
        assert z[0] and not z[1] and z[2] > z[3] == E.LINE_MAX_GRID
    if shape == (8193, 2, 3):                                    # y pass: LDS stacks past the cap
        assert y[0] and y[1] and y[2] > y[3] == E.LINE_MAX_GRID
    if shape == (2, 8193, 3):                                    # z pass: LDS stacks past the cap
        assert z[0] and z[1] and z[2] > z[3] == E.LINE_MAX_GRID
    if (shape, two_d) in (((8193, 33, 3), True), ((33, 8193, 3), False), ((2, 8193, 3), False)):
        assert E.final_partials(shape, two_d) >= 2 * E.FOLD_THREADS   # k_edt_fold: several partials a thread


TURN_CASES = [(shape, pitch, two_d) for shape in E.TURN_SHAPES for two_d in (False, True) for pitch in E.TURN_PITCHES
              if not two_d or shape in E.TURN_SHAPES[:2]]


@pytest.mark.parametrize('shape,pitch,two_d', TURN_CASES,
                         ids=['%dx%dx%d-%s-%s' % (s + (p, '2d' if t else '3d')) for s, p, t in TURN_CASES])
def test_turn_shapes(gpu, shape, pitch, two_d):
    """k_edt_x's and k_edt_line's `for (g = blockIdx.x; g < groups; g += gridDim.x)`
    past their first turn, and k_edt_fold's `i += 256` (csrc/ctg_edt.hip):
    boxes of more than EDT_X_WAVES x EDT_X_MAX_GRID = 32768 rows and of more
    than EDT_LINE_MAX_GRID = 8192 groups of columns with lines of 33 (stacks in
    the buffer, BufStack.stride = gridDim.x x 64) and of 2 (stacks in LDS) --
    the LDS seed words rewritten behind three barriers a turn, a ragged last
    group, k / top / j reset and best / unseeded carried from turn to turn.
    Every output starts at -1.  In 2-D mode the sparse patterns leave thousands
    of unseeded slices, info[1] a sum over all workgroups and turns; with the
    far corner seed the arg-max is voxel 0; with 'all' every partial ties at 0
    and the first voxel must win."""
    turns_asserted(shape, two_d)
    V = shape[0] * shape[1] * shape[2]
    for name in E.turn_pattern_names(shape):
        seeds, d2 = E.turn_case(shape, name, pitch, two_d)
        dist, info = run_dev(seeds, pitch, two_d)
        try:
            E.check(dist, info, seeds, pitch, two_d, d2)
            if name == 'all':
                assert info == (V, 0, 0, 0.0)
            if name.startswith('corner') and not two_d:
                assert info[2] == 0
            if two_d and name == 'random_0.002' and shape == (8193, 33, 3):
                assert info[1] > 1000 * shape[1] * shape[2]
        except AssertionError as err:
            raise AssertionError('%s: %s' % (name, err)) from None


# --------------------------------------------------------------------------- long rows, deep stacks, the bound
@pytest.mark.parametrize('nx', E.LONG_ROWS)
def test_long_rows(gpu, nx):
    """edt_prev_seed / edt_next_seed (csrc/ctg_edt.h) in k_edt_x on rows of more
    than E.ROW_TOP = 4096 voxels: both walks over the top words and their word
    edges, a different seed set in each of a workgroup's four waves (their LDS
    words differ), as tests/test_edt_host.py runs them on the host."""
    assert nx > E.ROW_TOP
    for seeds, d2 in E.long_row_cases(nx):
        dist, info = run_dev(seeds)
        E.check(dist, info, seeds, None, False, d2)


@pytest.mark.parametrize('shape', E.DEEP_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_deep_stacks(gpu, shape):
    """k_edt_line's buffer stacks thousands of entries deep: lines of 4099 and
    300 whose envelope keeps every parabola or pops often."""
    assert max(shape[0], shape[1]) > E.LDS_LINE
    for name in E.DEEP_PATTERNS:
        for pitch in E.DEEP_PITCHES:
            seeds, d2 = E.case(shape, name, pitch)
            dist, info = run_dev(seeds, pitch)
            E.check(dist, info, seeds, pitch, False, d2)


@pytest.mark.parametrize('shape', E.BOUND_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_integer_pitches_up_to_the_bound(gpu, shape):
    """Bit-exact against brute force with integer pitches up to the documented
    bound (nz pz)^2 + (ny py)^2 + (nx px)^2 < 2^53 (include/ctg.h), which is
    asserted of every case: edt_takeover's floor near the bound."""
    for pitch in E.bound_pitches(shape):
        assert E.is_exact(pitch) and E.diag2(shape, pitch, False) < E.BOUND
        for density in E.BOUND_DENSITIES:
            seeds, d2 = E.bound_case(shape, pitch, density)
            dist, info = run_dev(seeds, pitch)
            E.check(dist, info, seeds, pitch, False, d2)
            sq, info2 = run_dev(seeds, pitch, squared=True)
            assert info2 == info
            assert_array_equal(sq.view(np.uint64), np.asarray(d2).view(np.uint64))


# --------------------------------------------------------------------------- the D2 expression
def test_single_seed_pins_the_expression(gpu):
    """The test that pins -ffp-contract=off (csrc/Makefile) and the order of the
    three additions of edt_d2 (csrc/ctg_edt.h): with one seed a domain there is
    nothing to choose between, so under any pitch D2 is the contract's
    (dz pz)^2 + (dy py)^2 + (dx px)^2 in float64, added in this order and
    uncontracted -- compared as bit patterns, with float32(sqrt(D2)) and info's
    largest D2.  tests/test_edt_host.py shows that each case has voxels that
    differ under a contraction or another order."""
    for shape in E.SINGLE_SHAPES:
        cases = [(E.patterns(shape)[name], False) for name in E.corner_names(shape)] + [(E.one_per_slice(shape), True)]
        assert len(cases) == 9
        for seeds, two_d in cases:
            for pitch in E.SINGLE_PITCHES:
                d2, info2 = run_dev(seeds, pitch, two_d, squared=True)
                dist, info = run_dev(seeds, pitch, two_d)
                assert info2 == info
                E.check_single_seed(seeds, pitch, two_d, dist, info, d2)


# --------------------------------------------------------------------------- 2-D mode
@pytest.mark.parametrize('shape', [(17, 9, 65), (3, E.LDS_LINE + 1, 66), (1, 70, 1), (70, 1, 1)],
                         ids=lambda s: '%dx%dx%d' % s)
def test_two_d_mode(gpu, shape):
    """Every slice on its own; 'last_slice' and the sparse random pattern leave
    slices without a seed, which get the slice's diagonal."""
    for name in ('random_0.002', 'random_0.02', 'random_0.3', 'none', 'last_slice', 'diagonal', 'plane_x'):
        for pitch in (None, (10, 1, 3), (1.7, 0.3, 1.1)):
            seeds, d2 = E.case(shape, name, pitch, True)
            dist, info = run(seeds, pitch, two_d=True)
            E.check(dist, info, seeds, pitch, True, d2)
    seeds, d2 = E.case(shape, 'last_slice', None, True)
    if shape[0] > 1:
        dist, info = run(seeds, two_d=True)
        assert info[1] == (shape[0] - 1) * shape[1] * shape[2] and info[2] == 0
        assert np.all(dist[0] == np.float32(np.sqrt(float(shape[1] ** 2 + shape[2] ** 2))))


def test_golden(gpu):
    for c in E.golden()['cases']:
        pitch = None if c['pitch'] is None else tuple(c['pitch'])
        dist, info = rag.distance_transform(c['source'], pitch=pitch, to_background=c['to_background'], two_d=c['two_d'])
        assert_array_equal(dist, np.sqrt(c['d2']).astype(np.float32))
        assert list(info) == c['info']
        d2, info2 = rag.distance_transform(c['source'], pitch=pitch, to_background=c['to_background'],
                                           two_d=c['two_d'], squared=True)
        assert d2.dtype == np.float64 and info2 == info
        assert_array_equal(d2, c['d2'])


# --------------------------------------------------------------------------- source kinds, both senses
SHAPE = (17, 9, 65)


@pytest.fixture(scope='module')
def noise():
    return np.random.default_rng(3).random(SHAPE, dtype=np.float32)


@pytest.mark.parametrize('to_background', [False, True])
def test_source_kinds(gpu, noise, to_background):
    pitch = (10, 1, 3)

    def want(p):
        seeds = p != to_background
        return seeds, E.via_scipy(seeds, pitch)

    def check(src, p, **kw):
        seeds, d2 = want(p)
        dist, info = rag.distance_transform(src, pitch=pitch, to_background=to_background, **kw)
        E.check(dist, tuple(info), seeds, pitch, False, d2)

    # uint8 and bool: nonzero, whatever the value
    p = noise > 0.9
    check(p, p)
    check(np.where(p, np.uint8(255), np.uint8(0)), p)
    check(np.where(p, np.uint8(1), np.uint8(0)), p)
    # float32: strictly greater, in float32; a NaN is not greater
    t = np.float32(0.9)
    v = noise.copy()
    v[noise > 0.97] = np.nan
    v[(noise > 0.8) & (noise < 0.83)] = t                       # equal to the threshold: not greater
    v[0, 0, 0], v[-1, -1, -1] = np.nextafter(t, np.float32(2)), np.nextafter(t, np.float32(0))
    with np.errstate(invalid='ignore'):
        p = v > t
    assert p[0, 0, 0] and not p[-1, -1, -1] and np.isnan(v).sum() > 50 and (v == t).sum() > 50
    check(v, p, threshold=float(t))
    # labels: uint32, uint64, an id of 2^32 and above, an id whose low word matches other labels
    lab = np.random.default_rng(4).integers(0, 40, SHAPE).astype(np.uint32)
    check(lab, lab == 7, label=7)
    check(lab.astype(np.int32), lab == 7, label=7)
    check(lab, np.zeros(SHAPE, dtype=bool), label=(1 << 32) + 7)       # matches nothing in a 32-bit volume
    big = lab.astype(np.uint64)
    big[lab == 7] = (1 << 32) + 7
    big[lab == 8] = 7                                                  # the low word alone must not match
    check(big, lab == 7, label=(1 << 32) + 7)
    check(big.view(np.int64), lab == 8, label=7)
    check(big, lab == 0, label=0)


# --------------------------------------------------------------------------- boxes, tensors, streams, out=
def test_sub_box_with_odd_begin(gpu, noise):
    """A box with an odd begin on every axis inside a larger array: the row
    starts are misaligned for the byte loads, and nothing outside is a seed."""
    big = np.random.default_rng(5).random((23, 15, 140)) < 0.05
    b, e = (3, 1, 7), (3 + 17, 1 + 9, 7 + 65)
    inner = big[tuple(slice(lo, hi) for lo, hi in zip(b, e))]
    for pitch in (None, (40, 4, 4)):
        d2 = E.via_scipy(inner, pitch)
        dist, info = rag.distance_transform(big, pitch=pitch, begin=b, end=e)
        E.check(dist, tuple(info), inner, pitch, False, d2)
    lab = np.where(big, np.uint64(5), np.uint64(1 << 40))
    dist, info = rag.distance_transform(lab, label=5, begin=b, end=e)
    E.check(dist, tuple(info), inner, None, False, E.via_scipy(inner))
    # an empty box: nothing written, success
    out = np.full((0, 9, 65), 7, dtype=np.float32)
    dist, info = rag.distance_transform(big, begin=(3, 1, 7), end=(3, 10, 72), out=out)
    assert dist is out and tuple(info) == (0, 0, 0, 0.0)


def test_tensors_streams_out_and_repeat(gpu, noise):
    import torch
    pitch = (40, 4, 4)
    p = noise > 0.95
    d2 = E.via_scipy(p, pitch)
    want = np.sqrt(d2).astype(np.float32)
    src = torch.from_numpy(noise).cuda()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dist, info = rag.distance_transform(src, pitch=pitch, threshold=0.95)
        again, info2 = rag.distance_transform(src, pitch=pitch, threshold=0.95)
    stream.synchronize()
    assert dist.is_cuda and dist.dtype == torch.float32
    E.check(dist.cpu().numpy(), tuple(info), p, pitch, False, d2)
    assert info2 == info and torch.equal(dist.view(torch.int32), again.view(torch.int32))   # identical bits
    out = torch.full(SHAPE, -1.0, dtype=torch.float32, device='cuda')
    got, _ = rag.distance_transform(src, pitch=pitch, threshold=0.95, out=out)
    assert got is out
    assert_array_equal(out.cpu().numpy(), want)
    pb = torch.from_numpy(p).cuda()                                # bool tensor, explicit stream handle
    got, _ = rag.distance_transform(pb, pitch=pitch, stream=ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    assert_array_equal(got.cpu().numpy(), want)
    sq, _ = rag.distance_transform(pb, pitch=pitch, squared=True)
    assert sq.dtype == torch.float64
    assert_array_equal(sq.cpu().numpy(), d2)
    host_out = np.full(SHAPE, 9, dtype=np.float32)
    got, _ = rag.distance_transform(p, pitch=pitch, out=host_out)
    assert got is host_out
    assert_array_equal(host_out, want)


def test_mirrors(gpu, noise):
    """vigra's and scipy's spellings, 2-D and 3-D, against scipy."""
    from scipy import ndimage as ndi
    obj = noise < 0.9
    for arr, sampling in ((obj, None), (obj, (4, 1, 1)), (obj[3], None), (obj[3], (2, 3))):
        want = ndi.distance_transform_edt(arr, sampling=sampling)
        got = distance.distance_transform_edt(arr, sampling=sampling)
        assert got.dtype == np.float64
        assert_array_equal(got, want)
        assert np.argmax(got) == np.argmax(want)
        v = distance.distanceTransform(arr.astype(np.uint32), background=False, pixel_pitch=sampling)
        assert v.dtype == np.float32 and v.shape == arr.shape
        assert_array_equal(v, want.astype(np.float32))
        v = distance.distanceTransform((~arr).astype(np.float32), pixel_pitch=sampling)   # background=True: to the nonzero
        assert_array_equal(v, want.astype(np.float32))


def test_apply_dt(gpu, noise):
    """_apply_dt in both modes against scipy per slice and in 3-D; None where
    nothing passes the threshold."""
    from scipy import ndimage as ndi
    above = noise > 0.93
    above[5] = False                                               # a slice without a seed (2-D mode: its diagonal)
    inp = np.where(above, noise, np.float32(0.1))
    got = distance.apply_dt(inp, threshold=0.93)
    for z in range(SHAPE[0]):
        if above[z].any():
            assert_array_equal(got[z], ndi.distance_transform_edt(~above[z]).astype(np.float32))
        else:
            assert np.all(got[z] == np.float32(np.sqrt(float(SHAPE[1] ** 2 + SHAPE[2] ** 2))))
    for pitch in (None, (4, 1, 1)):
        got = distance.apply_dt(inp, threshold=0.93, pixel_pitch=pitch, apply_dt_2d=False)
        assert_array_equal(got, ndi.distance_transform_edt(~above, sampling=pitch).astype(np.float32))
    assert distance.apply_dt(inp, threshold=2.0) is None
    assert distance.apply_dt(inp, threshold=2.0, apply_dt_2d=False) is None


# --------------------------------------------------------------------------- the C ABI's argument errors
def test_c_abi_argument_statuses(gpu):
    lib = _lib.load()
    vol = np.ones((2, 3, 4), dtype=np.uint8)
    out = np.full((2, 3, 4), 7, dtype=np.float32)
    shape = (ctypes.c_int64 * 3)(2, 3, 4)
    info = (ctypes.c_uint64 * 4)()

    def call(kind=_lib.CTG_EDT_SRC_NONZERO, bits=8, shape=shape, begin=None, end=None, pitch=None, flags=0,
             mem=_lib.CTG_MEM_HOST, src=vol.ctypes.data):
        p = (ctypes.c_double * 3)(*pitch) if pitch is not None else None
        return lib.ctg_distance_transform(src, kind, bits, shape, begin, end, 0.5, 0, p, flags, out.ctypes.data, mem,
                                          None, info)
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    assert call(end=(ctypes.c_int64 * 3)(2, 3, 5)) == ERR_ARG                       # a box outside the array
    assert call(begin=(ctypes.c_int64 * 3)(0, 0, -1)) == ERR_ARG
    assert call(begin=(ctypes.c_int64 * 3)(0, 2, 0), end=(ctypes.c_int64 * 3)(2, 1, 4)) == ERR_ARG
    assert call(kind=3) == ERR_ARG and call(kind=-1) == ERR_ARG                     # a bad kind, or its width
    assert call(bits=32) == ERR_ARG and call(kind=_lib.CTG_EDT_SRC_GREATER, bits=8) == ERR_ARG
    assert call(kind=_lib.CTG_EDT_SRC_EQUAL, bits=16) == ERR_ARG
    assert call(flags=8) == ERR_ARG and call(flags=-1) == ERR_ARG                   # a bad flag
    assert call(mem=2) == ERR_ARG
    for bad in ((1, 0, 1), (1, 1, -1), (float('nan'), 1, 1), (1, float('inf'), 1)):
        assert call(pitch=bad) == ERR_ARG
    assert call(src=None) == ERR_ARG
    assert b'ctg_distance_transform' in lib.ctg_last_error()
    # 2^32 voxels, and an axis of 32768: refused before the source is looked at
    assert call(shape=(ctypes.c_int64 * 3)(2048, 2048, 1024)) == ERR_UNSUPPORTED
    assert call(shape=(ctypes.c_int64 * 3)(1, 1, 32768)) == ERR_UNSUPPORTED
    assert call(shape=(ctypes.c_int64 * 3)(32768, 1, 1)) == ERR_UNSUPPORTED
    assert np.all(out == 7) and list(info) == [0, 0, 0, 0]                          # the output stays untouched
    # an empty box writes nothing and succeeds
    assert call(begin=(ctypes.c_int64 * 3)(1, 1, 1), end=(ctypes.c_int64 * 3)(1, 3, 4)) == 0
    assert np.all(out == 7)
    assert call() == 0                                                              # and the call as it should be
    assert np.all(out == 0) and list(info)[:2] == [24, 0]
    long_row = np.zeros((1, 1, 32767), dtype=np.uint8)                              # the longest axis that is taken
    long_row[0, 0, 100] = 1
    dist, inf = rag.distance_transform(long_row)
    assert_array_equal(dist[0, 0], np.abs(np.arange(32767) - 100).astype(np.float32))
    assert tuple(inf) == (1, 0, 32766, float(32666 ** 2))


# --------------------------------------------------------------------------- no workspace state
def test_deferred_stats_survive_the_call(gpu, noise):
    """A CTG_DEFER_STATS table taken before a transform still packs after it:
    the call uses call-sized buffers only (the exchange simulation of
    tests/exchange_sim.py, as tests/test_gpu_cc.py runs it for the components)."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    calls = []

    def between():
        rag.distance_transform(noise, threshold=0.5, pitch=(4, 1, 1))
        rag.distance_transform(np.zeros((3, E.LDS_LINE + 1, 66), dtype=np.uint8), two_d=True)
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=between)
    assert calls
    assert_array_equal(np.concatenate([x.edges() for x in shards]), np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)
