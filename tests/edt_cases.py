"""Oracle and inputs of the exact Euclidean distance transform (include/ctg.h:
ctg_distance_transform), shared by tests/test_edt_host.py and the GPU tests.

The contract: for a voxel p with nearest seed q, d = p - q in index units,

    D2  = (dz*pz)*(dz*pz) + (dy*py)*(dy*py) + (dx*px)*(dx*px)      float64, this order
    out = float32(sqrt(D2))

and a voxel whose domain (the box; in 2-D mode its slice) has no seed gets the
domain's diagonal.  Two oracles: ``brute`` takes the minimum of exactly that
expression over all seeds (small boxes), ``via_scipy`` lets
scipy.ndimage.distance_transform_edt name a nearest seed per voxel and
evaluates the expression on it.  With integer pitches every term is exact, so
the two agree bit for bit whatever seed of several equally near ones is named;
with other pitches a different choice among near-equal seeds changes D2 by a
few units of 2^-53 relative, at most 1 ulp after the square root and the
rounding to float32 (derived, not measured)."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_LINE = 32   # csrc/ctg_plan.h: EDT_LDS_LINE (test_edt_host.py checks the plan function at it)
# The caps past which a kernel's grid-stride loop takes a second turn, mirrored here once;
# test_edt_host.py (test_cap_mirrors) pins each against the plan functions through tools/edt_check.cpp.
X_WAVES = 4             # csrc/ctg_plan.h: EDT_X_WAVES, rows a workgroup of k_edt_x takes a turn
X_MAX_GRID = 8192       # csrc/ctg_plan.h: EDT_X_MAX_GRID, the most workgroups of k_edt_x
LINE_MAX_GRID = 8192    # csrc/ctg_plan.h: EDT_LINE_MAX_GRID, the most workgroups of k_edt_line
FOLD_THREADS = 256      # csrc/ctg_edt.hip: k_edt_fold's one workgroup (`i += 256`), a partial per k_edt_line workgroup
ROW_TOP = 4096          # csrc/ctg_edt.h: voxels under one top ("super") word of a row, 64 words x 64 bits

# the smallest shapes at which each thing can go wrong: one voxel; one row of three ballot words with a ragged
# tail; single columns; one past the tile and wave multiples on every axis; a y line and a z line just past the
# LDS limit of the envelope stacks
SHAPES = [(1, 1, 1), (1, 1, 130), (1, 70, 1), (70, 1, 1), (17, 9, 65), (33, 17, 129),
          (3, LDS_LINE + 1, 66), (LDS_LINE + 1, 3, 66)]
PITCHES = [None, (40, 4, 4), (10, 1, 3), (0.025, 0.01, 0.01), (1.7, 0.3, 1.1)]


# the shapes that drive the grid-stride loops of k_edt_x and k_edt_line past their first turn (see the functions
# below for which loop of which pass)
TURN_SHAPES = [(8193, 33, 3), (33, 8193, 3), (8193, 2, 3), (2, 8193, 3)]
TURN_PATTERNS = ['random_0.002', 'random_0.02', 'random_0.3', 'none', 'all', 'last_slice', 'plane_z']
TURN_PITCHES = [None, (10, 1, 3), (1.7, 0.3, 1.1)]


def x_turns(shape):
    """Turns of k_edt_x's `for g += gridDim.x` loop: groups of X_WAVES rows over the grid."""
    groups = -(-shape[0] * shape[1] // X_WAVES)
    return groups / min(groups, X_MAX_GRID)


def line_pass(shape, axis, two_d=False):
    """(runs, lds, groups, grid) of k_edt_line along ``axis`` (1: y, 0: z), as
    csrc/ctg_plan.h plans it (edt_passes, edt_line_plan; the grid before any
    shrinking to EDT_STACK_BYTES, which test_edt_host.py checks stays out of play)."""
    nz, ny, nx = shape
    z = not two_d and nz > 1
    runs = z if axis == 0 else not (z and ny == 1)
    groups = (nz if axis == 1 else ny) * -(-nx // 64)
    return runs, shape[axis] <= LDS_LINE, groups, min(groups, LINE_MAX_GRID)


def final_partials(shape, two_d=False):
    """Partials k_edt_fold reads: one per workgroup of the call's last pass."""
    z = line_pass(shape, 0, two_d)
    return z[3] if z[0] else line_pass(shape, 1, two_d)[3]


def is_exact(pitch):
    return pitch is None or all(float(v).is_integer() for v in pitch)


def pitch3(pitch):
    return np.ones(3) if pitch is None else np.asarray(pitch, dtype=np.float64)


def d2_of(dz, dy, dx, pitch):
    p = pitch3(pitch)
    a, b, c = dz.astype(np.float64) * p[0], dy.astype(np.float64) * p[1], dx.astype(np.float64) * p[2]
    return a * a + b * b + c * c


def diag2(shape, pitch, two_d):
    n = np.array(shape, dtype=np.int64)
    return float(d2_of(n[0] * (0 if two_d else 1), n[1], n[2], pitch))


def _domains(seeds, two_d):
    return [(slice(z, z + 1),) for z in range(seeds.shape[0])] if two_d else [(slice(None),)]


def brute(seeds, pitch=None, two_d=False):
    """D2 (float64) by the minimum over all seeds of the contract's expression."""
    seeds = np.asarray(seeds, dtype=bool)
    out = np.empty(seeds.shape, dtype=np.float64)
    for dom in _domains(seeds, two_d):
        s = seeds[dom]
        q = np.argwhere(s)
        if not len(q):
            out[dom] = diag2(seeds.shape, pitch, two_d)
            continue
        p = np.argwhere(np.ones(s.shape, dtype=bool))
        best = np.full(len(p), np.inf)
        for k in range(0, len(q), 256):
            d = np.abs(p[:, None, :] - q[None, k:k + 256, :])
            best = np.minimum(best, d2_of(d[..., 0], d[..., 1], d[..., 2], pitch).min(axis=1))
        out[dom] = best.reshape(s.shape)
    return out


def via_scipy(seeds, pitch=None, two_d=False):
    """D2 (float64) of the seed scipy names as nearest."""
    from scipy import ndimage as ndi
    seeds = np.asarray(seeds, dtype=bool)
    out = np.empty(seeds.shape, dtype=np.float64)
    for dom in _domains(seeds, two_d):
        s = seeds[dom]
        if not s.any():
            out[dom] = diag2(seeds.shape, pitch, two_d)
            continue
        idx = ndi.distance_transform_edt(~s, sampling=None if pitch is None else pitch, return_distances=False,
                                         return_indices=True)
        g = np.indices(s.shape)
        out[dom] = d2_of(np.abs(g[0] - idx[0]), np.abs(g[1] - idx[1]), np.abs(g[2] - idx[2]), pitch)
    return out


def via_scipy_2d(seeds, pitch=None):
    """via_scipy(two_d=True) in one scipy call, for boxes of thousands of slices:
    a z pitch so large that a seed of another slice never wins -- 2^40 times the
    slice's diagonal, so a step in z outweighs any in-slice distance by 2^80 and
    no rounding of scipy's own arithmetic can change a comparison between two
    seeds of one slice, whose z terms are both exactly 0 -- names the nearest
    seed of the slice wherever the slice has one; D2 is evaluated on the
    in-slice offsets.  test_edt_host.py asserts it equal to via_scipy."""
    from scipy import ndimage as ndi
    seeds = np.asarray(seeds, dtype=bool)
    p = pitch3(pitch)
    far = float(np.hypot(seeds.shape[1] * p[1], seeds.shape[2] * p[2]) * 2.0 ** 40)
    has = seeds.any(axis=(1, 2))
    out = np.full(seeds.shape, diag2(seeds.shape, pitch, True), dtype=np.float64)
    if has.any():
        idx = ndi.distance_transform_edt(~seeds, sampling=(far, p[1], p[2]), return_distances=False,
                                         return_indices=True)
        g = np.indices(seeds.shape)
        d2 = d2_of(np.zeros_like(g[1]), np.abs(g[1] - idx[1]), np.abs(g[2] - idx[2]), pitch)
        assert np.array_equal(idx[0][has], g[0][has])
        out[has] = d2[has]
    return out


def expected(d2, seeds, two_d=False):
    """(float32 distances, (n_seeds, n_unseeded, argmax, max_d2)) of a D2 array."""
    seeds = np.asarray(seeds, dtype=bool)
    if two_d:
        unseeded = int(sum(seeds[z].size for z in range(seeds.shape[0]) if not seeds[z].any()))
    else:
        unseeded = 0 if seeds.any() else seeds.size
    k = int(np.argmax(d2))                       # (the first of equal maxima)
    return np.sqrt(d2).astype(np.float32), (int(seeds.sum()), unseeded, k, float(d2.ravel()[k]))


def ulps(a, b):
    """|a - b| in float32 units in the last place (finite, non-negative values)."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) -
                  np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def check(dist, info, seeds, pitch, two_d, d2):
    """The transform's answer against the oracle's D2: bit-exact with integer
    pitches, within 1 float32 ulp otherwise (see the module docstring)."""
    want, (n_seeds, unseeded, k, top) = expected(d2, seeds, two_d)
    assert dist.dtype == np.float32 and dist.shape == want.shape
    assert info[0] == n_seeds and info[1] == unseeded
    if is_exact(pitch):
        np.testing.assert_array_equal(dist.view(np.uint32), want.view(np.uint32))
        assert info[2] == k and info[3] == top
    else:
        assert int(ulps(dist, want).max()) <= 1
        assert 0 <= info[2] < dist.size
        assert int(ulps(dist.ravel()[info[2]], want.max())) <= 1
        assert int(ulps(np.float32(np.sqrt(info[3])), want.max())) <= 1


# --------------------------------------------------------------------------- seed patterns
def patterns(shape):
    """name -> bool array of seeds"""
    nz, ny, nx = shape
    out = {}
    for c in sorted({(z, y, x) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)}):
        s = np.zeros(shape, dtype=bool)
        s[c] = True
        out['corner_%d_%d_%d' % c] = s
    for density in (0.002, 0.02, 0.3):
        rng = np.random.default_rng([nz, ny, nx, int(density * 1000)])
        out['random_%g' % density] = rng.random(shape) < density
    out['all'] = np.ones(shape, dtype=bool)
    out['none'] = np.zeros(shape, dtype=bool)
    for axis, name in enumerate('zyx'):            # one full plane: every column of the next pass sees equal values
        s = np.zeros(shape, dtype=bool)
        s[tuple(slice(None) if a != axis else shape[a] // 2 for a in range(3))] = True
        out['plane_' + name] = s
    s = np.zeros(shape, dtype=bool)                # a diagonal line: strictly convex lines, every parabola stays
    m = max(shape)
    t = np.arange(m)
    s[t * nz // m, t * ny // m, t * nx // m] = True
    out['diagonal'] = s
    g = np.indices(shape).sum(axis=0)
    out['checkerboard'] = g % 2 == 0
    for axis, name in enumerate(('last_slice', 'last_row', 'last_column')):
        s = np.zeros(shape, dtype=bool)
        s[tuple(slice(None) if a != axis else shape[a] - 1 for a in range(3))] = True
        out[name] = s
    return out


@functools.lru_cache(maxsize=None)
def case(shape, name, pitch, two_d=False):
    """(seeds, D2) of a pattern, computed once per session and left unchanged."""
    seeds = patterns(shape)[name]
    d2 = via_scipy(seeds, pitch, two_d)
    seeds.setflags(write=False)
    d2.setflags(write=False)
    return seeds, d2


def pattern_names(shape):
    return list(patterns(shape))


# --------------------------------------------------------------------------- past the first turn
def turn_pattern_names(shape):
    """TURN_PATTERNS and the far corner seed: the arg-max is then voxel 0."""
    return TURN_PATTERNS + ['corner_%d_%d_%d' % tuple(n - 1 for n in shape)]


def turn_case(shape, name, pitch, two_d=False):
    """(seeds, D2) of a pattern of a TURN_SHAPES box; not kept (6.5 MB a case)."""
    seeds = patterns(shape)[name]
    return seeds, (via_scipy_2d(seeds, pitch) if two_d else via_scipy(seeds, pitch, False))


# --------------------------------------------------------------------------- long rows
LONG_ROWS = [4097, 8193, 32767]


def row_seed_sets(nx):
    """Seed positions of a row of nx > ROW_TOP voxels: the row's two ends, the
    two sides of the first top-word border, the last bit of the first word and
    the first bit of the last full one, one seed in the second top word (or,
    where the row ends before it, at its image in the first), the middle, five
    random ones."""
    rng = np.random.default_rng(nx)
    sets = [[0], [nx - 1], [0, nx - 1], [ROW_TOP - 1, ROW_TOP], [63, nx - 64], [4160 % nx], [nx // 2],
            sorted(rng.choice(nx, size=5, replace=False).tolist())]
    return sets


def long_row_cases(nx):
    """[(seeds, D2)]: two (3,2,nx) boxes with a different seed set in each row
    (the eight sets, the second box in another order) and the plain (1,1,nx)
    row with one seed in the second top word's range or its image.  The oracle
    knows each row's |dx| = min |x - seed| and takes the minimum over the rows
    of |dx|^2 + dy^2 + dz^2 (unit pitch: every term exact)."""
    sets = row_seed_sets(nx)
    x = np.arange(nx)
    out = []
    for shape, order in (((3, 2, nx), [0, 1, 2, 3, 4, 5]), ((3, 2, nx), [7, 6, 3, 5, 4, 1]), ((1, 1, nx), [5])):
        seeds = np.zeros(shape, dtype=bool)
        rowd = np.empty(shape, dtype=np.float64)
        for r, k in enumerate(order):
            z, y = divmod(r, shape[1])
            seeds[z, y, sets[k]] = True
            rowd[z, y] = np.abs(x[:, None] - np.array(sets[k])[None, :]).min(axis=1)
        d2 = np.full(shape, np.inf)
        for z in range(shape[0]):
            for y in range(shape[1]):
                for zz in range(shape[0]):
                    for yy in range(shape[1]):
                        d2[z, y] = np.minimum(d2[z, y], rowd[zz, yy] ** 2 + float((y - yy) ** 2 + (z - zz) ** 2))
        out.append((seeds, d2))
    return out


# --------------------------------------------------------------------------- deep stacks
DEEP_SHAPES = [(4099, 1, 3), (1, 4099, 3), (300, 2, 70)]
DEEP_PITCHES = [None, (3, 1000, 7)]
DEEP_PATTERNS = ['diagonal', 'random_0.3']


# --------------------------------------------------------------------------- one seed: the D2 expression itself
SINGLE_SHAPES = [(17, 9, 65), (3, 33, 66)]
SINGLE_PITCHES = [(0.025, 0.01, 0.01), (1.7, 0.3, 1.1)]


def corner_names(shape):
    return [n for n in pattern_names(shape) if n.startswith('corner_')]


def one_per_slice(shape):
    """One seed in every slice, at another (y, x) in each."""
    nz, ny, nx = shape
    s = np.zeros(shape, dtype=bool)
    z = np.arange(nz)
    s[z, (7 * z + 3) % ny, (13 * z + 5) % nx] = True
    return s


def single_seed_d2(seeds, pitch, two_d=False):
    """D2 of a box whose every domain holds exactly one seed: the contract's
    expression on the offsets to it -- nothing to choose between."""
    seeds = np.asarray(seeds, dtype=bool)
    out = np.empty(seeds.shape, dtype=np.float64)
    for dom in _domains(seeds, two_d):
        s = seeds[dom]
        (q,) = np.argwhere(s)
        g = np.indices(s.shape)
        out[dom] = d2_of(np.abs(g[0] - q[0]), np.abs(g[1] - q[1]), np.abs(g[2] - q[2]), pitch)
    return out


def check_single_seed(seeds, pitch, two_d, dist, info, d2=None):
    """The answer for one seed a domain, bit for bit, whatever the pitch:
    ``d2`` (the call's squared=True result, where the caller has it) equals
    d2_of as float64 bit patterns, ``dist`` equals float32(sqrt(that)) and
    ``info`` names the first voxel of the largest D2 and that D2 exactly."""
    want = single_seed_d2(seeds, pitch, two_d)
    if d2 is not None:
        assert d2.dtype == np.float64 and d2.shape == want.shape
        np.testing.assert_array_equal(d2.view(np.uint64), want.view(np.uint64))
    assert dist.dtype == np.float32 and dist.shape == want.shape
    np.testing.assert_array_equal(dist.view(np.uint32), np.sqrt(want).astype(np.float32).view(np.uint32))
    k = int(np.argmax(want))
    assert tuple(info) == (int(seeds.sum()), 0, k, float(want.ravel()[k]))
    assert info[3] == want.max()


def contracted_d2(seeds, pitch, two_d=False):
    """What the D2 of single_seed_d2 would be were the sum contracted into fused
    multiply-adds, in the two ways a compiler can do it: fma(c,c, fma(b,b, a*a))
    and fma(c,c, fma(a,a, b*b)) -- by exact rationals rounded once a step."""
    from fractions import Fraction
    seeds = np.asarray(seeds, dtype=bool)
    p = pitch3(pitch)
    outs = [np.empty(seeds.shape, dtype=np.float64) for _ in range(2)]
    for dom in _domains(seeds, two_d):
        s = seeds[dom]
        (q,) = np.argwhere(s)
        g = np.indices(s.shape)
        off = [np.abs(g[k] - q[k]).astype(np.float64) * p[k] for k in range(3)]     # (one rounding each, as in d2_of)
        memo = {}
        res = [np.empty(s.shape), np.empty(s.shape)]
        for i in np.ndindex(s.shape):
            a, b, c = (float(off[k][i]) for k in range(3))
            if (a, b, c) not in memo:
                fa, fb, fc = Fraction(a), Fraction(b), Fraction(c)
                first = float(fb * fb + Fraction(a * a))
                second = float(fa * fa + Fraction(b * b))
                memo[a, b, c] = (float(fc * fc + Fraction(first)), float(fc * fc + Fraction(second)))
            res[0][i], res[1][i] = memo[a, b, c]
        outs[0][dom], outs[1][dom] = res
    return outs


# --------------------------------------------------------------------------- integer pitches up to the bound
BOUND = 2.0 ** 53
BOUND_SHAPES = [(1, 200, 3), (200, 1, 3), (40, 40, 5), (9, 130, 2)]
BOUND_DENSITIES = [0.01, 0.1, 0.5]


def bound_pitches(shape):
    """Three fixed integer pitches and the largest isotropic one: floor(sqrt(2^53))
    = 94906265 over the longest axis where that keeps the box's diagonal below
    2^53, else the largest integer that does (the other axes count too)."""
    import math
    n2 = sum(int(n) ** 2 for n in shape)
    p = min(94906265 // max(shape), math.isqrt((2 ** 53 - 1) // n2))     # p^2 n2 <= 2^53 - 1
    return [(262145, 262147, 3), (3, 262147, 262145), (1, 1, 333333), (p, p, p)]


@functools.lru_cache(maxsize=None)
def bound_case(shape, pitch, density):
    """(seeds, D2) by brute force, the box's diagonal below 2^53 (asserted by the tests)."""
    rng = np.random.default_rng([shape[0], shape[1], shape[2], int(density * 100)])
    seeds = rng.random(shape) < density
    seeds[tuple(rng.integers(0, n) for n in shape)] = True
    d2 = brute(seeds, pitch)
    seeds.setflags(write=False)
    d2.setflags(write=False)
    return seeds, d2


def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'edt_kat.json')) as f:
        g = json.load(f)
    for c in g['cases']:
        shape = tuple(c['shape'])
        c['shape'] = shape
        c['source'] = np.array(c['source'], dtype=np.uint8).reshape(shape)
        c['d2'] = np.array(c['d2'], dtype=np.float64).reshape(shape)
    return g
