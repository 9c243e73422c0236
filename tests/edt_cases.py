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

# the smallest shapes at which each thing can go wrong: one voxel; one row of three ballot words with a ragged
# tail; single columns; one past the tile and wave multiples on every axis; a y line and a z line just past the
# LDS limit of the envelope stacks
SHAPES = [(1, 1, 1), (1, 1, 130), (1, 70, 1), (70, 1, 1), (17, 9, 65), (33, 17, 129),
          (3, LDS_LINE + 1, 66), (LDS_LINE + 1, 3, 66)]
PITCHES = [None, (40, 4, 4), (10, 1, 3), (0.025, 0.01, 0.01), (1.7, 0.3, 1.1)]


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


def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'edt_kat.json')) as f:
        g = json.load(f)
    for c in g['cases']:
        shape = tuple(c['shape'])
        c['shape'] = shape
        c['source'] = np.array(c['source'], dtype=np.uint8).reshape(shape)
        c['d2'] = np.array(c['d2'], dtype=np.float64).reshape(shape)
    return g
