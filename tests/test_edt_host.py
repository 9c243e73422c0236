"""The exact Euclidean distance transform on the CPU.  The functions the
kernels of ctg_edt.hip run (csrc/ctg_edt.h: the row's seed words and their
nearest-seed lookups, the envelope's push and seek, D2, the diagonal) and the
plan functions (csrc/ctg_plan.h: edt_line_plan, edt_passes) are driven by
tools/edt_check.cpp -- a serial rendering of the three passes, built with the
host compiler and -fsanitize=address,undefined and run as a child process --
and its answers are compared with the oracles of tests/edt_cases.py and the
golden fixture.  Then the oracles against each other and the fixture, and the
argument rules that raise before any library call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import edt_cases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def edt(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('edt') / 'edt_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'edt_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def ask(queries):
        r = subprocess.run([exe], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


def query(seeds, pitch, two_d):
    p = E.pitch3(pitch)
    return 'edt %d %d %d %s %s %s %d ' % (seeds.shape + tuple(float(v).hex() for v in p) + (int(two_d),)) + \
        ''.join('1' if v else '0' for v in np.asarray(seeds).ravel())


def parse(line, shape):
    t = line.split()
    info = (int(t[0]), int(t[1]), int(t[2]), float(np.array([int(t[3], 16)], dtype=np.uint64).view(np.float64)[0]))
    dist = np.array([int(w, 16) for w in t[4:]], dtype=np.uint32).view(np.float32).reshape(shape)
    return dist, info


# --------------------------------------------------------------------------- plan functions
def test_line_plan(edt):
    L = E.LDS_LINE
    got = [[int(t) for t in line.split()] for line in
           edt(['plan 1 5 70', 'plan %d 3 66' % L, 'plan %d 3 66' % (L + 1), 'plan 32767 2 64', 'plan 32767 1000 6400'])]
    assert got[0] == [1, 10, 10, 0]                            # a line of one voxel: in LDS, no buffer
    assert got[1] == [1, 6, 6, 0]                              # the longest line whose stacks fit LDS
    assert got[2] == [0, 6, 6, 6 * (L + 1) * 64 * 8]           # one more: the buffer, depth x workgroup x lane entries
    assert got[3] == [0, 2, 2, 2 * 32767 * 64 * 8]
    lds, groups, grid, nbytes = got[4]                         # the longest line over many columns: the grid shrinks
    assert lds == 0 and groups == 100000 and 1 <= grid < groups
    assert nbytes == grid * 32767 * 64 * 8 <= 1 << 30
    # an LDS stack of L entries a lane is 64 x L x 8 bytes: at least two workgroups in a CU's 160 KiB
    assert 2 * 64 * L * 8 <= 160 << 10


def test_passes(edt):
    got = edt(['passes 5 6 7 0', 'passes 5 6 7 1', 'passes 1 6 7 0', 'passes 5 1 7 0', 'passes 1 1 7 0',
               'passes 1 70 1 0', 'passes 70 1 1 0'])
    assert got == ['1 1', '1 0', '1 0', '0 1', '1 0', '1 0', '0 1']


def test_cap_mirrors(edt):
    """The caps mirrored in tests/edt_cases.py against the plan functions: a
    change of EDT_X_WAVES, EDT_X_MAX_GRID or EDT_LINE_MAX_GRID fails here, not
    by quietly taking the second turn out of the GPU tests."""
    W, G, LG = E.X_WAVES, E.X_MAX_GRID, E.LINE_MAX_GRID
    rows = [1, W, W + 1, W * (G - 1), W * (G - 1) + 1, W * G, W * G + 1, 100 * W * G]
    got = [int(t) for t in edt(['xgrid %d' % r for r in rows])]
    assert got == [1, 1, 2, G - 1, G, G, G, G]
    L = E.LDS_LINE
    got = [[int(t) for t in line.split()] for line in
           edt(['plan 2 %d 64' % LG, 'plan 2 %d 64' % (LG + 1), 'plan 2 %d 65' % LG,
                'plan %d %d 64' % (L + 1, LG), 'plan %d %d 64' % (L + 1, LG + 1)])]
    assert got[0] == [1, LG, LG, 0] and got[1] == [1, LG + 1, LG, 0] and got[2] == [1, 2 * LG, LG, 0]
    assert got[3] == [0, LG, LG, LG * (L + 1) * 64 * 8] and got[4] == [0, LG + 1, LG, LG * (L + 1) * 64 * 8]
    with open(os.path.join(ROOT, 'cluster_tools_amd', 'csrc', 'ctg_edt.hip')) as f:
        src = f.read()
    fold = src[src.index('void k_edt_fold('):src.index('void launch_line(')]
    assert 'i += %d)' % E.FOLD_THREADS in fold and 'dim3(%d), 0, s, part, n, info' % E.FOLD_THREADS in src


@pytest.mark.parametrize('shape', E.TURN_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_turn_shapes_cross_the_caps(edt, shape):
    """E.line_pass is the plan the library makes for the TURN_SHAPES boxes (no
    grid shrinks to fit the stack buffer, which stays under 150 MB), and each
    box takes the loops it is there for past their first turn."""
    nz, ny, nx = shape
    for two_d in (False, True):
        y, z = [bool(int(t)) for t in edt(['passes %d %d %d %d' % (shape + (int(two_d),))])[0].split()]
        for axis, runs in ((1, y), (0, z)):
            want = E.line_pass(shape, axis, two_d)
            assert want[0] == runs
            lds, groups, grid, nbytes = [int(t) for t in
                                         edt(['plan %d %d %d' % (shape[axis], nz if axis == 1 else ny, nx)])[0].split()]
            assert (bool(lds), groups, grid) == want[1:]
            assert nbytes == (0 if lds else grid * shape[axis] * 64 * 8) <= 150 << 20
    assert int(edt(['xgrid %d' % (nz * ny)])[0]) == min(-(-nz * ny // E.X_WAVES), E.X_MAX_GRID)
    crossed = {(8193, 33, 3): [E.x_turns(shape) > 8, E.line_pass(shape, 1)[1:] == (False, 8193, 8192)],
               (33, 8193, 3): [E.x_turns(shape) > 8, E.line_pass(shape, 0)[1:] == (False, 8193, 8192),
                               E.final_partials(shape) > E.FOLD_THREADS],
               (8193, 2, 3): [E.line_pass(shape, 1)[1:] == (True, 8193, 8192)],
               (2, 8193, 3): [E.line_pass(shape, 0)[1:] == (True, 8193, 8192),
                              E.final_partials(shape) > E.FOLD_THREADS]}[shape]
    assert all(crossed)


def test_two_d_oracle_in_one_call():
    """via_scipy_2d (one scipy call with a far z pitch) names the seeds via_scipy
    names slice by slice: equal D2, bit for bit, whatever the pitch."""
    for shape in ((40, 33, 3), (33, 50, 3), (50, 2, 3), (17, 9, 65)):
        for name in E.turn_pattern_names(shape) + ['diagonal', 'checkerboard']:
            for pitch in E.TURN_PITCHES + [(40, 4, 4), (0.025, 0.01, 0.01)]:
                seeds = E.patterns(shape)[name]
                np.testing.assert_array_equal(E.via_scipy_2d(seeds, pitch), E.via_scipy(seeds, pitch, True))


# --------------------------------------------------------------------------- the transform
@pytest.mark.parametrize('shape', E.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_host_transform_matches_oracle(edt, shape):
    """All patterns x pitches of a shape, 3-D, and the random ones in 2-D mode:
    bit-exact with integer pitches, within 1 float32 ulp otherwise; info entry
    for entry (tests/edt_cases.py: check)."""
    cases = [(name, pitch, False) for name in E.pattern_names(shape) for pitch in E.PITCHES]
    cases += [(name, pitch, True) for name in ('random_0.002', 'random_0.02', 'none', 'last_slice')
              for pitch in (None, (10, 1, 3), (1.7, 0.3, 1.1))]
    answers = edt([query(E.case(shape, name, pitch, two_d)[0], pitch, two_d) for name, pitch, two_d in cases])
    for (name, pitch, two_d), line in zip(cases, answers):
        seeds, d2 = E.case(shape, name, pitch, two_d)
        dist, info = parse(line, shape)
        try:
            E.check(dist, info, seeds, pitch, two_d, d2)
        except AssertionError as err:
            raise AssertionError('%s pitch %s two_d %s: %s' % (name, pitch, two_d, err)) from None


def test_golden(edt):
    """The hand-computed cases: both oracles and the host rendering give them."""
    g = E.golden()
    assert len(g['cases']) == 3
    assert {(c['to_background'], c['two_d']) for c in g['cases']} == {(False, False), (False, True), (True, False)}
    for c in g['cases']:
        pitch = None if c['pitch'] is None else tuple(c['pitch'])
        seeds = (c['source'] != 0) != c['to_background']
        for oracle in (E.brute, E.via_scipy):
            np.testing.assert_array_equal(oracle(seeds, pitch, c['two_d']), c['d2'])
        dist, info = parse(edt([query(seeds, pitch, c['two_d'])])[0], c['shape'])
        np.testing.assert_array_equal(dist, np.sqrt(c['d2']).astype(np.float32))
        assert list(info) == c['info']
        E.check(dist, info, seeds, pitch, c['two_d'], c['d2'])


# --------------------------------------------------------------------------- long rows, deep stacks, the bound
def ask_cases(edt, cases):
    """[(seeds, pitch, two_d)] -> [(dist, info)] in one run of the tool."""
    lines = edt([query(seeds, pitch, two_d) for seeds, pitch, two_d in cases])
    return [parse(line, seeds.shape) for line, (seeds, _, _) in zip(lines, cases)]


@pytest.mark.parametrize('nx', E.LONG_ROWS)
def test_long_rows(edt, nx):
    """edt_prev_seed / edt_next_seed (csrc/ctg_edt.h) past one top word, rows of
    more than E.ROW_TOP = 4096 voxels: the walks over the top words in both
    directions and the (w & 63) == 0 / == 63 edges, seeds at the row's ends, on
    both sides of a top-word border and in the second top word.  The oracle is
    min |x - seed| per row, combined across the rows by brute force; scipy
    agrees with it."""
    assert nx > E.ROW_TOP
    cases = E.long_row_cases(nx)
    for (seeds, d2), (dist, info) in zip(cases, ask_cases(edt, [(s, None, False) for s, _ in cases])):
        np.testing.assert_array_equal(d2, E.via_scipy(seeds))
        E.check(dist, info, seeds, None, False, d2)


@pytest.mark.parametrize('shape', E.DEEP_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_deep_stacks(edt, shape):
    """Lines of 4099 and 300 positions whose envelope keeps every parabola
    ('diagonal') or pops often ('random_0.3'): stacks thousands of entries deep."""
    cases = [(name, pitch) for name in E.DEEP_PATTERNS for pitch in E.DEEP_PITCHES]
    answers = ask_cases(edt, [(E.case(shape, name, pitch)[0], pitch, False) for name, pitch in cases])
    for (name, pitch), (dist, info) in zip(cases, answers):
        seeds, d2 = E.case(shape, name, pitch)
        E.check(dist, info, seeds, pitch, False, d2)


@pytest.mark.parametrize('shape', E.BOUND_SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_integer_pitches_up_to_the_bound(edt, shape):
    """Integer pitches up to (nz pz)^2 + (ny py)^2 + (nx px)^2 < 2^53, where the
    contract still promises bit-exactness and edt_takeover's floor is argued to
    be the true one: against brute force (scipy's own arithmetic is no oracle
    here).  The bound is asserted of every case -- a condition on the inputs."""
    cases = [(pitch, density) for pitch in E.bound_pitches(shape) for density in E.BOUND_DENSITIES]
    assert E.diag2(shape, cases[-1][0], False) > 0.97 * E.BOUND or cases[-1][0][0] == 94906265 // max(shape)
    for pitch, _ in cases:
        assert E.is_exact(pitch) and E.diag2(shape, pitch, False) < E.BOUND
    answers = ask_cases(edt, [(E.bound_case(shape, pitch, density)[0], pitch, False) for pitch, density in cases])
    for (pitch, density), (dist, info) in zip(cases, answers):
        seeds, d2 = E.bound_case(shape, pitch, density)
        E.check(dist, info, seeds, pitch, False, d2)


# --------------------------------------------------------------------------- the D2 expression
def single_seed_cases():
    out = [(shape, name, E.patterns(shape)[name], pitch, False) for shape in E.SINGLE_SHAPES
           for name in E.corner_names(shape) for pitch in E.SINGLE_PITCHES]
    out += [(shape, 'one_per_slice', E.one_per_slice(shape), pitch, True) for shape in E.SINGLE_SHAPES
            for pitch in E.SINGLE_PITCHES]
    return out


def test_single_seed_pins_the_expression(edt):
    """One seed a domain: the host rendering gives float32(sqrt(D2)) and the
    largest D2 of the contract's expression bit for bit under non-integer
    pitches (E.check_single_seed; the GPU test also compares D2 itself)."""
    cases = single_seed_cases()
    assert len(cases) == 2 * 8 * 2 + 2 * 2
    for (shape, name, seeds, pitch, two_d), (dist, info) in \
            zip(cases, ask_cases(edt, [(seeds, pitch, two_d) for _, _, seeds, pitch, two_d in cases])):
        E.check_single_seed(seeds, pitch, two_d, dist, info)


def test_single_seed_cases_would_notice_a_contraction():
    """Every single-seed case has voxels whose D2 differs when the sum is
    contracted into fused multiply-adds, either way round: without that the
    case would pin neither -ffp-contract=off nor the order of the additions.
    A reordered sum (the x term first) differs somewhere too."""
    for shape, name, seeds, pitch, two_d in single_seed_cases():
        want = E.single_seed_d2(seeds, pitch, two_d)
        for other in E.contracted_d2(seeds, pitch, two_d):
            assert (other != want).sum() >= 10, (shape, name, pitch)
        g = np.indices(shape)
        p = E.pitch3(pitch)
        far = np.abs(g - np.array([n - 1 for n in shape]).reshape(3, 1, 1, 1))      # reordering: any offsets will do
        a, b, c = (far[k].astype(np.float64) * p[k] for k in range(3))
        assert ((c * c + b * b + a * a) != (a * a + b * b + c * c)).any()


# --------------------------------------------------------------------------- the oracle against itself
@pytest.mark.parametrize('two_d', [False, True])
def test_brute_force_matches_scipy(two_d):
    """A wrong oracle cannot pass silently: the minimum over all seeds equals
    the D2 of the seed scipy names, bit for bit with integer pitches, and
    scipy's own float64 distances are its square root."""
    from scipy import ndimage as ndi
    for shape in ((1, 1, 130), (1, 70, 1), (70, 1, 1), (5, 9, 13), (9, 7, 20)):
        for name in ('random_0.02', 'random_0.3', 'diagonal', 'checkerboard', 'plane_y', 'none', 'last_column'):
            seeds = E.patterns(shape)[name]
            for pitch in E.PITCHES:
                a, b = E.brute(seeds, pitch, two_d), E.via_scipy(seeds, pitch, two_d)
                if E.is_exact(pitch):
                    np.testing.assert_array_equal(a, b)
                    if seeds.any() and not two_d:
                        s = ndi.distance_transform_edt(~seeds, sampling=pitch)
                        np.testing.assert_array_equal(s.astype(np.float32), np.sqrt(a).astype(np.float32))
                else:
                    assert np.all(a <= b) and np.allclose(a, b, rtol=1e-14, atol=0)
                    assert int(E.ulps(np.sqrt(a).astype(np.float32), np.sqrt(b).astype(np.float32)).max()) <= 1


# --------------------------------------------------------------------------- argument rules before the library
def test_argument_rules(monkeypatch):
    from cluster_tools_amd import _lib, distance, rag

    def no_library(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'load', no_library)
    monkeypatch.setattr(_lib, 'init_device', no_library)
    vol = np.zeros((2, 3, 4), dtype=np.uint8)
    lab = np.zeros((2, 3, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match='3-D'):
        rag.distance_transform(vol[0])
    with pytest.raises(ValueError, match='3-D'):
        rag.distance_transform(vol[None])
    for bad in ((1, 0, 1), (1, -2, 1), (1, float('nan'), 1), (float('inf'), 1, 1)):
        with pytest.raises(ValueError, match='finite and positive'):
            rag.distance_transform(vol, pitch=bad)
    for bad in ((1, 1), (1, 1, 1, 1)):
        with pytest.raises(ValueError, match='3 entries'):
            rag.distance_transform(vol, pitch=bad)
    with pytest.raises(ValueError, match='outside'):
        rag.distance_transform(vol, begin=(0, 0, 0), end=(2, 3, 5))
    with pytest.raises(ValueError, match='outside'):
        rag.distance_transform(vol, begin=(1, 2, 3), end=(2, 1, 4))
    with pytest.raises(ValueError, match='threshold'):
        rag.distance_transform(lab, threshold=0.5)                       # a threshold with a label source
    with pytest.raises(ValueError, match='not both'):
        rag.distance_transform(lab, threshold=0.5, label=3)
    with pytest.raises(ValueError, match='label'):
        rag.distance_transform(vol.astype(np.float32), label=3)
    with pytest.raises(ValueError, match='uint8 or bool'):
        rag.distance_transform(vol.astype(np.float32))
    with pytest.raises(ValueError, match='uint64 value'):
        rag.distance_transform(lab, label=-1)
    with pytest.raises(ValueError, match='out must'):
        rag.distance_transform(vol, out=np.zeros((2, 3, 5), dtype=np.float32))
    with pytest.raises(ValueError, match='out must'):
        rag.distance_transform(vol, out=np.zeros((2, 3, 4), dtype=np.float64))
    with pytest.raises(ValueError, match='out must'):
        rag.distance_transform(vol, begin=(0, 0, 1), out=np.zeros((2, 3, 4), dtype=np.float32))
    torch = pytest.importorskip('torch')
    with pytest.raises(ValueError, match='same kind'):                   # mixed numpy / tensor
        rag.distance_transform(vol, out=torch.zeros((2, 3, 4), dtype=torch.float32))
    with pytest.raises(ValueError, match='contiguous CUDA'):
        rag.distance_transform(torch.zeros((2, 3, 4), dtype=torch.uint8))
    # the mirrors
    with pytest.raises(ValueError, match='2-D or 3-D'):
        distance.distanceTransform(np.zeros(5, dtype=np.uint32))
    with pytest.raises(ValueError, match='2-D or 3-D'):
        distance.distance_transform_edt(np.zeros((2, 2, 2, 2), dtype=bool))
    with pytest.raises(ValueError, match='entries'):
        distance.distanceTransform(np.zeros((4, 5), dtype=np.uint32), pixel_pitch=(1, 1, 1))
    with pytest.raises(ValueError, match='finite and positive'):
        distance.distance_transform_edt(np.zeros((4, 5), dtype=bool), sampling=(1, 0))
    with pytest.raises(AssertionError):
        distance.apply_dt(np.zeros((2, 3, 4), dtype=np.float32), pixel_pitch=(2, 1, 1), apply_dt_2d=True)
