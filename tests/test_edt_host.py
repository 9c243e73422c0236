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
