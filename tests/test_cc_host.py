"""The thresholded components on the CPU.  The union-find and the run-head bit
helpers the kernels of ctg_cc.hip run (csrc/ctg_uf.h) and the labelling's plan
functions (csrc/ctg_plan.h: the neighbour-row table, the tile grid, the seam
threads) are driven by tools/cc_check.cpp -- a serial rendering of the tile,
seam, flatten and number steps, built with the host compiler and
-fsanitize=address,undefined -- and its answers are compared with the oracle of
tests/cc_cases.py, a Python dict union-find and the golden fixture.  Then the
oracle itself against scipy and the fixture, merge_offsets against hand-written
tables, and the argument rules that raise before any library call."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import cc_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cc(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('cc') / 'cc_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'cc_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def ask(queries):
        r = subprocess.run([exe], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


def host_label(cc, fg, c):
    fg = np.asarray(fg)
    q = 'label %d %d %d %d ' % ((c,) + fg.shape) + ' '.join('1' if v else '0' for v in fg.ravel())
    t = cc([q])[0].split()
    return np.array(t[1:], dtype=np.uint64).reshape(fg.shape), int(t[0])


# --------------------------------------------------------------------------- plan functions
def test_neighbor_rows(cc):
    rows = [[int(t) for t in line.split()] for line in cc(['rows 1', 'rows 2', 'rows 3'])]
    assert rows[0] == [2, 0, -1, 0, -1, 0, 0]
    assert rows[1] == [4, 0, -1, 1, -1, 0, 1, -1, -1, 0, -1, 1, 0]
    assert rows[2] == [4, 0, -1, 1, -1, 0, 1, -1, -1, 1, -1, 1, 1]
    # the rows with their dilation are the earlier half of the neighbourhood: 3, 9, 13 offsets
    for c, row in zip((1, 2, 3), rows):
        half = set()
        for k in range(row[0]):
            dz, dy, dil = row[1 + 3 * k:4 + 3 * k]
            half |= {(dz, dy, dx) for dx in ((-1, 0, 1) if dil else (0,))}
        half.add((0, 0, -1))                                  # (within a row: the run itself)
        want = {d for d in C.offsets(c) if d < (0, 0, 0)}
        assert half == want


def test_grid(cc):
    got = [[int(t) for t in line.split()] for line in
           cc(['grid 1 1 1', 'grid 16 8 64', 'grid 17 9 65', 'grid 33 17 129', 'grid 0 5 5', 'grid 1 1 130'])]
    assert got[0] == [1, 1, 1, 0, 0, 0, 1]
    assert got[1] == [1, 1, 1, 0, 0, 0, 4]                    # exactly one tile: no seam
    assert got[2] == [2, 2, 2, 17 * 9, 17 * 65, 9 * 65, -(-17 * 9 * 65 // 2048)]
    assert got[3] == [3, 3, 3, 2 * 33 * 17, 2 * 33 * 129, 2 * 17 * 129, -(-33 * 17 * 129 // 2048)]
    assert got[4] == [0, 1, 1, 0, 0, 0, 0]
    assert got[5] == [1, 1, 3, 2, 0, 0, 1]


def test_cap_mirrors(cc):
    """The caps mirrored in tests/cc_cases.py: CC_SEG through the grid's segment
    count (cc_segments), the scan step and the range launch through the text of
    csrc/ctg_cc.hip, which holds them as literals.  A change fails here instead
    of taking the second step or turn out of tests/test_gpu_cc.py."""
    got = [[int(t) for t in line.split()] for line in
           cc(['grid 1 1 %d' % C.SEG, 'grid 1 1 %d' % (C.SEG + 1), 'grid 128 128 128', 'grid %d %d %d' % C.BIG])]
    assert [g[6] for g in got] == [1, 2, C.SCAN_STEP, 1032]
    assert got[3][0] * got[3][1] * got[3][2] == 9 * 16 * 2 == 288
    assert C.scan_steps(C.SEG * C.SCAN_STEP) == 1 and C.scan_steps(C.SEG * C.SCAN_STEP + 1) == 2
    assert C.scan_steps(int(np.prod(C.BIG))) == 2 and C.BIG[0] * C.BIG[1] > 2 * C.RANGE_ROWS
    with open(os.path.join(ROOT, 'cluster_tools_amd', 'csrc', 'ctg_cc.hip')) as f:
        src = f.read()
    scan = src[src.index('void k_uf_scan('):src.index('uf_id(')]
    assert '__launch_bounds__(%d) void k_uf_scan(' % C.SCAN_STEP in src
    assert 'base += %d)' % C.SCAN_STEP in scan and 'k_uf_scan, dim3(1), dim3(%d)' % C.SCAN_STEP in src
    assert 'std::min<int64_t>((rows + 3) / 4, %d)' % (C.RANGE_ROWS // 4) in src


# --------------------------------------------------------------------------- the labelling
SHAPES = [(1, 1, 1), (1, 1, 130), (16, 8, 64), (17, 9, 65), (5, 9, 70), (33, 17, 129)]


@pytest.mark.parametrize('c', [1, 2, 3])
def test_host_labelling_matches_oracle(cc, c):
    for shape in SHAPES:
        for p in ((0.25, 0.45) if c == 1 else (0.08, 0.15)) + (1.0, 0.0):
            fg = C.random_fg(shape, p, seed=len(shape) + shape[2] + c)
            want, n = C.oracle_label(fg, c)
            got, m = host_label(cc, fg, c)
            assert m == n, (shape, p)
            assert_array_equal(got, want)


@pytest.mark.parametrize('c', [1, 2, 3])
def test_host_labelling_structures(cc, c):
    for fg in (C.checkerboard((4, 9, 66)), C.serpentine(), C.u_shape()):
        want, n = C.oracle_label(fg, c)
        got, m = host_label(cc, fg, c)
        assert m == n
        assert_array_equal(got, want)
    assert C.oracle_label(C.serpentine(), c)[1] == 1 and C.oracle_label(C.u_shape(), c)[1] == 1
    if c == 1:
        assert C.oracle_label(C.checkerboard((4, 9, 66)), 1)[1] == 4 * 9 * 66 // 2
    else:
        assert C.oracle_label(C.checkerboard((4, 9, 66)), c)[1] == 1


def test_golden(cc):
    """The hand-computed case: the oracle and the host rendering both give it."""
    g = C.golden()
    assert_array_equal(C.normalize(g['values']), g['normalized'])
    assert len({(k['connectivity'], k['n']) for k in g['cases'] if k['mode'] == 'greater' and not k['mask']}) == 3
    for case in g['cases']:
        fg = C.foreground(g['values'], case['threshold'], case['mode'], case['normalize'],
                          g['mask'] if case['mask'] else None)
        want, n = C.oracle_label(fg, case['connectivity'])
        assert n == case['n']
        assert_array_equal(want, case['labels'])
        got, m = host_label(cc, fg, case['connectivity'])
        assert m == n
        assert_array_equal(got, case['labels'])


@pytest.mark.parametrize('c', [1, 2, 3])
def test_oracle_matches_scipy(c):
    ndi = pytest.importorskip('scipy.ndimage')
    for shape in ((5, 9, 70), (17, 9, 130), (33, 17, 65)):
        for p in (0.08, 0.15, 0.25, 0.45):
            fg = C.random_fg(shape, p, seed=7)
            want, n = ndi.label(fg, structure=ndi.generate_binary_structure(3, c))
            got, m = C.oracle_label(fg, c)
            assert m == n
            assert_array_equal(got, want.astype(np.uint64))


# --------------------------------------------------------------------------- the merge
def host_merge(cc, pairs, n_labels):
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    t = cc(['merge %d %d ' % (n_labels, len(pairs)) + ' '.join(str(int(v)) for v in pairs.ravel())])[0].split()
    return t


def test_host_merge_against_a_dict(cc):
    rng = np.random.default_rng(5)
    n_labels = 20000
    cases = [rng.integers(1, n_labels, size=(15000, 2)),
             rng.permutation(np.stack([np.arange(1, 5000), np.arange(2, 5001)], 1)),          # a chain, shuffled
             np.stack([np.full(300, 7), np.arange(8, 308)], 1),                               # a star
             np.array([[3, 9], [9, 3], [3, 9], [n_labels - 1, 3]]),                           # repeats, reversed, the last id
             np.zeros((0, 2), dtype=np.int64)]
    for pairs in cases:
        t = host_merge(cc, pairs, n_labels)
        want, max_id = C.merge_table(pairs, n_labels)
        assert int(t[0]) == max_id
        assert_array_equal(np.array(t[1:], dtype=np.uint64), want)
        fast, fast_max = C.merge_table_fast(pairs, n_labels)               # the oracle of the large cases
        assert fast.dtype == want.dtype and fast_max == max_id
        assert_array_equal(fast, want)
    t = host_merge(cc, cases[-1], n_labels)
    assert_array_equal(np.array(t[1:], dtype=np.uint64), np.arange(n_labels, dtype=np.uint64))   # no pairs: the identity


def test_host_merge_refuses_bad_members(cc):
    assert host_merge(cc, [[1, 10]], 10) == ['bad']
    assert host_merge(cc, [[0, 3]], 10) == ['bad']
    assert host_merge(cc, [[3, 0]], 10) == ['bad']
    assert host_merge(cc, [[1, 9]], 10)[0] == '8'
    assert cc(['merge %d 0' % (1 << 32)]) == ['unsupported']


def test_step_cap_fires_on_a_cycle(cc):
    """A parent array that is no forest -- 1 -> 2 -> 3 -> 1 -- never reaches a
    root: uf_find stops at its cap and says so (host code only)."""
    over, _ = cc(['find 4 1 0 2 3 1'])[0].split()
    assert over == '1'
    assert cc(['find 4 3 0 0 1 2'])[0].split() == ['0', '0']       # a chain of all four nodes fits the cap exactly
    assert cc(['find 3 3 0 0 1 2'])[0].split()[0] == '1'           # ... and not a smaller one


# --------------------------------------------------------------------------- merge_offsets
def test_merge_offsets():
    from cluster_tools_amd.thresholded_components import merge_offsets
    # contributions max + 1 per block, keys as the job files hold them (any order, str or int)
    assert merge_offsets({'2': 4, '0': 3, '1': 0, '3': 6}) == dict(offsets=[0, 3, 3, 7], empty_blocks=[1], n_labels=14)
    assert merge_offsets({0: 0, 1: 5, 2: 2}) == dict(offsets=[0, 0, 5], empty_blocks=[0], n_labels=8)       # first empty
    assert merge_offsets({0: 5, 1: 2, 2: 0}) == dict(offsets=[0, 5, 7], empty_blocks=[2], n_labels=8)       # last empty
    assert merge_offsets({0: 0, 1: 0, 2: 0}) == dict(offsets=[0, 0, 0], empty_blocks=[0, 1, 2], n_labels=1)  # all empty
    assert merge_offsets({10: 2, 9: 3}) == dict(offsets=[0, 3], empty_blocks=[], n_labels=6)               # no string sort
    out = merge_offsets({0: 3, 1: 4})
    assert all(type(v) is int for v in out['offsets']) and type(out['n_labels']) is int                    # JSON-ready


# --------------------------------------------------------------------------- argument rules before the library
def test_argument_rules(monkeypatch):
    from cluster_tools_amd import _lib, rag

    def no_library(*a, **k):
        raise AssertionError('the library was called')
    monkeypatch.setattr(_lib, 'load', no_library)
    monkeypatch.setattr(_lib, 'init_device', no_library)
    vol = np.zeros((2, 3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match='mode'):
        rag.threshold_components(vol, 0.5, mode='above')
    for c in (0, 4):
        with pytest.raises(ValueError, match='connectivity'):
            rag.threshold_components(vol, 0.5, connectivity=c)
    with pytest.raises(ValueError, match='mask shape'):
        rag.threshold_components(vol, 0.5, mask=np.ones((2, 3, 5), dtype=np.uint8))
    with pytest.raises(TypeError, match='mask'):
        rag.threshold_components(vol, 0.5, mask=np.ones((2, 3, 4), dtype=np.float32))
    with pytest.raises(ValueError, match='3-D'):
        rag.threshold_components(vol[0], 0.5)
    with pytest.raises(TypeError, match='float32 or uint8'):
        rag.threshold_components(vol.astype(np.float64), 0.5)
    with pytest.raises(ValueError, match='outside'):
        rag.threshold_components(vol, 0.5, begin=(0, 0, 0), end=(2, 3, 5))
    with pytest.raises(ValueError, match='out must'):
        rag.threshold_components(vol, 0.5, out=np.zeros((2, 3, 4), dtype=np.uint32))
    for bad in (np.zeros((3, 3), dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros((2, 2, 2), dtype=np.uint64)):
        with pytest.raises(ValueError, match=r'\(n, 2\)'):
            rag.merge_assignments(bad, 10)
    with pytest.raises(TypeError, match='integers'):
        rag.merge_assignments(np.zeros((3, 2), dtype=np.float32), 10)
    with pytest.raises(ValueError, match='negative'):
        rag.merge_assignments(np.array([[1, -2]]), 10)
    with pytest.raises(ValueError, match='2\\^32'):
        rag.merge_assignments(np.zeros((0, 2), dtype=np.uint64), 1 << 32)
    for bad in (np.zeros(9, dtype=np.uint64), np.zeros(10, dtype=np.uint32), np.zeros((10, 1), dtype=np.uint64)):
        with pytest.raises(ValueError, match='out must'):
            rag.merge_assignments(np.array([[1, 2]]), 10, out=bad)
