"""The seeded watershed on the CPU.  The two oracles of tests/ws_cases.py agree
with each other and with the golden fixture; every label attains the minimal
pass height; a priority flood with FIFO ties differs from the rule only where
two labels tie in pass height.  The functions the kernels of ctg_ws.hip run
(csrc/ctg_ws.h: the key, the order, the pick, the hook, the chase) and the plan
functions (csrc/ctg_plan.h) are driven by tools/ws_check.cpp -- the rounds
rendered serially, built with the host compiler and
-fsanitize=address,undefined -- and its answers are compared with the oracle.
Then the argument rules that raise before any library call."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import rag
from tests import ws_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = W.load_kats(os.path.join(ROOT, 'tests', 'golden', 'ws_kat.json'))
SMALL = [(1, 1, 1), (1, 1, 40), (3, 4, 5), (2, 7, 9), (5, 6, 7)]


@pytest.fixture(scope='module')
def ws(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('ws') / 'ws_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'ws_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def ask(queries):
        r = subprocess.run([exe], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


def flood_query(h, s, two_d):
    h = np.ascontiguousarray(h, dtype=np.float32)
    return 'flood %d %d %d %d ' % ((int(two_d),) + h.shape) + ' '.join(map(str, h.view(np.uint32).ravel())) + \
        ' ' + ' '.join(map(str, np.asarray(s, dtype=np.uint64).ravel()))


def host_floods(ws, cases):
    """[(labels, rounds, chase launches)] of (h, s, two_d) cases, one process for all."""
    out = []
    for (h, s, _), line in zip(cases, ws([flood_query(*c) for c in cases])):
        t = line.split()
        out.append((np.array(t[2:], dtype=np.uint64).reshape(h.shape), int(t[0]), int(t[1])))
    return out


# --------------------------------------------------------------------------- the rule
def test_key_order():
    v = np.array([-np.inf, -2.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32)
    k = W.key_u32(v).astype(np.int64)
    assert k[3] == k[4] == 0x80000000
    assert (np.diff(np.delete(k, 3)) > 0).all()
    assert k[0] == 0x007FFFFF and k[-1] == 0xFF800000


@pytest.mark.parametrize('c', KATS, ids=[c['name'] for c in KATS])
def test_oracles_match_the_fixture(c):
    assert_array_equal(W.oracle_kruskal(c['hmap'], c['seeds'], c['two_d']), c['labels'])
    assert_array_equal(W.oracle_fast(c['hmap'], c['seeds'], c['two_d']), c['labels'])


@pytest.mark.parametrize('two_d', [False, True])
@pytest.mark.parametrize('hk', W.HEIGHTS)
def test_oracles_agree(hk, two_d):
    for shape in SMALL + [(17, 9, 65)]:
        for sk in W.SEEDS:
            h, s = W.heights(hk, shape, seed=1), W.seeds(sk, shape, seed=2)
            assert_array_equal(W.oracle_fast(h, s, two_d), W.oracle_kruskal(h, s, two_d), err_msg=str((shape, sk)))


@pytest.mark.parametrize('two_d', [False, True])
@pytest.mark.parametrize('hk', ['distinct', 'levels2', 'levels8', 'levels256', 'special'])
def test_labels_attain_the_minimal_pass_height(hk, two_d):
    for shape in SMALL[2:]:
        for sk in ('scattered', 'blobs', 'one'):
            h, s = W.heights(hk, shape, seed=3), W.seeds(sk, shape, seed=4)
            got = W.oracle_kruskal(h, s, two_d)
            best = W.pass_height(h, s != 0, two_d)
            assert_array_equal(got == 0, best < 0)      # 0 exactly where no seed is reachable
            for lab in np.unique(got[got != 0]):
                mine = W.pass_height(h, s == lab, two_d)
                assert_array_equal(mine[got == lab], best[got == lab])


@pytest.mark.parametrize('hk', ['distinct', 'levels2', 'levels8', 'levels256'])
def test_fifo_flood_differs_only_in_tie_zones(hk):
    """The deviation from vigra's flood, documented: outside the voxels where two
    labels tie in pass height the two agree.  (Ties exist with distinct heights
    too: a voxel higher than every path to it ties all its neighbours' labels.)"""
    n_free = n_all = 0
    for shape in SMALL[2:] + [(4, 9, 20)]:
        h, s = W.heights(hk, shape, seed=5), W.seeds('scattered', shape, seed=6)
        at = np.arange(0, s.size, max(1, s.size // 7))
        s.ravel()[at] = 101 + np.arange(at.size, dtype=np.uint64)
        got, flood = W.oracle_kruskal(h, s), W.fifo_flood(h, s)
        ties = W.tie_zone(h, s)
        assert_array_equal(got[~ties], flood[~ties])
        n_free += int((~ties & (s == 0)).sum())
        n_all += int((s == 0).sum())
    # not vacuous: unseeded voxels outside the tie zones exist (with seeds this dense, a minority)
    assert 0 < n_free < n_all


def test_size_filter_oracle():
    h = np.zeros((1, 1, 10), dtype=np.float32)
    s = np.array([1, 0, 0, 0, 0, 0, 0, 2, 0, 0], dtype=np.uint64).reshape(1, 1, 10)
    out, info = W.oracle(h, s, 0)
    assert out.ravel().tolist() == [1] * 7 + [2] * 3 and info == (2, 0, 0)
    assert W.oracle(h, s, 3)[0].ravel().tolist() == [1] * 7 + [2] * 3          # a size equal to the limit is kept
    out, info = W.oracle(h, s, 4)
    assert out.ravel().tolist() == [1] * 10 and info == (1, 0, 1)              # its seed went with it
    out, info = W.oracle(h, s, 8)
    assert not out.any() and info == (0, 10, 2)


# --------------------------------------------------------------------------- the host rendering
def test_key_and_plan_functions(ws):
    bits = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], dtype=np.float32).view(np.uint32)
    got = [int(t) for t in ws(['key %d' % b for b in bits])]
    assert got == W.key_u32(bits.view(np.float32)).tolist()
    # ceil(log2(U + 1)) + 1
    assert [int(t) for t in ws(['cap %d' % u for u in (0, 1, 2, 3, 4, 7, 8, 129, (1 << 30) - 1, 1 << 30)])] == \
        [1, 2, 3, 3, 4, 4, 5, 9, 31, 32]
    plan = [[int(t) for t in line.split()] for line in
            ws(['plan 1 1 1 0', 'plan 17 9 65 0', 'plan 17 9 65 1', 'plan 1024 1024 1024 0'])]
    assert plan[0] == [1, 1, 4, 4, 8, 4, 1]
    assert plan[1] == [9945, 39, 39780, 39780, 79560, 39780, 1] and plan[2][6] == 17
    assert plan[3][:2] == [1 << 30, 4096]                     # the grid is capped: the workgroups stride
    # the mirror of the cap in tests/ws_cases.py: the last box of one turn, the first of two
    turn = [[int(t) for t in line.split()] for line in
            ws(['plan 1 1 %d 0' % (W.GRID_TURN - 256), 'plan 1 1 %d 0' % W.GRID_TURN, 'plan %d %d %d 0' % W.BIG])]
    assert [p[1] for p in turn] == [4095, 4096, 4096]
    assert W.GRID_TURN < turn[2][0] < 2 * W.GRID_TURN and turn[2][0] % 256 != 0
    assert [W.round_bound(np.zeros(u)) for u in (0, 1, 2, 3, 4, 129)] == [1, 2, 3, 3, 4, 9]


@pytest.mark.parametrize('c', KATS, ids=[c['name'] for c in KATS])
def test_host_rendering_matches_the_fixture(ws, c):
    got, rounds, _ = host_floods(ws, [(c['hmap'], c['seeds'], c['two_d'])])[0]
    assert_array_equal(got, c['labels'])
    assert rounds <= W.round_bound(c['seeds'])


@pytest.mark.parametrize('two_d', [False, True])
@pytest.mark.parametrize('shape', W.SHAPES)
def test_host_rendering_matches_the_oracle(ws, shape, two_d):
    cases = [(W.heights(hk, shape, seed=shape[2]), W.seeds(sk, shape, seed=shape[0]), two_d)
             for hk in W.HEIGHTS for sk in W.SEEDS]
    segments = 0
    for (h, s, _), (got, rounds, launches) in zip(cases, host_floods(ws, cases)):
        want = W.oracle_fast(h, s, two_d)
        assert_array_equal(got, want)
        assert rounds <= W.round_bound(s)
        assert launches <= 6
        segments = max(segments, W.n_segments(want))
    if shape[2] > 64:
        assert segments >= 2


def test_host_rendering_takes_rounds_not_steps(ws):
    """A ramp far from its seed: every voxel hooks to its lower neighbour in the
    first round, and the chase flattens a chain longer than one launch follows."""
    h = W.heights('ramp', (1, 1, 300))
    s = np.zeros(h.shape, dtype=np.uint64)
    s[0, 0, 0] = 4
    got, rounds, launches = host_floods(ws, [(h, s, False)])[0]
    assert (got == 4).all() and rounds == 2 and launches == 2


# --------------------------------------------------------------------------- argument rules
def test_argument_rules_raise_before_the_library(monkeypatch):
    monkeypatch.setattr(rag.L, 'load', lambda: pytest.fail('the library was reached'))
    h = np.zeros((2, 3, 4), dtype=np.float32)
    s = np.zeros((2, 3, 4), dtype=np.uint64)
    with pytest.raises(TypeError):
        rag.seeded_watershed(h.astype(np.float64), s)
    with pytest.raises(TypeError):
        rag.seeded_watershed(h, s.astype(np.uint8))
    with pytest.raises(TypeError):
        rag.seeded_watershed(h, s.astype(np.float32))
    with pytest.raises(ValueError):
        rag.seeded_watershed(h[0], s[0])
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s[:, :, :3])
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, begin=(0, 0))
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, begin=(0, 0, 2), end=(2, 3, 1))
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, end=(2, 3, 5))
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, size_filter=-1)
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, out=np.zeros((2, 3, 4), dtype=np.uint32))
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, out=np.zeros((2, 3, 3), dtype=np.uint64))
    with pytest.raises(ValueError):   # in place: 64-bit seeds and the whole array only
        s32 = s.astype(np.uint32)
        rag.seeded_watershed(h, s32, out=s32)
    with pytest.raises(ValueError):
        rag.seeded_watershed(h, s, end=(1, 3, 4), out=s)
    # the 2^30 limit, on arrays that take no memory
    big = (1025, 1024, 1024)
    with pytest.raises(ValueError, match='2\\^30'):
        rag.seeded_watershed(np.broadcast_to(np.float32(0), big), np.broadcast_to(np.uint64(0), big))
    # a NaN counts inside the box only
    bad = h.copy()
    bad[1, 2, 3] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        rag.seeded_watershed(bad, s)
    with pytest.raises(pytest.fail.Exception, match='reached'):
        rag.seeded_watershed(bad, s, end=(1, 3, 4))
    with pytest.raises(pytest.fail.Exception, match='reached'):   # +-inf are ordinary heights
        rag.seeded_watershed(np.full((2, 3, 4), np.inf, dtype=np.float32), s)
