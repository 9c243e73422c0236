"""The sparse assignment's hash table (csrc/ctg_take.h: the hash, insert and
lookup functions the kernels of ctg_take.hip run) and the two host decisions of
the apply call (csrc/ctg_plan.h: take_capacity, take_chunk_prefix) on the CPU:
tools/take_check.cpp drives them -- built with the host compiler and
-fsanitize=address,undefined -- and its answers are compared with a Python dict
and the tables below.  Then the argument rules of the nifty.tools mirrors that
raise before any GPU call (no GPU, no library call)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 64) - 1
CHUNK = 4096


@pytest.fixture(scope='module')
def take(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('take') / 'take_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'take_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)

    def ask(queries):
        r = subprocess.run([exe], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return out
    return ask


def build_and_look(take, table, queries):
    """The table built from the dict, then the answers for ``queries`` (None: absent)."""
    b = 'build %d ' % len(table) + ' '.join('%d %d' % kv for kv in table.items())
    built, looked = take([b, 'look %d ' % len(queries) + ' '.join(str(q) for q in queries)])
    dups, cap = map(int, built.split())
    assert dups == 0
    return cap, [None if t == '-' else int(t) for t in looked.split()]


def test_capacity(take):
    ns = [0, 1, 31, 32, 33, 1 << 16, (1 << 16) + 1]
    got = [int(g) for g in take(['cap %d' % n for n in ns])]
    assert got == [64, 64, 64, 64, 128, 1 << 17, 1 << 18]
    for n, c in zip(ns, got):                 # a power of two of at least 2 n and at least 64
        assert c & (c - 1) == 0 and c >= max(64, 2 * n) and (c == 64 or c < 4 * n)


def test_count_slots(take):
    ns = [0, 1, 4096, 4097, 1 << 20]
    got = [int(g) for g in take(['slots %d' % n for n in ns])]
    assert got == [64, 64, 64, 1, 1]
    assert all(g & (g - 1) == 0 for g in got)        # the kernel masks the workgroup index with slots - 1


def test_cap_mirrors(take):
    """The caps mirrored in tests/take_cases.py against take_count_slots, the
    chunk plan and the text of launch_take_max (csrc/ctg_take.hip), which holds
    its grid as literals: a change fails here instead of un-pinning the second
    turn and the slot wrap in tests/test_gpu_take.py."""
    from tests import take_cases as T
    ns = [1, T.SLOT_SEGMENTS, T.SLOT_SEGMENTS + 1]
    assert [int(g) for g in take(['slots %d' % n for n in ns])] == [T.count_slots(n) for n in ns] == [T.SLOTS, T.SLOTS, 1]
    assert T.CHUNK == CHUNK and chunks(take, (70 * T.CHUNK,), chunk=T.CHUNK)[-1] == 70 > T.SLOTS
    with open(os.path.join(ROOT, 'cluster_tools_amd', 'csrc', 'ctg_plan.h')) as f:
        assert 'constexpr int64_t TAKE_CHUNK = %d;' % T.CHUNK in f.read()
    with open(os.path.join(ROOT, 'cluster_tools_amd', 'csrc', 'ctg_take.hip')) as f:
        src = f.read()
    assert 'std::min<int64_t>((n + 255) / 256, %d)' % (T.MAX_TURN // 256) in src
    assert 'k_take_max, dim3((unsigned)blocks), dim3(256)' in src
    assert T.max_turns(T.MAX_TURN) == 1 and T.max_turns(T.MAX_TURN + 1) == 2


def test_build_and_lookup_against_a_dict(take):
    rng = np.random.default_rng(2024)
    keys = np.unique(rng.integers(0, 1 << 63, size=100000, dtype=np.uint64))
    table = {int(k): int(v) for k, v in zip(keys, rng.integers(0, 1 << 63, size=keys.size, dtype=np.uint64))}
    queries = [int(k) for k in keys[::3]] + [int(k) + 1 for k in keys[::5]] + [0, TOP]
    cap, got = build_and_look(take, table, queries)
    assert cap == 1 << 18
    assert got == [table.get(q) for q in queries]


def test_keys_that_collide_under_a_masked_identity_hash(take):
    table = {i << 20: i + 7 for i in range(1000)}
    queries = list(table) + [(i << 20) + 1 for i in range(50)] + [1000 << 20]
    _, got = build_and_look(take, table, queries)
    assert got == [table.get(q) for q in queries]


def test_extreme_keys(take):
    table = {0: 5, 1 << 63: 6, TOP: 7}
    _, got = build_and_look(take, table, [0, 1 << 63, TOP, 1, TOP - 1, (1 << 63) - 1])
    assert got == [5, 6, 7, None, None, None]
    # the free-slot value is a key only where it was inserted
    _, got = build_and_look(take, {0: 5}, [TOP, 0])
    assert got == [None, 5]
    _, got = build_and_look(take, {}, [0, TOP, 3])
    assert got == [None, None, None]


def test_duplicates_are_detected(take):
    out = take(['build 5 3 1 4 1 3 2 9 9 3 7', 'look 3 3 4 9',
                'build 3 %d 1 %d 2 5 5' % (TOP, TOP), 'look 2 %d 5' % TOP])
    assert out[0].split()[0] == '2' and out[1] == '1 1 9'          # the first value stays
    assert out[2].split()[0] == '1' and out[3] == '1 5'


def chunks(take, lens, chunk=CHUNK, seg=True):
    begin = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    q = 'chunks %d %d %d %d ' % (chunk, begin[-1], int(seg), len(lens)) + ' '.join(str(b) for b in begin)
    return [int(t) for t in take([q])[0].split()]


def test_chunk_prefix(take):
    assert chunks(take, (5, 0, 130), chunk=64) == [0, 0, 1, 1, 4]
    assert chunks(take, (5, 0, 130)) == [0, 0, 1, 1, 2]
    assert chunks(take, (0,)) == [0, 0, 0]
    assert chunks(take, ()) == [0, 0]
    for n, c in ((CHUNK - 1, 1), (CHUNK, 1), (CHUNK + 1, 2)):
        assert chunks(take, (n,)) == [0, 0, c]
        assert [int(t) for t in take(['chunks %d %d 0 0' % (CHUNK, n)])[0].split()] == [0, 0, c]   # no segment list
    assert [int(t) for t in take(['chunks %d 0 0 0' % CHUNK])[0].split()] == [0, 0, 0]


def test_chunk_prefix_refuses_bad_segments(take):
    bad = ['chunks 64 10 1 2 0 5 9',        # does not end at n
           'chunks 64 10 1 2 1 5 10',       # does not start at 0
           'chunks 64 10 1 2 0 11 10',      # descends
           'chunks 64 10 1 0 0',            # no segment for 10 voxels
           'chunks 64 -1 0 0']
    assert [t.split()[0] for t in take(bad)] == ['1'] * len(bad)
    assert take(['chunks 1 %d 0 0' % (1 << 31)])[0].split()[0] == '2'      # 2^31 workgroups
    assert take(['chunks 1 %d 0 0' % ((1 << 31) - 1)])[0].split() == ['0', '0', str((1 << 31) - 1)]


# --------------------------------------------------------------------------- tools.take / takeDict before the GPU
def test_mirror_argument_rules():
    from cluster_tools_amd import tools
    vol = np.zeros((2, 3), dtype=np.uint64)
    with pytest.raises(ValueError, match='1-D'):
        tools.take(np.zeros((3, 2), dtype=np.uint64), vol)
    with pytest.raises(TypeError, match='integers'):
        tools.take(np.zeros(3, dtype=np.float32), vol)
    with pytest.raises(OverflowError):
        tools.take(np.array([1, -1], dtype=np.int64), vol)
    with pytest.raises(TypeError, match='integer labels'):
        tools.take(np.zeros(3, dtype=np.uint64), vol.astype(np.float64))
    with pytest.raises(ValueError, match='negative'):
        tools.take(np.zeros(3, dtype=np.uint64), np.array([-1], dtype=np.int64))
    with pytest.raises(TypeError, match='dict'):
        tools.takeDict(np.zeros(3, dtype=np.uint64), vol)
    with pytest.raises(TypeError, match='integer labels'):
        tools.takeDict({0: 0}, vol.astype(np.float32))
    with pytest.raises(OverflowError, match='uint32'):                 # the reference truncates here (write.py:180)
        tools.takeDict({0: 0, 1: 1 << 32}, vol.astype(np.uint32))
    with pytest.raises(OverflowError, match='uint8'):
        tools.takeDict({0: 256}, vol.astype(np.uint8))
    with pytest.raises(OverflowError):
        tools.takeDict({0: -1}, vol)
    assert tools.blocking is not None                                  # nifty.tools.blocking, next to them
