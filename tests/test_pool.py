"""The caching device allocator (csrc/ctg_pool.h) and the buffers that own
themselves (csrc/ctg_buffers.h) are plain C++ over an allocate / free back
end; tools/pool_check.cpp runs them on the CPU against a fake back end that
keeps a ledger and refuses on demand -- built with the host compiler and
-fsanitize=address,undefined -- so the failure paths that must never be
provoked on a GPU are pinned here (no GPU, no library).  The wait_* cases pin
StreamWait: with a fake stream_wait that logs into the same list as dev_free,
every return path of a scope waits for the stream before a block of the scope
goes back to the pool, unless the guard was disarmed or never armed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('pool') / 'pool_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', os.path.join(ROOT, 'tools', 'pool_check.cpp'), '-o', exe],
                   check=True, capture_output=True, timeout=300)
    # every case ends with its pool purged and checks that no block is left at
    # the back end or was freed twice; ASan's leak check covers the rest at exit
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _round_up(b):
    r = 256
    while r < b:
        r = r * 2 if r < (1 << 20) else r + (r >> 2)
    return r


def test_size_classes(report):
    got = {int(b): int(r) for _, b, r in (l.split() for l in report if l.startswith('class '))}
    Mi = 1 << 20
    # 256 B doubling to 1 MiB, then x1.25
    assert [got[b] for b in (0, 1, 255, 256, 257, 511, 512, 513)] == [256, 256, 256, 256, 512, 512, 512, 1024]
    assert [got[b] for b in (Mi - 1, Mi, Mi + 1, 1310720, 1310721, 1638400, 1638401)] == \
        [Mi, Mi, 1310720, 1310720, 1638400, 1638400, 2048000]
    assert len(got) == 18 and all(r == _round_up(b) for b, r in got.items())
    assert got[1 << 36] >= 1 << 36 and got[(1 << 32) + 1] < ((1 << 32) + 1) * 5 // 4


def test_stream_cases_restates_the_size_classes(report):
    """tests/stream_cases.py sizes the block that two calls on two streams
    share (tests/test_gpu_streams.py) by its own pool_round_up and reuse rule:
    the same classes as the library's, and the reuse bound of `reuse_bound`."""
    import stream_cases as SC
    got = {int(b): int(r) for _, b, r in (l.split() for l in report if l.startswith('class '))}
    assert len(got) == 18 and all(SC.pool_round_up(b) == r for b, r in got.items())
    assert SC.same_block_class(1000, 512) and SC.same_block_class(1000, 1024)   # up to twice the request's class
    assert not SC.same_block_class(2048, 512) and not SC.same_block_class(512, 1000)
    # the case of the test: V uint16 distances and V / 4 uint64 values, V = 5 * 33 * 70
    V = 5 * 33 * 70
    assert SC.pool_round_up(V * 2) == SC.pool_round_up((V // 4) * 8) == 32768


CASES = ['reuse_bound', 'purge_and_retry', 'purge_and_retry_refused', 'freed_to_allocating_device',
         'purge_with_refused_free', 'dev_buf', 'wait_before_frees', 'wait_on_early_return', 'wait_disarmed',
         'wait_without_buffers', 'wait_armed_later', 'grow_buf', 'sort_scratch_growth'] + \
        ['sort_scratch_refused_%d' % k for k in range(9)]


@pytest.mark.parametrize('case', CASES)
def test_case_held(report, case):
    assert 'ok ' + case in report


def test_no_case_unlisted(report):
    assert [l[3:] for l in report if l.startswith('ok ')] == CASES
