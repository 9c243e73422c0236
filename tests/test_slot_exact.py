"""The face scan bins a sample of the default [0, 1] range with an integer
clamp and one ordered compare (sample_slot<true>, csrc/ctg_stats.h) instead of
a ladder of four f64 compare / select pairs.  tools/slot_exact.hip -- host
code only, no GPU, no library -- walks all 2^32 float bit patterns and counts
where the new rule differs from the ladder (kept in that program) and from
hist_slot, the rule every other path and the oracle use: nowhere."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'no hipcc'
    exe = str(tmp_path_factory.mktemp('slot') / 'slot_exact')
    subprocess.run([hipcc, '-O2', '-std=c++17', '--offload-host-only', os.path.join(ROOT, 'tools', 'slot_exact.hip'),
                    '-o', exe, '-lpthread'], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return dict((k, int(v)) for k, v in (l.split() for l in r.stdout.splitlines()))


def test_every_float_was_checked(report):
    assert report['checked'] == 1 << 32


def test_same_slot_as_the_ladder(report):
    assert report['mismatch_ladder'] == 0


def test_same_slot_as_hist_slot(report):
    assert report['mismatch_hist_slot'] == 0
