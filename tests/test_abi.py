"""The C-ABI library loads and exports every symbol include/ctg.h declares
(CPU: no compute calls); the Python shim binds exactly those symbols; the
product path has no CPU fallback."""
import ctypes
import os
import re

import pytest

from cluster_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    with open(os.path.join(ROOT, 'include', 'ctg.h')) as fh:
        src = fh.read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(ctg_\w+)\s*\(', src)))


def header_defines():
    with open(os.path.join(ROOT, 'include', 'ctg.h')) as fh:
        return dict(re.findall(r'#define\s+(CTG_\w+)\s+(-?\d+)', fh.read()))


def test_header_parses():
    fns = header_functions()
    assert 'ctg_rag_features' in fns and 'ctg_free' in fns and len(fns) >= 20


def test_library_exports_every_header_symbol():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [f for f in header_functions() if not hasattr(lib, f)]
    assert not missing, missing


def test_shim_binds_exactly_the_header():
    assert sorted(_lib.PROTOTYPES) == header_functions()


def test_shim_constants_match_header():
    d = header_defines()
    for name, val in d.items():
        if hasattr(_lib, name):
            assert getattr(_lib, name) == int(val), name
    for name in ('CTG_KEEP_STATS', 'CTG_NO_ADJ_FILTER', 'CTG_MEM_DEVICE', 'CTG_DATA_U8',
                 'CTG_WIDE_RECORD_WORDS', 'CTG_MAX_CHANNELS'):
        assert getattr(_lib, name) == int(d[name]), name


def test_version_without_gpu():
    assert _lib.load().ctg_version() >= 1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'libctg.so'))
    with pytest.raises(_lib.CtgError):
        _lib.load()


def test_product_package_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'cluster_tools_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                with open(os.path.join(dirpath, f)) as fh:
                    src = fh.read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, re.M), f


@pytest.fixture(scope='module')
def qfuzz(tmp_path_factory):
    """tools/quantile_fuzz.hip built once for the tests that run it (a host
    build of the device statistics code)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    exe = str(tmp_path_factory.mktemp('qfuzz') / 'qfuzz')
    src = os.path.join(ROOT, 'tools', 'quantile_fuzz.hip')
    subprocess.run([hipcc, '-O2', '-std=c++17', '--offload-arch=gfx950', src, '-o', exe], check=True,
                   capture_output=True, timeout=300)
    return exe


def test_quantile_crossing_matches_keypoint_walk(qfuzz):
    """The reduction's quantiles (vigra_quantiles_cross: crossing search over the
    bins) are bit-identical to the keypoint walk restating vigra's
    computeStandardQuantiles, on 2 M random histograms incl. outliers, bin-edge
    minima/maxima and single-bin edges (host build of the same device code)."""
    import subprocess
    r = subprocess.run([qfuzz], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    assert ' 0 / ' in r.stdout or r.stdout.startswith('0 / ')


def test_host_statistics_match_python_oracle(qfuzz):
    """The link from the device statistics code to the Python oracle the GPU
    tests trust: 20 000 seeded sample sets (ranges [0,1], [-1,2],
    [-0.37,0.91] and u8 samples k/255; bin edges, their float neighbours,
    outliers on both sides, the (-1, 0) bin-space interval that truncates into
    bin 0) binned by ctg::hist_slot and finalised by vigra_quantiles_cross in
    a host build, against oracle.rag_oracle.histogram_slots and
    vigra_quantiles on the same float32 samples: slots and quantiles equal,
    bit for bit."""
    import subprocess
    import numpy as np
    from oracle import rag_oracle as O
    n_cases = 20000
    r = subprocess.run([qfuzz, '--dump', str(n_cases), '2024'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == n_cases
    u8 = np.arange(256, dtype=np.float32) / np.float32(255.0)      # oracle.as_samples' mapping
    bad_slots, bad_q, kinds, edge_hits, outliers = [], [], set(), 0, 0
    for i, line in enumerate(lines):
        t = line.split()
        kind, lo, hi, n = int(t[0]), float(t[1]), float(t[2]), int(t[3])
        vmin, vmax = float(t[4]), float(t[5])
        slots = np.array(t[6:48], dtype=np.int64)
        q = np.array(t[48:53], dtype=np.float64)
        x = np.array([int(w, 16) for w in t[53:]], dtype=np.uint32).view(np.float32)
        assert x.shape[0] == n and (lo, hi) == [(0.0, 1.0), (-1.0, 2.0), (-0.37, 0.91), (0.0, 1.0)][kind]
        assert vmin == x.min() and vmax == x.max()
        if kind == 3:
            assert np.isin(x, u8).all()
        kinds.add(kind)
        s_ref = O.histogram_slots(x, lo, hi)
        h_ref = np.bincount(s_ref, minlength=O.NBINS + 2)
        edge_hits += int((x == np.float32(hi)).sum())
        outliers += int(h_ref[0] + h_ref[-1])
        if not np.array_equal(h_ref, slots):
            bad_slots.append(i)
            continue
        q_ref = O.vigra_quantiles(h_ref, x.min(), x.max(), n, lo, hi)[1:6]
        if not np.array_equal(q_ref, q):
            bad_q.append((i, float(np.abs(q_ref - q).max())))
    assert kinds == {0, 1, 2, 3} and edge_hits > 100 and outliers > 1000
    assert not bad_slots, 'histogram slots differ in %d cases, first %s' % (len(bad_slots), bad_slots[:5])
    assert not bad_q, 'quantiles differ in %d cases, first %s' % (len(bad_q), bad_q[:5])


def test_diag_bounds_only_in_diag_builds():
    """ctg_diag_bounds answers only in CTG_DIAG builds; the product library
    compiles the bounds checks out and says so (no GPU call either way here)."""
    import ctypes
    if os.environ.get('CTG_LIB'):
        pytest.skip('a variant build is loaded')
    out = (ctypes.c_uint64 * 4)()
    assert _lib.load().ctg_diag_bounds(out) == -4
    assert b'CTG_DIAG' in _lib.load().ctg_last_error()
