"""bench.py on the GPU at a small size: a plain run times the steps it is
asked for and nothing else, and --dump-outputs writes what the timed call
returned (against the oracle on the same synthetic volume, north_star bars of
test_gpu_parity), as a fixed sample when the tables exceed the dump budget.
"""
import json
import os
import sys

import numpy as np
import pytest

from cluster_tools_amd import rag
from oracle import rag_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, CELL = 48, 6
ARGV = ['--gpus', '1', '--config', '1', '--size', str(SIZE), '--cell', str(CELL), '--warmup', '1']


def run_bench(monkeypatch, capsys, argv):
    """bench.main() in this process (the suite's device is already open);
    returns the parsed result line."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + argv)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope='module')
def reference(gpu):
    """Oracle tables of the bench's input volume (same generator arguments)."""
    lab, bnd = rag.synth_volume((SIZE, SIZE, SIZE), cell=CELL, seed=0, z_offset=0, global_shape=(SIZE, SIZE, SIZE))
    labels = lab.cpu().numpy().view(np.uint64)
    edges, feats = O.boundary_features(labels, bnd.cpu().numpy())
    return edges, O.unique_labels(labels), feats


def check_features(f_gpu, f_ref):
    assert f_gpu.shape == f_ref.shape
    np.testing.assert_array_equal(f_gpu[:, 9], f_ref[:, 9])
    for c in (0, 1, 2, 8):
        np.testing.assert_allclose(f_gpu[:, c], f_ref[:, c], rtol=1e-5, atol=0.0)
    np.testing.assert_array_less(np.abs(f_gpu[:, 3:8] - f_ref[:, 3:8]), 1.0 / 40 + 1e-12)


def load(d):
    return {n: np.load(os.path.join(d, n + '.npy')) for n in ('edges', 'nodes', 'features', 'counts')}


def test_plain_run_line_and_dump(gpu, reference, tmp_path, monkeypatch, capsys):
    edges, nodes, feats = reference
    d = str(tmp_path / 'out')
    line = run_bench(monkeypatch, capsys, ARGV + ['--steps', '3', '--dump-outputs', d])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['ms_per_step'] > 0
    assert line['unit'] == 'Gvoxels/s' and line['higher_is_better'] is True
    assert line['value'] == pytest.approx(SIZE ** 3 / (line['ms_per_step'] * 1e-3) / 1e9, rel=1e-3)
    assert line['cpu_baseline'] is None            # behind --full
    assert line['config']['edges'] == edges.shape[0]
    got = load(d)
    assert all(a.dtype == np.float64 for a in got.values())
    assert sorted(os.listdir(d)) == ['counts.npy', 'edges.npy', 'features.npy', 'nodes.npy']
    np.testing.assert_array_equal(got['counts'], [edges.shape[0], nodes.shape[0]])
    np.testing.assert_array_equal(got['edges'], edges.astype(np.float64))
    np.testing.assert_array_equal(got['nodes'], nodes.astype(np.float64))
    check_features(got['features'], feats)
    assert line['outputs']['arrays']['features'] == [edges.shape[0], 10]


def test_dump_sample_of_large_tables(gpu, reference, tmp_path, monkeypatch, capsys):
    """Tables above the budget: the same sorted rows of edges and features in
    every run, the full lengths in counts."""
    edges, nodes, feats = reference
    import bench
    monkeypatch.setattr(bench, 'DUMP_MAX_ROWS', 101)
    monkeypatch.setattr(bench, 'DUMP_MAX_NODES', 37)
    rows, nrows = bench.sample_rows(edges.shape[0], 101), bench.sample_rows(nodes.shape[0], 37)
    assert rows is not None and nrows is not None
    for k in range(2):
        d = str(tmp_path / ('out%d' % k))
        run_bench(monkeypatch, capsys, ARGV + ['--steps', '1', '--dump-outputs', d])
        got = load(d)
        np.testing.assert_array_equal(got['counts'], [edges.shape[0], nodes.shape[0]])
        np.testing.assert_array_equal(got['edges'], edges[rows].astype(np.float64))
        np.testing.assert_array_equal(got['nodes'], nodes[nrows].astype(np.float64))
        check_features(got['features'], feats[rows])
