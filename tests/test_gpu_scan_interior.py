"""The face scan's two plane loops (csrc/ctg_scan.hip) against the oracle and
against each other.  A wave whose columns, rows and planes, and the neighbour
above each, all lie in the owned box (scan_wave_interior, csrc/ctg_plan.h)
walks its planes without ownership masks; every other wave, and every wave with
CTG_SCAN_INTERIOR=0, takes the general loop.  Each case runs both ways: both
results meet the bars of tests/test_gpu_scan_loads.py against the oracle
(edges, nodes and counts exact, min / max bit for bit, quantiles to QTOL, mean
and variance to the parity tolerance), and against each other edges, nodes,
counts, min, max and the quantile columns are identical.  ctg_last_scan must
report the expected number of interior waves with the switch on and none with
it off.

All cases use two-plane tiles (CTG_TILE_Z=2), the smallest volumes at which
the choice of loop can go wrong:

* mixed: 5 x 37 x 131 -- three x tiles (the last has 3 columns), two y tiles
  (the last has 5 rows: wave 0 of it is interior, wave 1 holds the array's last
  row, the others lie past Y, so waves of one workgroup take different loops),
  three z layers (the last has one plane);
* exact: 4 x 64 x 128 -- exact multiples of the tile: the last tiles are full
  yet not interior (a loop chosen from "the tile is full" reads past the array);
* onepast: 5 x 33 x 65 -- one voxel, one row and one plane beyond the first
  tile: exactly the neighbours its last lane, wave and plane need;
* slab: 5 x 37 x 131 with own_begin = (1, 0, 0) -- the layer that holds the
  halo plane 0 takes the general loop, and faces of plane 0 carry no samples;
* narrow: 5 x 37 x 131 with CTG_NARROW_ROWS=1 -- the one-row kernel of boundary
  maps (graphs and affinities have no narrow kernel and scan as `mixed`).

uint32 and uint64 labels, float32 and uint8 data, graph only, boundary map and
the three nearest-neighbour channels.
"""
import functools

import numpy as np
import pytest

from cluster_tools_amd import rag
from cluster_tools_amd import synthetic as S
from oracle import rag_oracle as O

from test_gpu_scan_loads import check_exact

pytestmark = pytest.mark.gpu

# name -> (shape, cell, seed, own_begin, narrow, interior waves of the wide launch, waves of it)
# interior = (x tiles with x0 + 64 < X) * (waves with yw + 4 < Y) * (layers with z1 < Z, from own_begin[0])
CASES = {
    'mixed': ((5, 37, 131), 3, 91, None, False, 2 * 9 * 2, 3 * 2 * 8 * 3),
    'exact': ((4, 64, 128), 3, 92, None, False, 1 * 15 * 1, 2 * 2 * 8 * 2),
    'onepast': ((5, 33, 65), 3, 93, None, False, 1 * 8 * 2, 2 * 2 * 8 * 3),
    'slab': ((5, 37, 131), 3, 94, (1, 0, 0), False, 2 * 9 * 1, 3 * 2 * 8 * 3),
    'narrow': ((5, 37, 131), 3, 95, None, True, 2 * 9 * 2, 3 * 2 * 8 * 3),
}
# the narrow launch of the `narrow` boundary map: 8-row tiles of one-row waves
NARROW_INTERIOR, NARROW_WAVES = 2 * 36 * 2, 3 * 5 * 8 * 3
LABEL_TYPES = ['uint32', 'uint64']
DATA_TYPES = ['float32', 'uint8']
EXACT_COLS = [2, 3, 4, 5, 6, 7, 8, 9]   # min, the five quantiles, max, count


def _data(bnd, dtype):
    return bnd if dtype == 'float32' else np.round(bnd * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def volume(name):
    shape, cell, seed = CASES[name][:3]
    lab, bnd = S.generate(shape, cell=cell, seed=seed)
    lab.setflags(write=False)
    bnd.setflags(write=False)
    return lab, bnd


def _own(name):
    return CASES[name][3] or (0, 0, 0)


@functools.lru_cache(maxsize=None)
def graph_ref(name):
    return O.rag_edges(volume(name)[0], own_begin=_own(name))


@functools.lru_cache(maxsize=None)
def boundary_ref(name, dtype):
    lab, bnd = volume(name)
    return O.boundary_features(lab, _data(bnd, dtype), own_begin=_own(name))


@functools.lru_cache(maxsize=None)
def nn_ref(name, dtype):
    lab, bnd = volume(name)
    affs = _data(S.affinities_from_boundary(bnd, S.NN_OFFSETS), dtype)
    affs.setflags(write=False)
    return affs, O.affinity_features(lab, affs, S.NN_OFFSETS, own_begin=_own(name))


def _both(monkeypatch, name, boundary_map, call):
    """call() with the interior loop on and off -> the two results, after the
    checks of what ctg_last_scan reports for each."""
    _, _, _, _, narrow, interior, waves = CASES[name]
    monkeypatch.setenv('CTG_TILE_Z', '2')
    if narrow:
        monkeypatch.setenv('CTG_NARROW_ROWS', '1')
    want = dict(waves=waves, interior_waves=interior, narrow_waves=0, narrow_interior_waves=0)
    if narrow and boundary_map:
        want = dict(waves=0, interior_waves=0, narrow_waves=NARROW_WAVES, narrow_interior_waves=NARROW_INTERIOR)
    assert want['interior_waves'] + want['narrow_interior_waves'] > 0
    outs = []
    for switch in (None, '0'):
        if switch is not None:
            monkeypatch.setenv('CTG_SCAN_INTERIOR', switch)
        outs.append(call())
        got = rag.last_scan()
        if switch == '0':
            want = dict(want, interior_waves=0, narrow_interior_waves=0)
        assert got == want, (switch, got, want)
    return outs


def _same_tables(on, off, features):
    np.testing.assert_array_equal(on['edges'], off['edges'])
    np.testing.assert_array_equal(on['nodes'], off['nodes'])
    if features:
        np.testing.assert_array_equal(on['features'][:, EXACT_COLS], off['features'][:, EXACT_COLS])


@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_graph_only(gpu, monkeypatch, name, ltype):
    lab, _ = volume(name)
    labels = lab.astype(ltype)
    on, off = _both(monkeypatch, name, False, lambda: rag.rag_features(labels, own_begin=CASES[name][3]))
    for out in (on, off):
        np.testing.assert_array_equal(out['edges'], graph_ref(name))
        if CASES[name][3] is None:
            np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    _same_tables(on, off, False)


@pytest.mark.parametrize('dtype', DATA_TYPES)
@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_boundary(gpu, monkeypatch, name, ltype, dtype):
    lab, bnd = volume(name)
    labels, data = lab.astype(ltype), _data(bnd, dtype)
    e_ref, f_ref = boundary_ref(name, dtype)
    on, off = _both(monkeypatch, name, True, lambda: rag.rag_features(labels, data, own_begin=CASES[name][3]))
    for out in (on, off):
        np.testing.assert_array_equal(out['edges'], e_ref)
        if CASES[name][3] is None:
            np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
        check_exact(out['features'], f_ref)
    _same_tables(on, off, True)


@pytest.mark.parametrize('dtype', DATA_TYPES)
@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(CASES))
def test_nearest_neighbour_channels(gpu, monkeypatch, name, ltype, dtype):
    lab, _ = volume(name)
    labels = lab.astype(ltype)
    affs, (e_ref, f_ref) = nn_ref(name, dtype)
    on, off = _both(monkeypatch, name, False,
                    lambda: rag.rag_features(labels, affs, offsets=S.NN_OFFSETS, own_begin=CASES[name][3]))
    for out in (on, off):
        np.testing.assert_array_equal(out['edges'], e_ref)
        if CASES[name][3] is None:
            np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
        check_exact(out['features'], f_ref)
    _same_tables(on, off, True)


def test_slab_plane_zero_carries_no_samples(gpu, monkeypatch):
    """own_begin = (1, 0, 0): an edge whose only faces lie in plane 0 (x and y
    faces there, both voxels in the halo plane) is no edge of the slab, and the
    counts of the others leave those faces out -- in both loops."""
    lab, bnd = volume('slab')
    e_all, f_all = O.boundary_features(lab, bnd)
    e_ref, f_ref = boundary_ref('slab', 'float32')
    assert f_ref[:, 9].sum() < f_all[:, 9].sum()
    on, off = _both(monkeypatch, 'slab', True, lambda: rag.rag_features(lab, bnd, own_begin=(1, 0, 0)))
    for out in (on, off):
        np.testing.assert_array_equal(out['features'][:, 9], f_ref[:, 9])
