"""The face scan's push sites and fold (csrc/ctg_scan.hip) on the smallest
volumes at which they can go wrong, against the oracle with the bars of
tests/test_gpu_parity.py (edges, nodes and counts exact, quantiles to QTOL,
mean / variance / min / max to rtol 1e-5).

The sites stage a face as they hold it -- (label, neighbour label, the two
samples) -- and the fold makes the key's (smaller, larger) order and, for
batched blocks, ors the block tag into it.  So the cases are:

* 9 x 37 x 70 and 5 x 33 x 129: X no multiple of 64 (lane 63 takes its
  partner from the x-halo, the last x tile is clamped), Y no multiple of 32, a
  tail plane;
* every volume as generated and with its labels mapped to max - l: the
  lower-coordinate voxel of a face holds the smaller label in one, the larger
  in the other, on every axis, so the fold's ordering is exercised both ways;
* a 4 x 32 x 64 volume of 1-voxel cells: more than 128 faces in the x and y
  sites of one wave's plane (a stage cannot take them at once) and more keys
  than the LDS table holds (direct records);
* the same volumes through the graph-only scan, uint8 data, nearest-neighbour
  and long-range affinities, the narrow-tile kernel, two batched blocks (the
  block tag) and labels >= 2^32 (the dense relabelling).
"""
import functools

import numpy as np
import pytest

from cluster_tools_amd import rag
from cluster_tools_amd import synthetic as S
from oracle import rag_oracle as O

from test_gpu_parity import check_features
from test_gpu_blocks import _block_geometry, _expected_boundary

pytestmark = pytest.mark.gpu

VOLUMES = {'9x37x70': ((9, 37, 70), 4, 51), '5x33x129': ((5, 33, 129), 3, 52)}
ORDERS = ['as_generated', 'reversed']


@functools.lru_cache(maxsize=None)
def volume(name, order):
    shape, cell, seed = VOLUMES[name]
    lab, bnd = S.generate(shape, cell=cell, seed=seed)
    if order == 'reversed':
        lab = (lab.max() - lab).astype(np.uint64)
    lab.setflags(write=False)
    bnd.setflags(write=False)
    return lab, bnd


@functools.lru_cache(maxsize=None)
def boundary_ref(name, order, dtype):
    lab, bnd = volume(name, order)
    return O.boundary_features(lab, _data(bnd, dtype))


@functools.lru_cache(maxsize=None)
def checkerboard():
    shape = (4, 32, 64)
    lab = (np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(1)).reshape(shape)
    bnd = np.random.default_rng(53).random(shape, dtype=np.float32)
    return lab, bnd, O.boundary_features(lab, bnd)


def _data(bnd, dtype):
    return bnd if dtype == 'float32' else np.round(bnd * 255).astype(np.uint8)


def test_both_label_orders_on_every_axis():
    """What the two label orders are for: on each axis, faces whose
    lower-coordinate voxel holds the smaller label and faces where it holds the
    larger one both occur, in each order (so each is the majority in one)."""
    for name in VOLUMES:
        up = {}
        for order in ORDERS:
            lab, _ = volume(name, order)
            for ax in range(3):
                a = np.moveaxis(lab, ax, 0)
                lo, hi = a[:-1], a[1:]
                assert (lo < hi).any() and (lo > hi).any()
                up[order, ax] = int((lo < hi).sum()) - int((lo > hi).sum())
        for ax in range(3):
            assert up['as_generated', ax] == -up['reversed', ax]


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_boundary(gpu, name, order, dtype):
    lab, bnd = volume(name, order)
    e_ref, f_ref = boundary_ref(name, order, dtype)
    out = rag.rag_features(lab, _data(bnd, dtype))
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_features(out['features'], f_ref)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_boundary_narrow_tile(gpu, monkeypatch, name, order):
    """The 1-row kernel: one staged entry per lane, a 64-entry stage."""
    lab, bnd = volume(name, order)
    e_ref, f_ref = boundary_ref(name, order, 'float32')
    monkeypatch.setenv('CTG_NARROW_ROWS', '1')
    out = rag.rag_features(lab, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_features(out['features'], f_ref)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_graph_only(gpu, name, order):
    lab, _ = volume(name, order)
    out = rag.rag_features(lab)
    np.testing.assert_array_equal(out['edges'], O.rag_edges(lab))
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))


@pytest.mark.parametrize('offsets', [S.NN_OFFSETS, S.LR_OFFSETS], ids=['nn', 'lr'])
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_affinities(gpu, name, order, offsets):
    lab, bnd = volume(name, order)
    affs = S.affinities_from_boundary(bnd, offsets)
    e_ref, f_ref = O.affinity_features(lab, affs, offsets)
    out = rag.rag_features(lab, affs, offsets=offsets)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_features(out['features'], f_ref)


@pytest.mark.parametrize('narrow', ['0', '1'])
def test_checkerboard_of_one_voxel_cells(gpu, monkeypatch, narrow):
    """Every face of the volume is a boundary face with a key of its own: a
    wave's x and y sites of one plane hold ~500 faces, four stages' worth, and
    the table cannot hold a tile's keys."""
    lab, bnd, (e_ref, f_ref) = checkerboard()
    assert e_ref.shape[0] == 3 * lab.size - (32 * 64 + 4 * 64 + 4 * 32)
    monkeypatch.setenv('CTG_NARROW_ROWS', narrow)
    out = rag.rag_features(lab, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_features(out['features'], f_ref)
    g = rag.rag_features(lab)
    np.testing.assert_array_equal(g['edges'], e_ref)


def test_checkerboard_reversed_and_affinities(gpu):
    lab, bnd, _ = checkerboard()
    rev = (lab.max() - lab).astype(np.uint64)
    e_ref, f_ref = O.boundary_features(rev, bnd)
    out = rag.rag_features(rev, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_features(out['features'], f_ref)
    affs = S.affinities_from_boundary(bnd, S.NN_OFFSETS)
    e_ref, f_ref = O.affinity_features(lab, affs, S.NN_OFFSETS)
    out = rag.rag_features(lab, affs, offsets=S.NN_OFFSETS)
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_features(out['features'], f_ref)


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('name', sorted(VOLUMES))
def test_two_batched_blocks(gpu, name, order):
    """Two z blocks in one ctg_rag_blocks launch: the second block's keys carry
    a non-zero tag, or-ed into the smaller label by the fold."""
    lab, bnd = volume(name, order)
    shape = lab.shape
    geo = _block_geometry(shape, ((shape[0] + 1) // 2, shape[1], shape[2]))
    assert len(geo) == 2
    blocks, lo = [], 0
    for g in geo:
        shp = lab[g['roi']].shape
        blocks.append(dict(label_offset=lo, data_offset=lo, shape=shp, own=g['own'], graph=g['graph']))
        lo += int(np.prod(shp))
    la = np.concatenate([lab[g['roi']].ravel() for g in geo])
    da = np.concatenate([bnd[g['roi']].ravel() for g in geo])
    res = rag.rag_blocks_arena(la, blocks, da)
    graph = rag.rag_blocks_arena(la, blocks)
    for g, r, gr in zip(geo, res, graph):
        eb, f = _expected_boundary(lab, bnd, g)
        np.testing.assert_array_equal(r['nodes'], np.unique(lab[g['inner']]))
        np.testing.assert_array_equal(r['edges'], eb)
        check_features(r['features'], f)
        np.testing.assert_array_equal(gr['edges'], eb)
        np.testing.assert_array_equal(gr['nodes'], np.unique(lab[g['inner']]))


@pytest.mark.parametrize('order', ORDERS)
def test_labels_above_2_32(gpu, order):
    """One label >= 2^32 sends the call through the dense relabelling."""
    lab, bnd = volume('9x37x70', order)
    big = lab.copy()
    top = big.max()
    big[big == top] = np.uint64(1) << np.uint64(40)
    e_ref, f_ref = O.boundary_features(big, bnd)
    out = rag.rag_features(big, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(big))
    check_features(out['features'], f_ref)
