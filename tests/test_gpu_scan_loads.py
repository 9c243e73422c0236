"""The face scan's plane loads and flush polls (csrc/ctg_scan.hip) against the
oracle: edges, nodes and counts exact, min / max exact, quantiles to QTOL (the
bars of tests/test_gpu_parity.py, with min / max held exactly).

The face kernels address a plane row as (uniform base of the wave's rows of
the plane) + (uniform row offset) + (the lane's 32-bit byte offset), so the
cases are the smallest at which one of the three can go wrong:

* 3 x 37 x 131: two full x tiles + 3 columns (the last tile's lanes and its
  x-halo lane are clamped), one full y tile + 5 rows (rows past Y clamp to the
  last row, and six waves of the second tile lie wholly past Y); 1 x 1 x 65 (one
  row, every wave but the first past Y, one voxel in the second x tile) and
  2 x 33 x 64 (no x-halo column at all, one row in the second y tile);
* uint32 and uint64 labels with float32 and uint8 data: the element sizes
  scale the row and lane offsets differently for the two arrays;
* graph only, boundary map, three nearest-neighbour channels (the channel
  stride is part of the base);
* device tensors that start one element into their allocation (labels 8-byte
  aligned, data 4-byte or 1-byte aligned only), and a second batched block at
  odd arena offsets (the block's offsets are part of the base);
* a slab with a halo plane (own_begin = (1, 0, 0));
* waves that never fold beside waves that ask for a flush at nearly every
  batch, and the per-wave sample budget's requests.
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

SHAPES = {'3x37x131': ((3, 37, 131), 3, 81), '1x1x65': ((1, 1, 65), 2, 82), '2x33x64': ((2, 33, 64), 3, 83)}
LABEL_TYPES = ['uint32', 'uint64']
DATA_TYPES = ['float32', 'uint8']


def check_exact(f_gpu, f_ref):
    """check_features, and min / max (columns 2 and 8) bit for bit."""
    check_features(f_gpu, f_ref)
    np.testing.assert_array_equal(f_gpu[:, 2], f_ref[:, 2])
    np.testing.assert_array_equal(f_gpu[:, 8], f_ref[:, 8])


def _data(bnd, dtype):
    return bnd if dtype == 'float32' else np.round(bnd * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def volume(name):
    shape, cell, seed = SHAPES[name]
    lab, bnd = S.generate(shape, cell=cell, seed=seed)
    lab.setflags(write=False)
    bnd.setflags(write=False)
    return lab, bnd


@functools.lru_cache(maxsize=None)
def boundary_ref(name, dtype):
    lab, bnd = volume(name)
    return O.boundary_features(lab, _data(bnd, dtype))


@functools.lru_cache(maxsize=None)
def nn_ref(name, dtype):
    lab, bnd = volume(name)
    affs = _data(S.affinities_from_boundary(bnd, S.NN_OFFSETS), dtype)
    return affs, O.affinity_features(lab, affs, S.NN_OFFSETS)


@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_graph_only(gpu, name, ltype):
    lab, _ = volume(name)
    out = rag.rag_features(lab.astype(ltype))
    np.testing.assert_array_equal(out['edges'], O.rag_edges(lab))
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))


@pytest.mark.parametrize('dtype', DATA_TYPES)
@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_boundary(gpu, name, ltype, dtype):
    lab, bnd = volume(name)
    e_ref, f_ref = boundary_ref(name, dtype)
    out = rag.rag_features(lab.astype(ltype), _data(bnd, dtype))
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_exact(out['features'], f_ref)


@pytest.mark.parametrize('dtype', DATA_TYPES)
@pytest.mark.parametrize('ltype', LABEL_TYPES)
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_nearest_neighbour_channels(gpu, name, ltype, dtype):
    lab, _ = volume(name)
    affs, (e_ref, f_ref) = nn_ref(name, dtype)
    out = rag.rag_features(lab.astype(ltype), affs, offsets=S.NN_OFFSETS)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_exact(out['features'], f_ref)


def _offset_view(arr, torch):
    """arr on the device, starting one element into its allocation."""
    host = torch.from_numpy(arr.copy()).reshape(-1)
    buf = torch.empty(arr.size + 1, dtype=host.dtype, device='cuda')
    buf[1:] = host.cuda()
    v = buf[1:].view(arr.shape)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


@pytest.mark.parametrize('dtype', DATA_TYPES)
@pytest.mark.parametrize('kind', ['boundary', 'nn'])
def test_bases_not_16_byte_aligned(gpu, kind, dtype):
    """Labels 8 bytes, data one element (4 bytes or 1 byte) into a 16-byte
    aligned allocation."""
    import torch
    name = '3x37x131'
    lab, bnd = volume(name)
    lab_t = _offset_view(lab.view(np.int64), torch)
    assert lab_t.data_ptr() % 16 == 8
    if kind == 'boundary':
        data, (e_ref, f_ref), offsets = _data(bnd, dtype), boundary_ref(name, dtype), None
    else:
        (data, (e_ref, f_ref)), offsets = nn_ref(name, dtype), S.NN_OFFSETS
    data_t = _offset_view(data, torch)
    assert data_t.data_ptr() % 16 == data.dtype.itemsize
    r = rag.rag_features_handle(lab_t, data_t, offsets=offsets)
    e, n, f = r.edges(), r.nodes(), r.features()
    r.free()
    np.testing.assert_array_equal(e, e_ref)
    np.testing.assert_array_equal(n, O.unique_labels(lab))
    check_exact(f, f_ref)


@pytest.mark.parametrize('ltype', LABEL_TYPES)
def test_second_block_at_odd_arena_offsets(gpu, ltype):
    """Two z blocks in one batched launch; a pad element in front of the second
    block's labels and three in front of its data make its offsets odd."""
    lab, bnd = volume('3x37x131')
    shape = lab.shape
    geo = _block_geometry(shape, (2, shape[1], shape[2]))
    assert len(geo) == 2
    parts_l, parts_d, blocks, lo, do = [], [], [], 0, 0
    for i, g in enumerate(geo):
        if i == 1:
            parts_l.append(np.zeros(1, lab.dtype))
            parts_d.append(np.zeros(3, bnd.dtype))
            lo += 1
            do += 3
        sub = lab[g['roi']]
        blocks.append(dict(label_offset=lo, data_offset=do, shape=sub.shape, own=g['own'], graph=g['graph']))
        parts_l.append(sub.ravel())
        parts_d.append(bnd[g['roi']].ravel())
        lo += sub.size
        do += sub.size
    assert blocks[1]['label_offset'] % 2 == 1 and blocks[1]['data_offset'] % 2 == 1
    la = np.concatenate(parts_l).astype(ltype)
    res = rag.rag_blocks_arena(la, blocks, np.concatenate(parts_d))
    graph = rag.rag_blocks_arena(la, blocks)
    for g, r, gr in zip(geo, res, graph):
        eb, f = _expected_boundary(lab, bnd, g)
        np.testing.assert_array_equal(r['nodes'], np.unique(lab[g['inner']]))
        np.testing.assert_array_equal(r['edges'], eb)
        check_exact(r['features'], f)
        np.testing.assert_array_equal(gr['edges'], eb)


@pytest.mark.parametrize('dtype', DATA_TYPES)
def test_slab_with_halo_plane(gpu, dtype):
    lab, bnd = S.generate((5, 37, 131), cell=3, seed=84)
    data = _data(bnd, dtype)
    e_ref, f_ref = O.boundary_features(lab, data, own_begin=(1, 0, 0))
    out = rag.rag_features(lab, data, own_begin=(1, 0, 0))
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_exact(out['features'], f_ref)
    g = rag.rag_features(lab, own_begin=(1, 0, 0))
    np.testing.assert_array_equal(g['edges'], O.rag_edges(lab, own_begin=(1, 0, 0)))


@functools.lru_cache(maxsize=None)
def unequal_waves():
    """20 x 40 x 130: rows y < 20 hold one label (their waves never fold and
    poll only at plane ends), rows y >= 20 random cells of 1-2 voxels (their
    waves take the table past its soft limit at nearly every batch).  The
    second y tile has 8 rows: two waves work, six wait in the exit loop."""
    shape = (20, 40, 130)
    rng = np.random.default_rng(85)
    lab = np.ones(shape, np.uint64)
    small = rng.integers(2, 200000, size=(20, 20, 65), dtype=np.uint64)
    lab[:, 20:, :] = np.repeat(small, 2, axis=2)[:, :, :130]
    lone = rng.random((20, 20, 130)) < 0.5   # cells of one voxel among the pairs
    lab[:, 20:, :][lone] = rng.integers(200000, 400000, size=int(lone.sum()), dtype=np.uint64)
    bnd = rng.random(shape, dtype=np.float32)
    return lab, bnd


@pytest.mark.parametrize('order', ['as_generated', 'reversed'])
def test_flushes_under_unequal_waves(gpu, order):
    lab, bnd = unequal_waves()
    if order == 'reversed':
        lab = (lab.max() - lab + np.uint64(1)).astype(np.uint64)
    e_ref, f_ref = O.boundary_features(lab, bnd)
    out = rag.rag_features(lab, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab))
    check_exact(out['features'], f_ref)
    assert out['n_records'] > e_ref.shape[0]   # the table was flushed on the way


def test_sample_budget_requests(gpu, monkeypatch):
    """Labels alternate in x: every x face is the edge (1, 2), so a wave's
    sample budget, not the table's fill, asks for the flushes."""
    monkeypatch.setenv('CTG_TILE_Z', '8')
    shape = (8, 32, 128)
    x = np.arange(shape[2])
    lab = np.broadcast_to((x % 2 + 1).astype(np.uint64), shape).copy()
    bnd = np.broadcast_to(np.where(x % 2, 0.7, 0.3).astype(np.float32), shape).copy()
    e_ref, f_ref = O.boundary_features(lab, bnd)
    out = rag.rag_features(lab, bnd)
    np.testing.assert_array_equal(out['edges'], e_ref)
    check_exact(out['features'], f_ref)
    assert out['features'][0, 9] == 2 * 8 * 32 * 127
