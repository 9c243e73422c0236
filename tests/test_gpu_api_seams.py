"""Seams of the face-scan entry points that the other suites do not reach:
the single-label fix with an owned box off the origin, long-range affinities
on labels >= 2^32 (the Bloom filter is built by the dense re-entry only),
profiled calls (the phase marks and their read-back) and the batched call
without node lists.  Exact against oracle.rag_oracle."""
import math

import numpy as np
import pytest

from cluster_tools_amd import rag
from cluster_tools_amd import synthetic as S
from oracle import rag_oracle as O

from test_gpu_blocks import _block_geometry
from test_gpu_parity import BIG, check_features

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('with_data', [False, True])
@pytest.mark.parametrize('dtype', [np.uint32, np.uint64])
def test_single_label_owned_box_off_origin(gpu, dtype, with_data):
    """One label everywhere: no record, and the only node is read from the
    owned box's first voxel (32-bit labels are widened on the host)."""
    lab = np.full((5, 6, 7), 42, dtype)
    data = np.zeros(lab.shape, np.float32) if with_data else None
    out = rag.rag_features(lab, data, own_begin=(1, 2, 3))
    assert out['edges'].shape == (0, 2)
    np.testing.assert_array_equal(out['nodes'], np.array([42], np.uint64))
    if with_data:
        assert out['features'].shape == (0, 10)


def test_long_range_affinities_labels_above_2_32(gpu):
    """The first entry meets labels >= 2^32 and skips the adjacency filter; the
    dense re-entry runs the graph pass and builds the Bloom filter."""
    lab, bnd = S.generate((18, 40, 44), cell=5, seed=15)
    big = lab * np.uint64(977) + BIG
    offs = S.LR_OFFSETS
    affs = S.affinities_from_boundary(bnd, offs)
    e_ref, f_ref = O.affinity_features(lab, affs, offs)
    out = rag.rag_features(big, affs, offsets=offs)
    np.testing.assert_array_equal(out['edges'], e_ref * np.uint64(977) + BIG)
    np.testing.assert_array_equal(out['nodes'], O.unique_labels(lab) * np.uint64(977) + BIG)
    check_features(out['features'], f_ref)


@pytest.fixture(scope='module')
def two_blocks():
    lab, bnd = S.generate((20, 40, 50), cell=5, seed=8)
    geo = _block_geometry(lab.shape, (10, 40, 50))
    assert len(geo) == 2
    return lab, bnd, geo


def _blocks(lab, bnd, geo):
    return rag.rag_blocks([lab[g['roi']] for g in geo], [g['own'] for g in geo], [g['graph'] for g in geo],
                          data=[bnd[g['roi']] for g in geo])


def _same(a, b, exact_sums):
    """Two runs of one call.  Edges, nodes, counts and every feature that comes
    from integers or single samples (min, quantiles, max, count) bit for bit.
    Mean and variance come from float sums whose order (and pivot, the entry's
    first sample) the scan's atomics decide, so they are bit-equal only where
    every sum is exact (exact_sums); else they get the bar of
    test_gpu_parity._same_result.  n_records / n_direct count flushes of the
    run and are no part of the tables."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k in ('n_records', 'n_direct'):
            continue
        if k == 'features' and not exact_sums:
            np.testing.assert_array_equal(a[k][:, 2:], b[k][:, 2:], err_msg=k)
            np.testing.assert_allclose(a[k][:, :2], b[k][:, :2], rtol=1e-12, atol=1e-15, err_msg=k)
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize('exact_sums', [True, False])
def test_profiled_calls_equal_unprofiled(gpu, two_blocks, exact_sums):
    """A profiled call (phase marks, their read-back, the table calls'
    epilogue) returns what the unprofiled call returns, and its phase times are
    finite, non-negative, the total no shorter than the scan.

    exact_sums: a constant boundary map, on which every sum is exact and the
    whole result is reproducible: profiled == unprofiled bit for bit.  On the
    noisy map two unprofiled runs already differ in the last bit of some means
    and variances (measured: 178 of 17950 feature values, 1.1e-16 at most), so
    there those two columns are compared within 1e-12 relative and the rest
    bit for bit."""
    lab, bnd, geo = two_blocks
    if exact_sums:
        bnd = np.full(bnd.shape, 0.5, np.float32)
    coarse = lab // np.uint64(5)

    def run():
        res, times = [], []
        for call in (lambda: [rag.rag_features(lab, bnd)], lambda: _blocks(lab, bnd, geo),
                     lambda: [rag.label_overlaps(lab, coarse)]):
            res.append(call())
            times.append(rag.last_timings())
        return res, times

    plain, _ = run()
    rag.set_profiling(True)
    try:
        prof, times = run()
    finally:
        rag.set_profiling(False)
    for p, q in zip(plain, prof):
        assert len(p) == len(q)
        for a, b in zip(p, q):
            _same(a, b, exact_sums)
    for t in times:
        assert all(math.isfinite(v) and v >= 0.0 for v in t.values()), t
        assert t['total'] >= t['scan'], t
    # against the oracle, so that "equal" is not "equally wrong"
    e_ref, f_ref = O.boundary_features(lab, bnd)
    np.testing.assert_array_equal(prof[0][0]['edges'], e_ref)
    check_features(prof[0][0]['features'], f_ref)
    pairs, counts = np.unique(np.stack([lab.ravel(), coarse.ravel()], 1), axis=0, return_counts=True)
    np.testing.assert_array_equal(prof[2][0]['pairs'], pairs)
    np.testing.assert_array_equal(prof[2][0]['counts'], counts.astype(np.uint64))


def test_blocks_without_node_lists(gpu, two_blocks):
    """nodes=False (CTG_NO_NODES): the edge tables of the call with nodes, every
    node offset zero, no node."""
    lab, bnd, geo = two_blocks
    ref = _blocks(lab, bnd, geo)
    arena = np.concatenate([lab[g['roi']].ravel() for g in geo])
    darena = np.concatenate([bnd[g['roi']].ravel() for g in geo])
    blocks, lo = [], 0
    for g in geo:
        shape = lab[g['roi']].shape
        blocks.append(dict(label_offset=lo, data_offset=lo, shape=shape, own=g['own'], graph=g['graph']))
        lo += int(np.prod(shape))
    res = rag.rag_blocks_arena(arena, blocks, darena, nodes=False)
    assert len(res) == 2
    for g, r, q in zip(geo, res, ref):
        _same(dict(edges=r['edges'], features=r['features']), dict(edges=q['edges'], features=q['features']), False)
        np.testing.assert_array_equal(r['edges'], O.rag_edges(lab[g['outer']]))
        assert r['nodes'].shape == (0,) and q['nodes'].shape[0] > 0
