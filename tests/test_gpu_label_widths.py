"""The record sort across label widths, with default switches: which of its
paths a call takes depends on nb = bits of the largest label, the slot bits
ib, the record count and the label range, and every call here says which one
it took (rag.last_sort()), checked against tests/sort_plan.py's restatement
of plan_record_sort / plan_group_sort on the reported ib and n.

a. The ladder: one small volume with its labels mapped into widths of 20 to
   32 bits, at the top of the range, around its middle and spread all over it.
b. Few record-heavy labels near 2^30: the smallest case in which the group
   sort's bucket index (pk >> shift) passes 2^32 -- bucket keys rebuilt in 32
   bits came out with u - 2^30 and no error.

Edges, nodes and counts are exact against oracle.rag_oracle or an analytic
expectation; features use check_features of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from cluster_tools_amd import rag
from cluster_tools_amd import synthetic as S
from oracle import rag_oracle as O

import sort_plan as SP
from test_gpu_blocks import _block_geometry, _expected_boundary
from test_gpu_parity import RTOL, check_features

pytestmark = pytest.mark.gpu

SHAPE = (24, 72, 100)
WIDTHS = (20, 24, 26, 28, 29, 30, 31, 32)
LAYOUTS = ('top', 'straddle', 'spread')
ODD = 2654435761            # an odd constant: x -> x * ODD mod 2^nb is a bijection of [0, 2^nb)
TOP_MODES = ('graph', 'affinity_nn', 'uint32')


def _mapping(lab, nb, layout):
    """The label map of a ladder case, as a function on uint64 arrays."""
    lo, hi = int(lab.min()), int(lab.max())
    if layout == 'top':             # the largest label is 2^nb - 1
        off = (1 << nb) - 1 - hi
        return lambda x: x + np.uint64(off)
    if layout == 'straddle':        # half of the labels on either side of 2^(nb - 1)
        off = (1 << (nb - 1)) - (lo + hi + 1) // 2
        assert off >= 0
        return lambda x: x + np.uint64(off)
    assert hi < (1 << 20)           # x * ODD stays below 2^64
    return lambda x: (x * np.uint64(ODD)) & np.uint64((1 << nb) - 1)


def _relabel(edges, rows, m):
    """The oracle's table of the base labels as the table of the mapped ones:
    a bijection renames the endpoints, the samples of a face stay its own."""
    a, b = m(edges[:, 0]), m(edges[:, 1])
    u, v = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((v, u))
    return np.stack([u, v], 1)[order], (rows[order] if rows is not None else None)


def _check_reported(info, nb, ub, min_label, max_label, spread=True):
    """rag.last_sort() of a default-switch call against the prediction from
    its own ib and n.  Returns the outcome's name."""
    assert (info['nb'], info['ub']) == (nb, ub), info
    assert info['n'] > 0 and 16 <= info['ib'] <= 32, info
    exp = SP.predict(info, min_label, max_label, spread=spread)
    assert info['group_tried'] == exp['group_tried'], (info, exp)
    g = exp['plan']
    if g is None:                                   # not offered to the group sort
        assert (info['path'], info['packed'], info['group_done'], info['group_decline'], info['group_shift'],
                info['largest_bucket']) == (exp['path'], exp['packed'], 0, 'none', -1, -1), (info, exp)
        return info['path']
    if g['why'] != 'none':                          # declined by the geometry, before any launch
        assert (info['path'], info['packed'], info['group_done'], info['group_decline'], info['largest_bucket']) == \
            (exp['path'], exp['packed'], 0, g['why'], -1), (info, exp)
        assert info['group_shift'] == g.get('shift', -1), (info, exp)
        return 'declined_' + g['why']
    assert (info['group_shift'], info['group_buckets']) == (g['shift'], g['nbk']), (info, exp)
    assert 0 < info['largest_bucket'] <= info['n'], info
    if info['largest_bucket'] > SP.GS_CAP:          # the device's counts decide
        fallback = SP.plan_record_sort(info['n'], info['ub'], info['nb'], info['ib'], spread)
        assert (info['path'], info['packed'], info['group_done'], info['group_decline']) == \
            (fallback[2], int(fallback[0]), 0, 'bucket_cap'), info
        return 'declined_bucket_cap'
    assert (info['path'], info['packed'], info['group_done'], info['group_decline']) == ('group', 0, 1, 'none'), info
    return 'group'


@pytest.fixture(scope='module')
def base():
    """The ladder's volume and its oracle tables, computed once."""
    lab, bnd = S.generate(SHAPE, cell=5)
    affs = S.affinities_from_boundary(bnd, S.NN_OFFSETS)
    e, f = O.boundary_features(lab, bnd)
    ea, fa = O.affinity_features(lab, affs, S.NN_OFFSETS)
    np.testing.assert_array_equal(e, O.rag_edges(lab))
    np.testing.assert_array_equal(ea, e)
    return dict(lab=lab, bnd=bnd, affs=affs, edges=e, feats=f, aff_feats=fa, nodes=O.unique_labels(lab))


@pytest.fixture(scope='module')
def ladder(gpu, base):
    """Every ladder call, made once with no environment switch, each with
    what rag.last_sort() said right after it.  The library's cached buffers
    are released first: the record buffer then starts from its smallest size
    (18 slot bits for this volume), whatever ran before, so the widths split
    between the paths the same way in every run."""
    rag.trim_cache()
    runs = {}
    for nb in WIDTHS:
        for layout in LAYOUTS:
            lab = _mapping(base['lab'], nb, layout)(base['lab'])
            for mode in ('boundary',) + (TOP_MODES if layout == 'top' else ()):
                if mode == 'graph':
                    out = rag.rag_features(lab)
                elif mode == 'affinity_nn':
                    out = rag.rag_features(lab, base['affs'], offsets=S.NN_OFFSETS)
                elif mode == 'uint32':
                    out = rag.rag_features(lab.astype(np.uint32), base['bnd'])
                else:
                    out = rag.rag_features(lab, base['bnd'])
                runs[(nb, layout, mode)] = (out, rag.last_sort())
    return runs


@pytest.mark.parametrize('layout', LAYOUTS)
def test_relabelled_reference_is_the_oracles(base, layout):
    """The reference of a ladder case is the base volume's oracle table
    renamed; at 31 bits it is what the oracle gives on the mapped labels."""
    m = _mapping(base['lab'], 31, layout)
    e_ref, f_ref = _relabel(base['edges'], base['feats'], m)
    e, f = O.boundary_features(m(base['lab']), base['bnd'])
    np.testing.assert_array_equal(e_ref, e)
    np.testing.assert_array_equal(f_ref[:, [2, 8, 9]], f[:, [2, 8, 9]])
    np.testing.assert_allclose(f_ref, f, rtol=1e-12, atol=1e-15)


CASES = [(nb, layout, 'boundary') for nb in WIDTHS for layout in LAYOUTS] + \
        [(nb, 'top', mode) for nb in WIDTHS for mode in TOP_MODES]


@pytest.mark.parametrize('nb,layout,mode', CASES)
def test_ladder(base, ladder, nb, layout, mode):
    out, info = ladder[(nb, layout, mode)]
    m = _mapping(base['lab'], nb, layout)
    rows = {'graph': None, 'affinity_nn': base['aff_feats']}.get(mode, base['feats'])
    e_ref, f_ref = _relabel(base['edges'], rows, m)
    assert int(e_ref[:, 1].max()).bit_length() == nb
    _check_reported(info, nb, nb, int(e_ref[:, 0].min()), int(e_ref[:, 1].max()))
    np.testing.assert_array_equal(out['edges'], e_ref)
    np.testing.assert_array_equal(out['nodes'], np.sort(m(base['nodes'])))
    if f_ref is not None:
        check_features(out['features'], f_ref)


def test_ladder_visits_every_outcome(base, ladder):
    """The ladder as a whole took the packed-key bucket sort, the group sort,
    the group sort's refusal of more than 32 key bits below its group bits
    (labels spread over 24 bits; spread over 30 and 31 bits the few buckets
    are so wide that a bucket-local key and the slot pass 64 bits, which is
    checked first) and its refusal of 64 key bits (32-bit labels)."""
    seen = {}
    for (nb, layout, mode), (out, info) in ladder.items():
        key = (info['path'], info['group_tried'], info['group_done'], info['group_decline'])
        seen.setdefault(key, []).append((nb, layout, mode))
    assert ('bucket_keys', 0, 0, 'none') in seen, seen.keys()
    assert ('group', 1, 1, 'none') in seen, seen.keys()
    assert (24, 'spread', 'boundary') in seen.get(('bucket_pairs', 1, 0, 'low_bits'), []), seen
    early = seen.get(('bucket_pairs', 1, 0, 'low_bits'), []) + seen.get(('bucket_pairs', 1, 0, 'item_bits'), [])
    assert (30, 'spread', 'boundary') in early and (31, 'spread', 'boundary') in early, seen
    wide = seen.get(('bucket_pairs', 1, 0, 'key_bits'), [])
    assert sorted(c for c in wide) == sorted(c for c in ladder if c[0] == 32), seen
    # labels at the top of 30 and 31 bits, the widths no test reached before, sort by the group sort
    assert all(ladder[(nb, 'top', 'boundary')][1]['group_done'] == 1 for nb in (29, 30, 31))


@pytest.mark.parametrize('nb', [18, 20, 28, 31])
def test_ladder_blocks(gpu, base, nb):
    """Two blocks of the ladder's volume through rag.rag_blocks: keys tagged
    with the block (32 bits of u, never spread), so they pack only where
    32 + nb + ib <= 63 and take onesweep either way; exact against the
    per-block oracle."""
    lab = _mapping(base['lab'], nb, 'top')(base['lab'])
    geo = _block_geometry(SHAPE, (12, 72, 100))
    assert len(geo) == 2
    res = rag.rag_blocks([lab[g['roi']] for g in geo], [g['own'] for g in geo], [g['graph'] for g in geo],
                         data=[base['bnd'][g['roi']] for g in geo])
    info = rag.last_sort()
    got = _check_reported(info, nb, 32, 0, int(lab.max()), spread=False)
    assert got == ('onesweep_keys' if 32 + nb + info['ib'] <= 63 else 'onesweep_pairs_wide')
    for g, r in zip(geo, res):
        np.testing.assert_array_equal(r['nodes'], np.unique(lab[g['inner']]))
        eb, f = _expected_boundary(lab, base['bnd'], g)
        np.testing.assert_array_equal(r['edges'], eb)
        check_features(r['features'], f)


# ---------------------------------------------------------------------------
# b. few record-heavy labels near 2^30
# ---------------------------------------------------------------------------
def _planes(first, n_planes, ny, nx):
    """Plane k of n_planes x ny x nx labelled first + k (uint32) and a
    boundary map with the value (k + 1) / 32 on plane k."""
    lab = np.empty((n_planes, ny, nx), np.uint32)
    lab[:] = (first + np.arange(n_planes, dtype=np.uint32))[:, None, None]
    bnd = np.empty((n_planes, ny, nx), np.float32)
    bnd[:] = ((np.arange(n_planes, dtype=np.float32) + 1) / 32)[:, None, None]
    return lab, bnd


def _check_planes(out, first, n_planes, face, with_map):
    """Analytic: edges (first + k, first + k + 1) with both voxels of every
    face, the nodes are the planes' labels; the map's two values an edge."""
    ids = first + np.arange(n_planes, dtype=np.uint64)
    np.testing.assert_array_equal(out['edges'], np.stack([ids[:-1], ids[1:]], 1))
    np.testing.assert_array_equal(out['nodes'], ids)
    if not with_map:
        return
    f = out['features']
    c = (np.arange(n_planes, dtype=np.float64) + 1) / 32
    np.testing.assert_array_equal(f[:, 9], np.full(n_planes - 1, 2.0 * face))
    np.testing.assert_array_equal(f[:, 2], c[:-1])
    np.testing.assert_array_equal(f[:, 8], c[1:])
    np.testing.assert_array_equal(f[:, 0], (c[:-1] + c[1:]) / 2)
    np.testing.assert_allclose(f[:, 1], np.full(n_planes - 1, (1.0 / 64) ** 2), rtol=RTOL, atol=0.0)


def _group_preconditions(info, first, n_planes, nb):
    """Before any result is looked at: the group sort took the records, no
    bucket above GS_CAP, and the reported shift is the plan's.  Returns the
    largest bucket index before the base is taken off, max_pk >> shift."""
    got = _check_reported(info, nb, nb, first, first + n_planes - 1)
    assert got == 'group' and info['largest_bucket'] <= SP.GS_CAP, info
    return SP.key_range(nb, nb, first, first + n_planes - 1)[1] >> info['group_shift']


@pytest.mark.parametrize('first,past', [((1 << 30), True), ((1 << 30) - 8, True), ((1 << 29), False)],
                         ids=['from_2_30', 'across_2_30', 'from_2_29'])
def test_record_heavy_labels_narrow_tiles(gpu, monkeypatch, first, past):
    """16 planes of 1792 x 2048 (uint32 labels, 235 MB), plane k labelled
    first + k, scanned with narrow tiles (footprint 64 x 8): every one of the
    15 faces yields 1792 * 2048 / 512 = 7168 records, 107 520 in all -- more
    than 6144 a label of the range, so the group sort's shift drops to 29
    (nb = 31) and pk >> shift passes 2^32: from 2^30 the bucket base itself
    needs 33 bits, across 2^30 the base fits 32 bits and base + bucket does
    not.  From 2^29 (nb = 30: the nodes come from the bitmap over [min_u,
    max_v]) the same records reach shift 28 and stay below 2^32.  Graph-only
    calls scan with wide tiles (1792 records a face: shift 30, below 2^32);
    they are held to the same analytic result and to the predicted path."""
    n_planes, ny, nx = 16, 1792, 2048
    nb = int(first + n_planes - 1).bit_length()
    lab, bnd = _planes(first, n_planes, ny, nx)
    monkeypatch.setenv('CTG_NARROW_ROWS', '1')
    out = rag.rag_features(lab, bnd)
    info = rag.last_sort()
    assert info['n'] == (n_planes - 1) * (ny // 8) * (nx // 64), info
    top = _group_preconditions(info, first, n_planes, nb)
    assert info['group_shift'] == (29 if nb == 31 else 28), info
    assert (top >= (1 << 32)) == past, (top, info)
    _check_planes(out, first, n_planes, ny * nx, True)
    out = rag.rag_features(lab)
    info = rag.last_sort()
    assert _check_reported(info, nb, nb, first, first + n_planes - 1) == 'group', info
    _check_planes(out, first, n_planes, ny * nx, False)


def test_record_heavy_labels_graph_only(gpu):
    """Graph only (wide tiles, footprint 64 x 32) past 2^32: 5 planes of 4096
    x 4096 labelled 2^30 + k give 8192 records a face, 32 768 in all -- above
    6144 a label and a full bucket (GS_CAP) each at shift 29."""
    first, n_planes, side = 1 << 30, 5, 4096
    lab = np.empty((n_planes, side, side), np.uint32)
    lab[:] = (first + np.arange(n_planes, dtype=np.uint32))[:, None, None]
    out = rag.rag_features(lab)
    info = rag.last_sort()
    assert info['n'] == (n_planes - 1) * (side // 32) * (side // 64), info
    top = _group_preconditions(info, first, n_planes, 31)
    assert info['group_shift'] == 29 and info['largest_bucket'] == SP.GS_CAP and top >= (1 << 32), (top, info)
    _check_planes(out, first, n_planes, side * side, False)
