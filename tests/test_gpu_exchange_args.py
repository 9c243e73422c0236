"""The error and edge paths of the multi-GPU exchange's host layer
(cluster_tools_amd/csrc/ctg_api_mgpu.hip) that no other test pins:

* the status and message of every refusal of ctg_mgpu_pack / ctg_mgpu_merge
  that is decided once the count matrix is read -- counts that do not cover
  the table, a missing buffer, a stale CTG_DEFER_STATS table, a shard passed as
  the local table, rows received by a table without statistics -- as the
  library reported them before its host layer was rewritten;
* a world-2 exchange in which a rank receives node ids and no rows (the node
  prefix of the receive table alone), and a world-32 exchange in which only
  the last source sends to rank 0, whose own range is empty: every shard
  against the numpy restatement (tests/dist_helpers.py).

Both volumes assert what they force from the restated splitter rule before
the library is called.  The volumes are a few thousand voxels; every case runs
in well under a second."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from cluster_tools_amd import _lib as L              # noqa: E402
from cluster_tools_amd import dist as cdist          # noqa: E402
from cluster_tools_amd import rag                    # noqa: E402
from oracle import rag_oracle as O                   # noqa: E402

from test_gpu_parity import check_features           # noqa: E402
from tests import exchange_cases as X                # noqa: E402
from tests.dist_helpers import OracleBackend, Part, S, SIGN, slab_nodes, split_counts, splitters  # noqa: E402
from tests.exchange_sim import simulate              # noqa: E402

ARG, HIP, STALE = -1, -2, -5
ROW = cdist.ROW_WORDS
SHAPE = (4, 8, 64)


def _volume():
    rng = np.random.default_rng(11)
    z, y, x = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing='ij')
    lab = (z * 100 + (y // 4) * 16 + x // 4 + 1).astype(np.uint64)
    return lab, (rng.integers(0, 257, SHAPE) / 256).astype(np.float32)


def _local(keep_stats=True, defer_stats=False):
    lab, data = _volume()
    return rag.rag_features_handle(lab, data, keep_stats=keep_stats, defer_stats=defer_stats)


def _counts(world, entries):
    c = np.zeros((world, world, 2), np.int64)
    for (s, d), v in entries.items():
        c[s, d] = v
    return c


def _pack(loc, counts, world, rank, send):
    return L.load().ctg_mgpu_pack(loc.handle, counts.ctypes.data_as(ctypes.c_void_p), world, rank,
                                  None if send is None else ctypes.c_void_p(send.data_ptr()), None)


def _merge(loc, counts, world, rank, recv):
    out = ctypes.c_void_p()
    rc = L.load().ctg_mgpu_merge(loc.handle, None if recv is None else ctypes.c_void_p(recv.data_ptr()),
                                 counts.ctypes.data_as(ctypes.c_void_p), world, rank, 0.0, 1.0, None, ctypes.byref(out))
    return rc, out


def _refused(rc, status, message, out=None):
    msg = L.load().ctg_last_error().decode()
    assert (rc, msg) == (status, message)
    assert out is None or not out.value, 'a refused merge left *out set'


def _words(n):
    return torch.zeros(n, dtype=torch.int64, device='cuda')


# ---------------------------------------------------------------- refusals
def test_merge_of_received_rows_needs_statistics(gpu):
    """One received row, but the local call kept no statistics: reported as
    HIP's invalid-argument error under the entry point's name."""
    loc = _local(keep_stats=False)
    try:
        c = _counts(2, {(0, 0): (loc.n_edges, loc.n_nodes), (1, 0): (1, 0)})
        rc, out = _merge(loc, c, 2, 0, _words(ROW))
        _refused(rc, HIP, 'ctg_mgpu_merge: invalid argument', out)
    finally:
        loc.free()


def test_merge_refuses_a_shard_as_local_table(gpu):
    loc = _local()
    c = _counts(1, {(0, 0): (loc.n_edges, loc.n_nodes)})
    rc, out = _merge(loc, c, 1, 0, None)
    shard = rag.Result(out, loc.device)
    try:
        assert rc == 0 and shard.n_edges == c[0, 0, 0] and shard.n_nodes == c[0, 0, 1]
        rc, out2 = _merge(shard, c, 1, 0, None)
        _refused(rc, ARG, 'ctg_mgpu_merge: the local table is itself a merge shard; pass the rank\'s local call', out2)
    finally:
        shard.free()
        loc.free()


def test_counts_must_cover_the_table(gpu):
    loc = _local()
    try:
        for entries in ({(0, 0): (loc.n_edges + 1, loc.n_nodes)}, {(0, 0): (loc.n_edges, loc.n_nodes - 1)},
                        {(0, 0): (loc.n_edges, loc.n_nodes), (0, 1): (1, 0)}):
            c = _counts(2, entries)
            _refused(_pack(loc, c, 2, 0, _words(ROW)), ARG, "ctg_mgpu_pack: counts do not cover this rank's table")
            rc, out = _merge(loc, c, 2, 0, _words(ROW))
            _refused(rc, ARG, "ctg_mgpu_merge: counts do not cover this rank's table", out)
        assert loc.n_edges > 0                                         # the refused merges left the table alone
    finally:
        loc.free()


def test_words_to_move_need_a_buffer(gpu):
    loc = _local()
    try:
        E, N = loc.n_edges, loc.n_nodes
        send = _counts(2, {(0, 0): (E - 1, N), (0, 1): (1, 0)})
        _refused(_pack(loc, send, 2, 0, None), ARG,
                 'ctg_mgpu_pack: rows to send need a CTG_KEEP_STATS table and a send buffer')
        nodes_only = _counts(2, {(0, 0): (E, N - 1), (0, 1): (0, 1)})
        _refused(_pack(loc, nodes_only, 2, 0, None), ARG,
                 'ctg_mgpu_pack: rows to send need a CTG_KEEP_STATS table and a send buffer')
        recv = _counts(2, {(0, 0): (E, N), (1, 0): (0, 1)})
        rc, out = _merge(loc, recv, 2, 0, None)
        _refused(rc, ARG, 'ctg_mgpu_merge: null receive buffer', out)
        # nothing to move: no buffer needed
        assert _pack(loc, _counts(2, {(0, 0): (E, N)}), 2, 0, None) == 0
    finally:
        loc.free()
    bare = _local(keep_stats=False)                                    # a send buffer, but no statistics to send
    try:
        c = _counts(2, {(0, 0): (bare.n_edges - 1, bare.n_nodes), (0, 1): (1, 0)})
        _refused(_pack(bare, c, 2, 0, _words(ROW)), ARG,
                 'ctg_mgpu_pack: rows to send need a CTG_KEEP_STATS table and a send buffer')
    finally:
        bare.free()


def test_stale_deferred_table(gpu):
    """A CTG_DEFER_STATS table after another call on the device overwrote its
    records: refused by pack and by merge where words move, accepted where
    none do."""
    loc = _local(defer_stats=True)
    _local().free()
    tail = ": the CTG_DEFER_STATS table's records were overwritten by a later call"
    try:
        E, N = loc.n_edges, loc.n_nodes
        _refused(_pack(loc, _counts(2, {(0, 0): (E - 1, N), (0, 1): (1, 0)}), 2, 0, _words(ROW)), STALE,
                 'ctg_mgpu_pack' + tail)
        rc, out = _merge(loc, _counts(2, {(0, 0): (E, N), (1, 0): (1, 0)}), 2, 0, _words(ROW))
        _refused(rc, STALE, 'ctg_mgpu_merge' + tail, out)
        assert _pack(loc, _counts(2, {(0, 0): (E, N)}), 2, 0, None) == 0
    finally:
        loc.free()


# ------------------------------------------------------------- edge exchanges
def _restated_counts(lab, world):
    """The count matrix the restated rules give for the z-slabs of lab
    (exchange_cases.plan, for a volume that is no named case)."""
    edges, nodes, meta = [], [], []
    for rd, own, end in X.slab_planes(lab.shape[0], world):
        e = O.rag_edges(lab[rd:end], own_begin=(own - rd, 0, 0))
        edges.append(e)
        nodes.append(slab_nodes(lab[rd:end], (own - rd, 0, 0)))
        m = np.zeros(S + 1, np.int64)
        if e.shape[0]:
            m[:S] = (e[(np.arange(S) * e.shape[0]) // S, 0] ^ SIGN).view(np.int64)
        m[S] = e.shape[0]
        meta.append(m)
    spl = splitters(np.stack(meta), world)
    return np.stack([split_counts(Part(e, None, None, None, n, False), spl, world) for e, n in zip(edges, nodes)])


def _exchange_against_restatement(lab, data, world, defer, want_counts):
    want = simulate(OracleBackend(), lab, data, world)
    lab_t = torch.from_numpy(lab.view(np.int64).copy()).cuda()
    trace = {}
    got = simulate(cdist.HipBackend(defer_stats=defer), lab_t, torch.from_numpy(data.copy()).cuda(), world,
                   fresh=defer, trace=trace)
    try:
        np.testing.assert_array_equal(trace['counts_all'], want_counts)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.edges(), w.edges())
            np.testing.assert_array_equal(g.nodes(), w.nodes())
            check_features(g.features(), w.features())
        np.testing.assert_array_equal(np.concatenate([g.nodes() for g in got]), O.unique_labels(lab))
        np.testing.assert_array_equal(np.concatenate([g.edges() for g in got]), O.rag_edges(lab))
    finally:
        for g in got:
            g.free()


@pytest.mark.parametrize('defer', [False, True])
def test_world2_rank_receives_nodes_without_rows(gpu, defer):
    """Two slabs of two planes; the upper slab and the plane below it are one
    label, the smallest: the upper rank has no edge and one node, which lies
    below the splitter -- the lower rank receives that id and no row."""
    rng = np.random.default_rng(5)
    z, y, x = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing='ij')
    lab = np.where(z == 0, (y // 2) * 16 + x // 4 + 10, 1).astype(np.uint64)
    data = (rng.integers(0, 257, SHAPE) / 256).astype(np.float32)
    counts = _restated_counts(lab, 2)
    assert tuple(counts[1, 0]) == (0, 1) and counts[1].sum() == 1       # one node to rank 0, nothing else
    assert counts[0, 0, 0] > 0 and counts[0, 1, 0] > 0                  # rank 0 keeps rows and sends rows
    _exchange_against_restatement(lab, data, 2, defer, counts)


@pytest.mark.parametrize('defer', [False, True])
def test_world32_only_last_source_sends_to_rank0(gpu, defer):
    """32 planes of 8 x 64, one per rank.  Plane 31 holds the smallest labels
    and most of them, plane 0 the largest: rank 0's splitter range lies inside
    plane 31's labels, so rank 0 keeps nothing of its own table and receives
    from rank 31 alone -- one receive segment, the last source's."""
    shape = (32, 8, 64)
    rng = np.random.default_rng(6)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    coarse = (y // 4) * 8 + x // 8                                       # 16 labels a plane
    fine = y * 32 + x // 2                                               # 256 labels
    lab = np.where(z == 31, fine + 1, np.where(z == 0, 100000 + coarse, 1000 * z + coarse)).astype(np.uint64)
    data = (rng.integers(0, 257, shape) / 256).astype(np.float32)
    counts = _restated_counts(lab, 32)
    assert not counts[1:31, 0].any() and counts[31, 0, 0] > 0 and counts[31, 0, 1] > 0
    assert tuple(counts[0, 0]) == (0, 0) and counts[0, :, 0].sum() > 0   # rank 0's own range is empty
    _exchange_against_restatement(lab, data, 32, defer, counts)
