"""The multi-GPU exchange kernels (ctg_mgpu_sample / split / pack / merge,
cluster_tools_amd/csrc/ctg_mgpu.hip) on the adversarial label layouts of
tests/exchange_cases.py, every rank simulated on the one device
(tests/exchange_sim.py), at world sizes up to CTG_MGPU_MAX_WORLD = 32:

* end to end: the shards concatenate to the whole-volume oracle (edges and
  nodes bit for bit, features at check_features' bars) and to the single call
  (1e-9 / 1e-12), with written and with deferred statistics rows;
* step by step (world <= 8): the gathered samples, the count matrix, every
  send buffer and every shard against the numpy restatement of the same step
  (tests/dist_helpers.py) on the same slabs;
* ignore_label, uint8 maps, a histogram range of (-1, 2) with both outlier
  slots filled, and long-range offset sets, through the exchange;
* ctg_mgpu_split of every rank against the restated splitter rule.

Every case asserts what it forces (exchange_cases.check_case) before the
library is called.  What each case is for: the SIGN xor of the samples
(columns_high, random_perm, one_edge), the tie rule of k_mgpu_order (columns:
one key from W - 1 remote sources), empty ranges / ranks / segments and equal
splitters (hub, reversed, mostly_uniform, one_label, one_edge), the by-value
segment tables at world 32, and the ADJ-bit decisions across ranks
(lr_adjacency, and columns with long-range offsets).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from cluster_tools_amd import dist as cdist          # noqa: E402
from cluster_tools_amd import rag                    # noqa: E402
from cluster_tools_amd import synthetic              # noqa: E402
from oracle import rag_oracle as O                   # noqa: E402

from test_gpu_parity import check_features           # noqa: E402
from test_gpu_stats_exact import check_stats         # noqa: E402
from tests import exchange_cases as X                # noqa: E402
from tests.dist_helpers import ADJ, ROW, WIDE, OracleBackend, Part, decode_stats, split_counts, splitters  # noqa: E402
from tests.exchange_sim import simulate              # noqa: E402

# the largest deviations seen in this process, in units of their bars (noted
# before the assertion): shard features against the single call (rtol 1e-9,
# atol 1e-12), and the decoded mean (rtol 1e-12) / variance (rtol 1e-5) of the
# send rows against the restatement's
WORST = {'single_call': 0.0, 'send_mean': 0.0, 'send_var': 0.0}

END_TO_END = [(n, w) for n in X.BOUNDARY_CASES for w in X.WORLDS] + [('lr_adjacency', X.LR_WORLD)]
STEPS = [(n, w) for n in X.BOUNDARY_CASES for w in X.WORLDS if w <= 8]
SIX_OFFSETS = synthetic.LR_OFFSETS[:6]


def _note(key, dev, bar):
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(dev == 0, 0.0, dev / bar)
    if q.size:
        WORST[key] = max(WORST[key], float(np.nanmax(q)))


@functools.lru_cache(maxsize=None)
def _device_case(name, kind='f32', variant=None, n_channels=None):
    """(labels, data) of a case as numpy arrays and as CUDA tensors."""
    lab = _variant_labels(name, variant)
    data = X.case_data(name, kind, n_channels)
    lab_t = torch.from_numpy(lab.view(np.int64).copy()).cuda()
    return lab, data, lab_t, torch.from_numpy(data.copy()).cuda()


def _variant_labels(name, variant):
    lab = X.case(name).labels
    if variant == 'zero':     # the hub (or, without one, the label of the first voxel) becomes the ignore label
        lab = np.where(lab == lab[0, 0, 0], np.uint64(0), lab)
    return lab


@functools.lru_cache(maxsize=None)
def _references(name, kind='f32', variant=None, hist=(0.0, 1.0), offsets=None):
    """(oracle edges, oracle features, unique labels, the single call's
    result) of a case -- computed once, before any exchange of the test that
    asks first, and shared (read-only)."""
    offs = X.case(name).offsets if offsets is None else [list(o) for o in offsets]
    lab, data, _, _ = _device_case(name, kind, variant, None if offs is None else len(offs))
    ignore = variant == 'zero'
    if offs is None:
        e_ref, f_ref = O.boundary_features(lab, data, ignore_label=ignore, lo=hist[0], hi=hist[1])
    else:
        e_ref, f_ref = O.affinity_features(lab, data, offs, ignore_label=ignore, lo=hist[0], hi=hist[1])
    one = rag.rag_features(lab, data, offsets=offs, ignore_label=ignore, hist_range=hist)
    return e_ref, f_ref, O.unique_labels(lab), one


def _exchange(name, world, defer, kind='f32', variant=None, hist=(0.0, 1.0), offsets=None, trace=None):
    """One simulated exchange through the HIP backend: the concatenated
    (edges, features, nodes) and every shard's edge table.  Every handle is
    freed, also on failure (simulate frees the local tables and, on a failure,
    its shards)."""
    offs = X.case(name).offsets if offsets is None else [list(o) for o in offsets]
    _, _, lab_t, data_t = _device_case(name, kind, variant, None if offs is None else len(offs))
    shards = simulate(cdist.HipBackend(defer_stats=defer), lab_t, data_t, world, offsets=offs, hist_range=hist,
                      fresh=defer, ignore_label=variant == 'zero', trace=trace)
    try:
        per = [x.edges() for x in shards]
        return (np.concatenate(per), np.concatenate([x.features() for x in shards]),
                np.concatenate([x.nodes() for x in shards]), per)
    finally:
        for x in shards:
            x.free()


def _check_whole(got, refs, lo=0.0, hi=1.0):
    e, f, n, _ = got
    e_ref, f_ref, n_ref, one = refs
    np.testing.assert_array_equal(e, e_ref)
    np.testing.assert_array_equal(n, n_ref)
    check_features(f, f_ref, lo, hi)
    np.testing.assert_array_equal(e, one['edges'])
    np.testing.assert_array_equal(n, one['nodes'])
    _note('single_call', np.abs(f - one['features']), 1e-12 + 1e-9 * np.abs(one['features']))
    np.testing.assert_allclose(f, one['features'], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name,world', END_TO_END)
def test_exchange_case_end_to_end(gpu, name, world, defer):
    """Every case at every world size it lists, statistics rows written
    (CTG_KEEP_STATS) and deferred (CTG_DEFER_STATS, every rank's local call
    re-run before its pack and merge): the concatenated shards against the
    whole-volume oracle and against the single call."""
    X.check_case(name, world)
    refs = _references(name)
    got = _exchange(name, world, defer)
    _check_whole(got, refs)


def test_lr_adjacency_decisions(gpu):
    """The two ADJ decisions that need more than one rank, asserted to occur:
    (A, B) -- and (A2, B2), mirrored -- is a face in one rank's planes only and
    a -2 pairing in another's: its row is in the output with both samples, and
    a row of it travels with the ADJ bit set and another without; (C, D),
    paired by two ranks and adjacent nowhere, travels and is dropped."""
    name = 'lr_adjacency'
    X.check_case(name, X.LR_WORLD)
    refs = _references(name)
    trace = {}
    e, f, n, _ = _exchange(name, X.LR_WORLD, False, trace=trace)
    _check_whole((e, f, n, None), refs)
    rows = {tuple(int(t) for t in k): i for i, k in enumerate(e)}
    for a, b in (('A', 'B'), ('A2', 'B2')):
        assert f[rows[(X.LR[a], X.LR[b])], 9] == 2
    assert (X.LR['C'], X.LR['D']) not in rows
    # what travelled: (key, ADJ) of every sent row, and what every rank held
    sent = set()
    for r, (keys, _, rec, _) in _segments(trace, X.LR_WORLD):
        sent |= {(int(k[0]), int(k[1]), bool(w & ADJ)) for k, w in zip(keys, rec[:, 42])}
    held = [{tuple(int(t) for t in k) for k in tab[0]} for tab in trace['tables']]
    cd = (X.LR['C'], X.LR['D'])
    assert cd in held[1] and cd in held[2] and cd + (False,) in sent and cd + (True,) not in sent
    proved_elsewhere = 0
    for a, b in (('A', 'B'), ('A2', 'B2')):
        k = (X.LR[a], X.LR[b])
        assert k in held[0] and k in held[3]
        proved_elsewhere += k + (True,) in sent     # the owner learns the adjacency from a received row
    assert proved_elsewhere >= 1


def _segments(trace, world):
    """(rank, (keys (n,2) u64, sums (n,2) f64, records (n,48) u32, node ids))
    of every destination segment of every send buffer, in buffer order."""
    counts = trace['counts_all']
    for r in range(world):
        buf = trace['sends'][r]
        off = 0
        for d in range(world):
            if d == r:
                continue
            nr, nn = int(counts[r, d, 0]), int(counts[r, d, 1])
            if buf is None:
                assert nr == 0 and nn == 0
                continue
            rows = buf[off:off + nr * ROW].reshape(nr, ROW)
            yield r, (np.ascontiguousarray(rows[:, :2]).view(np.uint64),
                      np.ascontiguousarray(rows[:, 2:4]).view(np.float64),
                      np.ascontiguousarray(rows[:, 4:]).view(np.uint32).reshape(nr, WIDE),
                      buf[off + nr * ROW:off + nr * ROW + nn].view(np.uint64))
            off += nr * ROW + nn
        assert buf is None or off == buf.shape[0]


# ---------------------------------------------------------------- step by step
@functools.lru_cache(maxsize=None)
def _restated(name, world):
    """The numpy restatement's trace and shard edge tables of a case."""
    c = X.case(name)
    trace = {}
    shards = simulate(OracleBackend(), c.labels, X.case_data(name), world, trace=trace)
    return trace, [s.edges() for s in shards]


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name,world', STEPS)
def test_exchange_case_steps_match_restatement(gpu, name, world, defer):
    """What travels between the four steps, HIP against numpy on the same
    slabs: the samples and the count matrix as integers; in every send buffer
    the keys and node ids bit for bit and the statistics words decoded at
    check_stats' bars (the two pivots differ, the decoded moments do not);
    every shard's edge table, so its first and last key."""
    X.check_case(name, world)
    want, want_shards = _restated(name, world)
    got = {}
    _, _, _, per = _exchange(name, world, defer, trace=got)
    np.testing.assert_array_equal(got['meta_all'], want['meta_all'])
    np.testing.assert_array_equal(got['counts_all'], want['counts_all'])
    for r in range(world):
        np.testing.assert_array_equal(got['tables'][r][0], want['tables'][r][0])
        np.testing.assert_array_equal(got['tables'][r][1], want['tables'][r][1])
        assert (got['sends'][r] is None) == (want['sends'][r] is None)
    for (r, g), (_, w) in zip(_segments(got, world), _segments(want, world)):
        np.testing.assert_array_equal(g[0], w[0])
        np.testing.assert_array_equal(g[3], w[3])
        np.testing.assert_array_equal(g[2][:, 42] & ADJ, w[2][:, 42] & ADJ)
        st = decode_stats(w[1], w[2])
        st['var'] = st['m2'] / np.maximum(st['count'], 1)
        d = decode_stats(g[1], g[2])
        _note('send_mean', np.abs(d['mean'] - st['mean']), 1e-12 * np.abs(st['mean']))
        _note('send_var', np.abs(d['m2'] / np.maximum(st['count'], 1) - st['var']), 1e-5 * np.abs(st['var']))
        check_stats(dict(records=g[2], sums=g[1]), st)
    assert len(per) == len(want_shards) == world
    for a, b in zip(per, want_shards):
        np.testing.assert_array_equal(a, b)


# -------------------------------------------------------------------- variants
@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name', ['hub', 'random_perm'])
def test_exchange_ignore_label(gpu, name, defer):
    """ignore_label through the exchange: the hub (random_perm: one label)
    relabelled to 0, whose edges are dropped while 0 stays a node; with
    defer_stats the library writes the rows itself."""
    refs = _references(name, variant='zero')
    e_all, _ = O.boundary_features(_variant_labels(name, 'zero'), X.case_data(name))
    assert refs[0].shape[0] < e_all.shape[0] and refs[2][0] == 0 and not (refs[0] == 0).any()
    _check_whole(_exchange(name, 3, defer, variant='zero'), refs)


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name', ['hub', 'random_perm'])
def test_exchange_uint8_map(gpu, name, defer):
    """uint8 maps (sampled as value / 255) through pack and merge."""
    _check_whole(_exchange(name, 3, defer, kind='u8'), _references(name, kind='u8'))


@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('name', ['hub', 'random_perm'])
def test_exchange_custom_hist_range(gpu, name, defer):
    """hist_range = (-1, 2) on a map stretched past it on both sides (a map
    stretched to exactly [-1, 2] has no outliers of that range): the merge's
    scale / offset re-finalise the merged rows, both outlier slots filled."""
    hist = (-1.0, 2.0)
    lab, data, _, _ = _device_case(name, 'wide')
    stats = O.boundary_features(lab, data, lo=hist[0], hi=hist[1], return_stats=True)[2]
    assert stats['hist'][:, 0].sum() > 0 and stats['hist'][:, 41].sum() > 0
    assert stats['hist'][:, 1:41].sum() > 0
    _check_whole(_exchange(name, 3, defer, kind='wide', hist=hist), _references(name, kind='wide', hist=hist),
                 lo=hist[0], hi=hist[1])


@pytest.mark.parametrize('world', [3, 8, 32])
@pytest.mark.parametrize('offsets', [synthetic.NN_OFFSETS, SIX_OFFSETS, synthetic.LR_OFFSETS],
                         ids=['nn', 'six', 'lr'])
def test_exchange_columns_affinities(gpu, offsets, world):
    """The offset sets of cluster_tools_amd/synthetic.py (and the first six of
    the long-range set) on `columns`: every rank sees every pair; the pairs of
    the x / y long-range channels that no face joins are adjacent nowhere and
    dropped by the merge.  (The slab plan clips the halo at plane 0, so every
    world size up to 32 fits the 4-plane halo.)"""
    offs = tuple(tuple(o) for o in offsets)
    refs = _references('columns', offsets=offs)
    if len(offs) > 3:
        lab = X.case('columns').labels
        far = {(int(min(a, b)), int(max(a, b))) for a, b in zip(lab[0, :, 3:].ravel(), lab[0, :, :-3].ravel()) if a != b}
        assert far - {tuple(int(t) for t in k) for k in refs[0]}     # a sampled pair that is no edge
    _check_whole(_exchange('columns', world, False, offsets=offs), refs)


# ------------------------------------------------- split against restatement
@pytest.mark.parametrize('world', [2, 8, 32])
@pytest.mark.parametrize('name', X.BOUNDARY_CASES)
def test_split_matches_restatement(gpu, name, world):
    """ctg_mgpu_split of every rank on the gathered samples against
    split_counts(part, splitters(meta_all, W), W), the numpy restatement of
    k_mgpu_splitters / k_mgpu_bounds, on the rank's own table."""
    X.check_case(name, world)
    _, _, lab_t, data_t = _device_case(name)
    backend = cdist.HipBackend(defer_stats=False)
    locs = []
    try:
        for r in range(world):
            rd, own, end = cdist.slab_plan(lab_t.shape[0], world, r)
            locs.append(backend.local(lab_t[rd:end].contiguous(), data_t[rd:end].contiguous(), None, (own - rd, 0, 0),
                                      None, False, (0.0, 1.0)))
        meta_all = torch.stack([backend.sample(x) for x in locs])
        spl = splitters(meta_all.cpu().numpy(), world)
        assert np.all(spl[1:] >= spl[:-1])
        for x in locs:
            got = backend.split(x, meta_all, world).cpu().numpy()
            part = Part(x.edges(), None, None, None, x.nodes(), False)
            np.testing.assert_array_equal(got, split_counts(part, spl, world))
    finally:
        for x in locs:
            x.free()
