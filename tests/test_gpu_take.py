"""Applying a node assignment on the GPU (ctg_take.hip through
rag.assignment_dense / assignment_sparse / apply_assignment, and the
nifty.tools mirrors tools.take / takeDict) against numpy: table[seg] for a dense
table, np.searchsorted on the sorted keys for a sparse one.  Everything is
integers: every comparison is exact."""
import json
import os

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import _lib, rag, tools
from tests import take_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = T.CHUNK       # voxels per workgroup (ctg_plan.h: TAKE_CHUNK)
U64 = np.uint64
TOP = (1 << 64) - 1


def value_of(k):
    """A value per key that no other key has (k -> an odd multiple mod 2^40, + 1)."""
    return (np.asarray(k, dtype=U64) * U64(2654435761) + U64(1)) & U64((1 << 40) - 1)


def oracle(labels, table=None, keys=None, values=None, seg_begin=None, seg_off=None):
    """(out, nonzero per segment, n_missing, first_missing) of the flat uint64
    ``labels`` under a dense ``table`` or the sparse (keys, values)."""
    labels = np.asarray(labels, dtype=U64).reshape(-1)
    n = labels.size
    if seg_begin is None:
        seg_begin, seg_off = [0, n], [0]
    shifted = labels.copy()
    nonzero = []
    for k in range(len(seg_off)):
        s = slice(int(seg_begin[k]), int(seg_begin[k + 1]))
        nz = labels[s] != 0
        nonzero.append(int(nz.sum()))
        with np.errstate(over='ignore'):
            shifted[s] = np.where(nz, labels[s] + U64(seg_off[k]), U64(0))
    wrapped = shifted < labels
    if table is not None:
        table = np.asarray(table, dtype=U64)
        found = ~wrapped & (shifted < U64(len(table)))
        looked = table[np.where(found, shifted, U64(0)).astype(np.int64)] if len(table) else shifted
    else:
        order = np.argsort(np.asarray(keys, dtype=U64), kind='stable')
        ks, vs = np.asarray(keys, dtype=U64)[order], np.asarray(values, dtype=U64)[order]
        if len(ks):
            pos = np.minimum(np.searchsorted(ks, shifted), len(ks) - 1)
            found = ~wrapped & (ks[pos] == shifted)
            looked = vs[pos]
        else:
            found, looked = np.zeros(n, dtype=bool), shifted
    out = np.where(found, looked, shifted)
    cand = np.where(wrapped, labels, shifted)[~found]
    return out, np.array(nonzero, dtype=U64), int((~found).sum()), (int(cand.min()) if cand.size else None)


def check(a, labels, oracle_kw, segments=None, allow_missing=False, **kw):
    """apply_assignment == the oracle, for the output and every count."""
    want, nz, n_missing, first = oracle(labels, seg_begin=None if segments is None else segments[0],
                                        seg_off=None if segments is None else segments[1], **oracle_kw)
    out, info = rag.apply_assignment(a, labels, segments=segments, allow_missing=allow_missing, **kw)
    assert out.dtype == U64 and out.shape == np.asarray(labels).shape
    assert_array_equal(out.reshape(-1), want)
    assert_array_equal(info['nonzero'], nz)
    assert (info['n_missing'], info['first_missing']) == (n_missing, first)
    return out, info


@pytest.fixture(scope='module')
def dense(gpu):
    table = value_of(np.arange(5000))
    a = rag.assignment_dense(table)
    yield a, dict(table=table)
    a.free()


@pytest.fixture(scope='module')
def sparse(gpu):
    keys = np.random.default_rng(5).permutation(5000).astype(U64)
    a = rag.assignment_sparse(keys, value_of(keys))
    yield a, dict(keys=keys, values=value_of(keys))
    a.free()


@pytest.fixture(params=['dense', 'sparse'])
def both(request, dense, sparse):
    return dense if request.param == 'dense' else sparse


# --------------------------------------------------------------------------- the hand-computed case
@pytest.fixture(scope='module')
def kat():
    with open(os.path.join(ROOT, 'tests', 'golden', 'write_kat.json')) as f:
        return json.load(f)


def test_kat_dense(gpu, kat):
    labels = np.array(kat['labels'], dtype=U64)
    a = rag.assignment_dense(np.array(kat['dense_table'], dtype=U64))
    assert (a.n, a.max_value, a.kind) == (len(kat['dense_table']), kat['dense_max'], 'dense')
    out, info = rag.apply_assignment(a, labels, offset=kat['offset'])
    assert_array_equal(out, np.array(kat['result'], dtype=U64))
    assert (int(info['nonzero'][0]), info['n_missing'], info['first_missing']) == (kat['nonzero'], 0, None)
    a.free()
    m = kat['missing_dense']
    a = rag.assignment_dense(np.array(kat['dense_table'][:m['table_length']], dtype=U64))
    with pytest.raises(IndexError, match=r'^%d:' % m['first_missing']):
        rag.apply_assignment(a, labels, offset=kat['offset'])
    _, info = rag.apply_assignment(a, labels[0], offset=kat['offset'], check_only=True)   # (plane 0 holds no 6 or 7)
    assert info['n_missing'] == 0
    a.free()


def test_kat_sparse(gpu, kat):
    labels = np.array(kat['labels'], dtype=U64)
    a = rag.assignment_sparse(kat['sparse_keys'], kat['sparse_values'])
    assert (a.n, a.max_value, a.kind) == (len(kat['sparse_keys']), kat['sparse_max'], 'sparse')
    out, info = rag.apply_assignment(a, labels, offset=kat['offset'])
    assert_array_equal(out, np.array(kat['result'], dtype=U64))
    assert (int(info['nonzero'][0]), info['n_missing'], info['first_missing']) == (kat['nonzero'], 0, None)
    a.free()
    m = kat['missing_sparse']
    kv = [(k, v) for k, v in zip(kat['sparse_keys'], kat['sparse_values']) if k not in m['drop_keys']]
    a = rag.assignment_sparse([k for k, _ in kv], [v for _, v in kv])
    with pytest.raises(KeyError, match=r'%d:' % m['first_missing']):
        rag.apply_assignment(a, labels, offset=kat['offset'])
    out, info = rag.apply_assignment(a, labels, offset=kat['offset'], allow_missing=True)
    assert_array_equal(out, np.array(m['result_allow_missing'], dtype=U64))
    assert (info['n_missing'], info['first_missing']) == (m['n_missing'], m['first_missing'])
    a.free()


# --------------------------------------------------------------------------- lengths
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1]


@pytest.mark.parametrize('dtype', [np.uint64, np.uint32])
@pytest.mark.parametrize('n', LENGTHS)
def test_lengths(both, n, dtype):
    a, kw = both
    labels = np.random.default_rng(n).integers(0, 5000, size=n).astype(dtype)
    labels[::7] = 0
    check(a, labels, kw)


# --------------------------------------------------------------------------- runs
def run_labels(kind, n):
    rng = np.random.default_rng(11)
    if kind == 'one':
        return np.full(n, 17, dtype=U64)
    if kind == 'alternate':
        return (np.arange(n) % 2 + 1).astype(U64)
    if kind == 'every':
        return (np.arange(n) % 4999 + 1).astype(U64)
    if kind == 'runs':                                   # runs of 1 .. 15 voxels, a new label each
        lens = np.tile(np.arange(1, 16), n // 120 + 1)
        return np.repeat(rng.integers(1, 5000, size=lens.size), lens)[:n].astype(U64)
    assert kind == 'edges'                               # runs across every wave (128 voxels) and chunk edge
    x = rng.integers(1, 5000, size=n).astype(U64)
    for edge in range(128, n, 128):
        x[edge - 3:edge + 2] = x[edge]
    for edge in range(CHUNK, n, CHUNK):
        x[edge - 70:edge + 70] = 4242
    return x


@pytest.mark.parametrize('dtype', [np.uint64, np.uint32])
@pytest.mark.parametrize('kind', ['one', 'alternate', 'every', 'runs', 'edges'])
def test_runs(both, kind, dtype):
    a, kw = both
    labels = run_labels(kind, 2 * CHUNK + 77).astype(dtype)
    check(a, labels, kw)
    check(a, labels[1:], kw)                             # the same runs on the other pair parity


# --------------------------------------------------------------------------- segments
def test_segments(both):
    a, kw = both
    lens, offs = (5, 0, 130, 64), (0, 7, 1000, 1 << 40)
    seg_begin = np.concatenate([[0], np.cumsum(lens)])
    assert seg_begin[2] % 2 == 1                         # the third segment starts at an odd index
    labels = np.random.default_rng(3).integers(0, 3000, size=seg_begin[-1]).astype(U64)
    labels[5:5 + 130:3] = 0                              # zeros stay unshifted
    labels[135:] = 0                                     # an all-zero segment, under the largest offset
    _, info = check(a, labels, kw, segments=(seg_begin, offs))
    assert int(info['nonzero'][3]) == 0 and int(info['nonzero'][1]) == 0 and int(info['nonzero'][2]) > 0
    # several chunks per segment, and every voxel of the last one out of reach
    lens = (CHUNK + 3, 0, 2 * CHUNK - 1, 200)
    seg_begin = np.concatenate([[0], np.cumsum(lens)])
    labels = np.random.default_rng(4).integers(0, 3000, size=seg_begin[-1]).astype(U64)
    labels[-200:] += U64(1)
    labels[-200] = 1
    segments = (seg_begin, (1, 99, 1000, 1 << 40))
    if a.kind == 'sparse':
        check(a, labels, kw, segments=segments, allow_missing=True)
    with pytest.raises(KeyError if a.kind == 'sparse' else IndexError, match=r'%d: .*\(200 voxel' % ((1 << 40) + 1)):
        rag.apply_assignment(a, labels, segments=segments)


# --------------------------------------------------------------------------- past the first turn, the slot plans
def check_dev(a, labels, oracle_kw, segments=None, allow_missing=False):
    """check() with the labels on the device and a device ``out`` prefilled with
    -1: a voxel that no workgroup writes keeps it, whatever an earlier call left
    in a pooled buffer.  With missing labels and no allow_missing the call must
    raise, naming the smallest label and the count."""
    import torch
    want, nz, n_missing, first = oracle(labels, seg_begin=None if segments is None else segments[0],
                                        seg_off=None if segments is None else segments[1], **oracle_kw)
    t = torch.from_numpy(labels.view(np.int64 if labels.dtype == U64 else np.int32)).cuda()
    out = torch.full((labels.size,), -1, dtype=torch.int64, device='cuda')
    if n_missing and not allow_missing:
        with pytest.raises(KeyError if a.kind == 'sparse' else IndexError, match=r'^.?%d: .*\(%d voxel' % (first, n_missing)):
            rag.apply_assignment(a, t, segments=segments, out=out)
        return
    got, info = rag.apply_assignment(a, t, segments=segments, allow_missing=allow_missing, out=out)
    assert got is out
    assert_array_equal(out.cpu().numpy().view(U64), want)
    assert_array_equal(info['nonzero'], nz)
    assert (info['n_missing'], info['first_missing']) == (n_missing, first)


@pytest.mark.parametrize('n', [(1 << 20) + 1, 3 * (1 << 20) + 7])
def test_dense_max_past_one_turn(gpu, n):
    """k_take_max (csrc/ctg_take.hip) past its first turn of 4096 x 256 = 2^20
    entries: the table's only maximum at the last entry, at entry 2^20 (the
    first of the second turn) and at entry 0; one lookup through each table."""
    assert T.max_turns(n) >= 2 and T.max_turns(1 << 20) == 1
    base = value_of(np.arange(n))                          # (below 2^40)
    labels = np.random.default_rng(n).integers(0, n, size=3 * CHUNK + 5).astype(U64)
    for at in (n - 1, 1 << 20, 0):
        table = base.copy()
        table[at] = U64((1 << 41) + at)
        labels[7] = at
        a = rag.assignment_dense(table)
        assert (a.n, a.max_value, a.kind) == (n, (1 << 41) + at, 'dense')
        check_dev(a, labels, dict(table=table))
        a.free()


def segment_plans():
    """name -> (lengths, expected count slots): 4097 segments, one count slot
    each; 4096, 64 slots each; three of which one holds 70 chunks, so that its
    workgroups wrap around the 64 slots (`t & 63`).  The short segments' lengths
    cycle 0 .. 5, with one of 2 CHUNK + 3 among them."""
    def short(k):
        lens = (np.arange(k) % 6).tolist()
        lens[k // 2] = 2 * CHUNK + 3
        return lens
    return dict(one_slot=(short(T.SLOT_SEGMENTS + 1), 1), slots=(short(T.SLOT_SEGMENTS), T.SLOTS),
                wrap=([5, 70 * CHUNK - 9, 300], T.SLOTS))


@pytest.mark.parametrize('dtype', [np.uint64, np.uint32])
@pytest.mark.parametrize('plan', ['one_slot', 'slots', 'wrap'])
def test_segment_count_slots(both, plan, dtype):
    """k_take's per-segment counters (csrc/ctg_take.hip; ctg_plan.h:
    take_count_slots): one slot a segment past 4096 segments, 64 up to there,
    and a segment of 70 chunks whose workgroups wrap around its 64 slots.
    seg_nonzero per segment, the output, and the missing count and smallest
    missing label with absent labels in the late segments, against numpy."""
    a, kw = both
    lens, slots = segment_plans()[plan]
    assert T.count_slots(len(lens)) == slots
    assert plan != 'wrap' or -(-max(lens) // CHUNK) > T.SLOTS
    seg_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    offs = (np.arange(len(lens)) % 7).astype(U64)
    rng = np.random.default_rng(len(lens))
    labels = rng.integers(0, 4990, size=int(seg_begin[-1])).astype(dtype)
    labels[::5] = 0
    check_dev(a, labels, kw, segments=(seg_begin, offs))
    late = rng.integers(int(seg_begin[-1]) * 3 // 4, int(seg_begin[-1]), size=40)
    labels[late] = (6000 + (late % 13)).astype(dtype)       # absent from the table, in the late segments only
    check_dev(a, labels, kw, segments=(seg_begin, offs))    # refused, naming the smallest and the count
    if a.kind == 'sparse':
        check_dev(a, labels, kw, segments=(seg_begin, offs), allow_missing=True)


# --------------------------------------------------------------------------- dense range
def test_dense_range(gpu):
    a = rag.assignment_dense(np.array([9], dtype=U64))   # a table of length 1
    out, info = rag.apply_assignment(a, np.zeros(5, dtype=U64), offset=3)
    assert_array_equal(out, np.full(5, 9, dtype=U64))
    assert info['n_missing'] == 0 and int(info['nonzero'][0]) == 0
    a.free()
    table = value_of(np.arange(100))
    a = rag.assignment_dense(table)
    labels = np.array([99, 0, 99, 5], dtype=U64)         # n_table - 1: found
    check(a, labels, dict(table=table))
    labels = np.array([99, 100, 7, 100, 250, 100], dtype=U64)   # n_table: out of range
    with pytest.raises(IndexError, match=r'^100: .*\(4 voxel\(s\)\); the table has 100 entries'):
        rag.apply_assignment(a, labels)
    a.free()


# --------------------------------------------------------------------------- sparse tables
def test_sparse_empty_and_one(gpu):
    a = rag.assignment_sparse([], [])
    assert (a.n, a.max_value) == (0, 0)
    labels = np.array([4, 0, 9, 4], dtype=U64)
    out, info = rag.apply_assignment(a, labels, allow_missing=True)      # every label missing, 0 included
    assert_array_equal(out, labels)
    assert (info['n_missing'], info['first_missing']) == (4, 0)
    a.free()
    a = rag.assignment_sparse([4], [77])
    check(a, labels, dict(keys=[4], values=[77]), allow_missing=True)
    a.free()


@pytest.mark.parametrize('case', ['multiples', 'many', 'extremes'])
def test_sparse_keys(gpu, case):
    if case == 'multiples':                              # collide under a masked identity hash
        keys = np.arange(1000, dtype=U64) << U64(20)
    elif case == 'many':                                 # 2^16 + 1 keys: the capacity doubles here
        keys = np.random.default_rng(1).permutation(1 << 18)[:(1 << 16) + 1].astype(U64)
    else:
        keys = np.array([0, 1 << 32, 1 << 63, TOP], dtype=U64)
    a = rag.assignment_sparse(keys, value_of(keys))
    assert a.n == len(keys) and a.max_value == int(value_of(keys).max())
    rng = np.random.default_rng(2)
    labels = np.concatenate([keys[rng.integers(0, len(keys), size=3000)], keys, keys + U64(1)])
    check(a, labels, dict(keys=keys, values=value_of(keys)), allow_missing=True)
    a.free()


def test_sparse_duplicates_refused(gpu):
    with pytest.raises(_lib.CtgError, match='2 duplicate'):
        rag.assignment_sparse(np.array([5, 6, 5, 7, TOP, TOP], dtype=U64), np.arange(6, dtype=U64))


# --------------------------------------------------------------------------- missing and wrap
def test_missing_and_wrap(both):
    a, kw = both
    labels = np.array([3, 0, TOP - 1, 6000, 0, 7000, 6000], dtype=U64)
    with pytest.raises(KeyError if a.kind == 'sparse' else IndexError, match=r'^.?6000:'):
        rag.apply_assignment(a, labels)
    # offset 5 wraps TOP - 1 to 3, which has an entry: missing all the same, candidate TOP - 1
    labels = np.array([3, 0, TOP - 1, 0, TOP - 1], dtype=U64)
    with pytest.raises(KeyError if a.kind == 'sparse' else IndexError, match=r'^.?%d:' % (TOP - 1)):
        rag.apply_assignment(a, labels, offset=5)
    if a.kind == 'sparse':
        out, info = check(a, labels, kw, segments=([0, 5], [5]), allow_missing=True)
        assert (info['n_missing'], info['first_missing']) == (2, TOP - 1)
        assert_array_equal(out, np.array([int(value_of(8)), int(value_of(0)), 3, int(value_of(0)), 3], dtype=U64))
        check(a, np.array([3, 6000, 0, 7000], dtype=U64), kw, allow_missing=True)
    else:
        with pytest.raises(ValueError):
            rag.apply_assignment(a, labels, allow_missing=True)


# --------------------------------------------------------------------------- check only, in place, streams
def test_check_only(both):
    a, kw = both
    import torch
    labels = np.random.default_rng(8).integers(0, 5000, size=CHUNK + 131).astype(U64)
    _, info = check(a, labels, kw)
    out, only = rag.apply_assignment(a, labels, check_only=True)
    assert out is None
    assert_array_equal(only['nonzero'], info['nonzero'])
    assert (only['n_missing'], only['first_missing']) == (info['n_missing'], info['first_missing'])
    # on the device next to a canary: the check-only call gets no out to write, and leaves its neighbours alone
    t = torch.full((labels.size + 64,), -7, dtype=torch.int64, device='cuda')
    t[32:-32] = torch.from_numpy(labels.astype(np.int64)).cuda()
    before = t.clone()
    _, dev = rag.apply_assignment(a, t[32:-32], check_only=True)
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    assert_array_equal(dev['nonzero'], info['nonzero'])


def test_in_place(both):
    a, kw = both
    import torch
    labels = np.random.default_rng(9).integers(0, 5000, size=(3, 37, 41)).astype(U64)
    want = oracle(labels, **kw)[0].reshape(labels.shape)
    t = torch.from_numpy(labels.astype(np.int64)).cuda()
    sep, _ = rag.apply_assignment(a, t)
    same, _ = rag.apply_assignment(a, t, out=t)
    assert same is t and torch.equal(sep, t)
    assert_array_equal(t.cpu().numpy().astype(U64), want)
    t = torch.from_numpy(labels.astype(np.int64)).cuda().reshape(-1)[1:]       # an odd address
    rag.apply_assignment(a, t, out=t)
    assert_array_equal(t.cpu().numpy().astype(U64), want.reshape(-1)[1:])
    host = labels.copy()
    rag.apply_assignment(a, host, out=host)
    assert_array_equal(host, want)
    buf = np.zeros(4, dtype=U64)
    with pytest.raises(ValueError, match='64-bit'):
        rag.apply_assignment(a, buf.view(np.uint32)[:4], out=buf)


def test_stream(both):
    a, kw = both
    import torch
    labels = np.random.default_rng(10).integers(0, 5000, size=3 * CHUNK + 5).astype(U64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(labels.astype(np.int64)).cuda()
        out, info = rag.apply_assignment(a, t)
    s.synchronize()
    want, nz, _, _ = oracle(labels, **kw)
    assert_array_equal(out.cpu().numpy().astype(U64), want)
    assert_array_equal(info['nonzero'], nz)


# --------------------------------------------------------------------------- the nifty.tools mirrors
def test_tools_take(gpu):
    rng = np.random.default_rng(12)
    table = rng.integers(0, 1 << 31, size=700).astype(np.uint32)
    vol = rng.integers(0, 700, size=(5, 9, 33)).astype(np.uint64)
    out = tools.take(table, vol)
    assert out.dtype == np.uint32 and out.shape == vol.shape          # the dtype of relabeling
    assert_array_equal(out, table[vol])
    uv = rng.integers(0, 700, size=(211, 2)).astype(np.uint32)
    table64 = table.astype(np.uint64) << np.uint64(20)
    out = tools.take(table64, uv)
    assert out.dtype == np.uint64 and out.shape == uv.shape
    assert_array_equal(out, table64[uv])
    with pytest.raises(IndexError, match='^700:'):
        tools.take(table, np.array([1, 700, 2], dtype=np.uint64))


def test_tools_take_dict(gpu):
    rng = np.random.default_rng(13)
    keys = rng.permutation(2000)[:700]
    d = {int(k): int(k) * 3 + 1 for k in keys}
    vol = keys[rng.integers(0, 700, size=(5, 9, 33))].astype(np.uint64)
    out = tools.takeDict(d, vol)
    assert out.dtype == np.uint64 and out.shape == vol.shape
    assert_array_equal(out, vol * np.uint64(3) + np.uint64(1))
    uv = keys[rng.integers(0, 700, size=(211, 2))].astype(np.uint32)
    out = tools.takeDict(d, uv)
    assert out.dtype == np.uint32 and out.shape == uv.shape           # the dtype of toRelabel
    assert_array_equal(out, uv * np.uint32(3) + np.uint32(1))
    with pytest.raises(KeyError):
        tools.takeDict(d, np.array([int(keys[0]), 2000], dtype=np.uint64))
    d[int(keys[0])] = 1 << 32
    with pytest.raises(OverflowError):
        tools.takeDict(d, uv)
    assert tools.takeDict(d, uv.astype(np.uint64)).dtype == np.uint64


# --------------------------------------------------------------------------- no workspace state
def test_deferred_stats_survive_an_apply_call(both):
    """A CTG_DEFER_STATS table still packs after assignment calls on its device:
    they use call-sized buffers only.  The exchange simulation of
    tests/exchange_sim.py with 2 slabs and a build, an apply and a check-only
    call right before every pack (features: float64 sums in another order, as in
    the overlaps' twin of this test)."""
    from cluster_tools_amd import dist as cdist
    from tests.exchange_sim import simulate
    a, kw = both
    lab, bnd = rag.synth_volume((40, 48, 56), cell=6, seed=21)
    labels = np.random.default_rng(14).integers(0, 5000, size=3 * CHUNK).astype(U64)
    calls = []

    def apply_between():
        check(a, labels, kw)
        rag.apply_assignment(a, labels, check_only=True)
        rag.assignment_sparse(labels[:64] + U64(1) + np.arange(64, dtype=U64) * U64(6000), labels[:64]).free()
        calls.append(1)

    eager = simulate(cdist.HipBackend(defer_stats=False), lab, bnd, 2)
    shards = simulate(cdist.HipBackend(defer_stats=True), lab, bnd, 2, fresh=True, before_pack=apply_between)
    assert calls
    assert_array_equal(np.concatenate([x.edges() for x in shards]), np.concatenate([x.edges() for x in eager]))
    np.testing.assert_allclose(np.concatenate([x.features() for x in shards]),
                               np.concatenate([x.features() for x in eager]), rtol=1e-12, atol=1e-15)
