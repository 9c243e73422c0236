"""Named label volumes that drive the multi-GPU exchange (ctg_mgpu_sample /
split / pack / merge, cluster_tools_amd/csrc/ctg_mgpu.hip) into the corners a
spatially ordered synthetic volume never reaches.  Pure numpy; shared by
tests/test_dist_cpu.py (the numpy restatement) and
tests/test_gpu_exchange_cases.py (the kernels).  Test infrastructure only.

Every case states what it forces as a precondition, asserted by
``check_case`` from numpy and oracle.rag_oracle on the z-slabs (and the
restated splitter rule of tests/dist_helpers.py) before any library call: a
case that no longer holds what it claims fails there, loudly.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import rag_oracle as O

SHAPE = (64, 12, 16)      # Z = 64: world 32 with two-plane slabs
WORLDS = (1, 2, 3, 8, 16, 32)
HIGH = (1 << 63) - 10     # columns_high: labels on both sides of bit 63
TOP = (1 << 64) - 2       # one_edge: the upper label
GOLDEN = 0x9E3779B97F4A7C15
NN = [[-1, 0, 0], [0, -1, 0], [0, 0, -1]]
LR_OFFSETS = NN + [[-2, 0, 0]]
LR_SHAPE, LR_WORLD = (32, 4, 8), 4
# lr_adjacency: (A, B) touch in rank 0 and are paired by the -2 offset in rank 3,
# (A2, B2) the other way round; (C, D) never touch, paired in ranks 1 and 2
LR = dict(A=10, B=20, A2=11, B2=21, C=40, D=50, T=30)

Case = namedtuple('Case', 'name labels worlds offsets')


def _grid(shape=SHAPE):
    return np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing='ij')


def _columns():
    z, y, x = _grid()
    return ((y // 3) * 8 + x // 2 + 1).astype(np.uint64)


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    z, y, x = _grid()
    if name == 'columns':
        return _columns()
    if name == 'columns_high':
        return _columns() + np.uint64(HIGH)
    if name == 'hub':
        lab = np.ones(SHAPE, np.uint64)
        m = rng.random(SHAPE) < 0.15
        lab[m] = rng.integers(2, 400, int(m.sum())).astype(np.uint64)
        return lab
    if name == 'reversed':
        return ((SHAPE[0] - 1 - z) // 2 * 100 + y // 4 * 10 + x // 4 + 1).astype(np.uint64)
    if name == 'mostly_uniform':
        lab = np.full(SHAPE, 7, np.uint64)
        lab[:8] = rng.integers(1, 50, (8,) + SHAPE[1:]).astype(np.uint64)
        return lab
    if name == 'one_label':
        return np.full(SHAPE, 3, np.uint64)
    if name == 'one_edge':
        lab = np.full(SHAPE, 3, np.uint64)
        lab[40:] = np.uint64(TOP)
        return lab
    if name == 'random_perm':
        return rng.integers(1, 2000, SHAPE).astype(np.uint64) * np.uint64(GOLDEN)   # mod 2^64
    if name == 'lr_adjacency':
        lab = np.ones(LR_SHAPE, np.uint64)
        # rank 0 (planes 0-7): A | B share an x face; A2 / T / B2 stacked along z
        lab[2, 1, 1], lab[2, 1, 2] = LR['A'], LR['B']
        lab[3, 2, 5], lab[4, 2, 5], lab[5, 2, 5] = LR['A2'], LR['T'], LR['B2']
        # rank 3 (planes 24-31): A / T / B stacked; A2 | B2 share an x face
        lab[26, 1, 1], lab[27, 1, 1], lab[28, 1, 1] = LR['A'], LR['T'], LR['B']
        lab[29, 2, 5], lab[29, 2, 6] = LR['A2'], LR['B2']
        # ranks 1 and 2 (planes 8-15, 16-23): C / T / D stacked, never touching
        for z0 in (10, 18):
            lab[z0, 2, 3], lab[z0 + 1, 2, 3], lab[z0 + 2, 2, 3] = LR['C'], LR['T'], LR['D']
        return lab
    raise KeyError(name)


BOUNDARY_CASES = ('columns', 'columns_high', 'hub', 'reversed', 'mostly_uniform', 'one_label', 'one_edge',
                  'random_perm')


@functools.lru_cache(maxsize=None)
def case(name):
    """The case ``name``; its arrays are shared between the tests (read-only)."""
    lab = _build(name)
    lab.setflags(write=False)
    if name == 'lr_adjacency':
        return Case(name, lab, (LR_WORLD,), LR_OFFSETS)
    return Case(name, lab, WORLDS, None)


@functools.lru_cache(maxsize=None)
def case_data(name, kind='f32', n_channels=None):
    """The boundary map / affinities of a case: k / 256 for random k in
    [0, 256], float32 (exact); 'u8': random bytes; 'wide': the map stretched
    to [-1.5, 2.5] (exact in float32), which leaves samples on both sides of
    the histogram range (-1, 2).  n_channels: affinities of that many
    channels (default: one per offset of the case, or a boundary map)."""
    c = case(name)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    if n_channels is None and c.offsets is not None:
        n_channels = len(c.offsets)
    shape = c.labels.shape if n_channels is None else (n_channels,) + c.labels.shape
    if kind == 'u8':
        d = rng.integers(0, 256, shape).astype(np.uint8)
    else:
        d = (rng.integers(0, 257, shape) / 256).astype(np.float32)
        if kind == 'wide':
            d = (d * np.float32(4.0) - np.float32(1.5)).astype(np.float32)
    d.setflags(write=False)
    return d


def slab_planes(Z, world, down=1):
    """(read_begin, own_begin, own_end) of every rank: ctg_mgpu_slab restated."""
    out = []
    for r in range(world):
        own, end = Z * r // world, Z * (r + 1) // world
        out.append((own - min(down, own), own, end))
    return out


@functools.lru_cache(maxsize=None)
def plan(name, world):
    """What the restated rules say the exchange of a boundary case does at
    this world size: every slab's local edges and nodes, the splitters, and
    the count matrix [src][dst][rows, nodes]."""
    from tests.dist_helpers import Part, S, SIGN, slab_nodes, split_counts, splitters
    lab = case(name).labels
    edges, nodes, meta = [], [], []
    for rd, own, end in slab_planes(lab.shape[0], world):
        e = O.rag_edges(lab[rd:end], own_begin=(own - rd, 0, 0))
        edges.append(e)
        nodes.append(slab_nodes(lab[rd:end], (own - rd, 0, 0)))
        m = np.zeros(S + 1, np.int64)
        if e.shape[0]:
            m[:S] = (e[(np.arange(S) * e.shape[0]) // S, 0] ^ SIGN).view(np.int64)
        m[S] = e.shape[0]
        meta.append(m)
    spl = splitters(np.stack(meta), world)
    counts = np.stack([split_counts(Part(e, None, None, None, n, False), spl, world) for e, n in zip(edges, nodes)])
    return dict(edges=edges, nodes=nodes, spl=spl, counts=counts)


def _multiplicity(edges):
    """How many slabs hold each key of their union."""
    allk = np.concatenate(edges)
    _, inv = O._unique_pairs(allk, return_inverse=True)
    return np.bincount(inv)


def check_case(name, world):
    """Assert what the case claims to force, at this world size."""
    c = case(name)
    if name == 'lr_adjacency':
        return _check_lr(c)
    p = plan(name, world)
    E = [e.shape[0] for e in p['edges']]
    cnt = p['counts']
    off = ~np.eye(world, dtype=bool)
    recv_rows = np.where(off, cnt[:, :, 0], 0).sum(axis=0)
    own_rows = cnt[np.arange(world), np.arange(world), 0]
    if name in ('columns', 'columns_high'):
        assert all(n == 52 for n in E) and E[0] < 1024          # every key in every slab; the samples repeat rows
        if world >= 3:
            assert _multiplicity(p['edges']).min() == world      # the same key from W - 1 remote sources
            remote = (np.where(off, cnt[:, :, 0], 0) > 0).sum(axis=0)
            assert remote.max() >= 2 and np.all((remote >= 2) | (cnt[:, :, 0].sum(axis=0) == 0))
        if world == 32:
            assert (cnt[:, :, 0].sum(axis=0) == 0).any()         # 31 distinct u over 32 ranks: empty shards
            assert (p['spl'][1:] == p['spl'][:-1]).any()   # and equal splitters
        if name == 'columns_high':
            u = p['edges'][0][:, 0]
            assert (u < np.uint64(1 << 63)).any() and (u >= np.uint64(1 << 63)).any()
            if world >= 8:
                assert (p['spl'] < np.uint64(1 << 63)).any() and (p['spl'] >= np.uint64(1 << 63)).any()
    elif name == 'hub':
        if world >= 3:
            assert (cnt[:, :, 0].sum(axis=0) == 0).any()         # an empty shard
        if world >= 8:
            assert (p['spl'][1:] == p['spl'][:-1]).any()   # equal splitters
            assert recv_rows.max() > 0.5 * sum(E)                # one rank receives most of every table
        if world == 8:
            assert (cnt[:, :, 0].sum(axis=0) == 0).sum() == 5
    elif name == 'reversed':
        if world >= 2:
            assert own_rows[0] == 0 and recv_rows[0] > 0         # rank 0: n_own == 0, M > 0
            assert own_rows.sum() < 0.4 * sum(E)                 # most rows leave their rank
        if world >= 2 and world != 3:
            assert own_rows.sum() < 0.01 * sum(E)                # (nearly all, unless a middle slab maps to itself)
    elif name == 'mostly_uniform':
        if world >= 2:
            assert min(E) == 0 and max(E) > 0                    # cnt_r == 0 next to ranks with rows
            assert all(n.shape[0] == 1 for n, e in zip(p['nodes'], E) if e == 0)
    elif name == 'one_label':
        assert sum(E) == 0
        if world >= 2:
            assert np.all(p['spl'] == 0)
            assert np.all(cnt[:-1, -1] == [0, 1])                # node-only segments, all to the last rank
    elif name == 'one_edge':
        assert sorted(E) == [0] * (world - 1) + [1]
        if world >= 2:
            assert (cnt[:, :, 0].sum(axis=0) == 0).sum() == world - 1
            assert (cnt[:, :, 0] == 0)[off].any() and ((cnt[:, :, 0] == 0) & (cnt[:, :, 1] > 0))[off].any()
    elif name == 'random_perm':
        allk = O._unique_pairs(np.concatenate(p['edges']))
        assert allk.shape[0] > 30000
        assert (allk[:, 0] >= np.uint64(1 << 63)).any() and (allk[:, 0] < np.uint64(1 << 32)).sum() == 0
        if world >= 3:
            assert own_rows.sum() < 0.5 * sum(E)                 # most rows are exchanged
            assert (_multiplicity(p['edges']) >= 2).any()


def _check_lr(c):
    """lr_adjacency, from the geometry: which rank's planes hold each face and
    each -2 pairing of the three label pairs."""
    lab = c.labels
    planes = slab_planes(lab.shape[0], LR_WORLD, down=2)

    def owners(u, v, what):
        """ranks whose owned planes hold a face / a -2 pairing of (u, v)"""
        out = set()
        for r, (_, own, end) in enumerate(planes):
            if what == 'face':
                hit = False
                for ax in range(3):
                    lo, up = O._face_slices(lab.shape, ax, (own, 0, 0), (end,) + lab.shape[1:])
                    a, b = lab[lo], lab[up]
                    hit |= bool((((a == u) & (b == v)) | ((a == v) & (b == u))).any())
            else:
                b0 = max(own, 2)
                p, q = lab[b0:end], lab[b0 - 2:end - 2]
                hit = bool((((p == u) & (q == v)) | ((p == v) & (q == u))).any())
            if hit:
                out.add(r)
        return out

    assert owners(LR['A'], LR['B'], 'face') == {0} and owners(LR['A'], LR['B'], 'pair') == {3}
    assert owners(LR['A2'], LR['B2'], 'face') == {3} and owners(LR['A2'], LR['B2'], 'pair') == {0}
    assert owners(LR['C'], LR['D'], 'face') == set() and owners(LR['C'], LR['D'], 'pair') == {1, 2}
    edges = O.rag_edges(lab)
    have = {tuple(int(t) for t in e) for e in edges}
    assert (LR['A'], LR['B']) in have and (LR['A2'], LR['B2']) in have and (LR['C'], LR['D']) not in have
