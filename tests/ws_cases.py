"""The seeded watershed's rule on the CPU (include/ctg.h: ctg_seeded_watershed):
the edge order, the defining oracle (a plain Kruskal over a list union-find), a
fast oracle for larger cases (edge ranks into scipy's minimum spanning tree), the
minimax pass height, a priority flood with FIFO ties to show where the rule may
differ from one, the size filter, and the case generators the CPU and GPU tests
share."""
import heapq

import numpy as np

SHAPES = [(1, 1, 1), (1, 1, 130), (16, 8, 64), (17, 9, 65), (33, 17, 129)]
HEIGHTS = ['distinct', 'levels2', 'levels8', 'levels256', 'constant', 'ramp', 'serpentine', 'special']
SEEDS = ['none', 'one', 'all', 'scattered', 'blobs', 'big']
# csrc/ctg_plan.h: WS_MAX_GRID workgroups of WS_THREADS voxels take one turn of the kernels' stride loops
# (tests/test_ws_host.py pins the mirror against ws_plan)
GRID_TURN = 4096 * 256
BIG = (5, 400, 530)             # 1.06 M voxels: a second, ragged turn


# --------------------------------------------------------------------------- the order
def key_u32(h):
    """k(h): the order-preserving u32 image of float32 heights."""
    b = np.ascontiguousarray(h, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b & 0x80000000) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def grid_edges(shape, two_d=False):
    """(lower voxel, upper voxel, edge id) of every edge of the box, C-order indices."""
    lin = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    us, vs, ids = [], [], []
    for axis in range(1 if two_d else 0, 3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis] = slice(0, shape[axis] - 1)
        hi[axis] = slice(1, shape[axis])
        u, v = lin[tuple(lo)].ravel(), lin[tuple(hi)].ravel()
        us.append(u)
        vs.append(v)
        ids.append(3 * u + axis)
    return np.concatenate(us), np.concatenate(vs), np.concatenate(ids)


def ordered_edges(h, two_d=False):
    """The edges of the box in ascending order of (max k, min k, id)."""
    k = key_u32(h).ravel().astype(np.int64)
    u, v, eid = grid_edges(h.shape, two_d)
    ku, kv = k[u], k[v]
    order = np.lexsort((eid, np.minimum(ku, kv), np.maximum(ku, kv)))
    return u[order], v[order], eid[order]


# --------------------------------------------------------------------------- the oracles
def oracle_kruskal(h, seeds, two_d=False):
    """The definition: the edges in ascending order, two sets joined unless they
    are one already or both hold a seed."""
    h = np.asarray(h, dtype=np.float32)
    s = np.asarray(seeds).astype(np.uint64).ravel()
    n = s.size
    parent = list(range(n))
    label = [int(x) for x in s]

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    u, v, _ = ordered_edges(h, two_d)
    for a, b in zip(u.tolist(), v.tolist()):
        a, b = find(a), find(b)
        if a == b or (label[a] and label[b]):
            continue
        parent[b] = a
        label[a] = label[a] or label[b]
    return np.array([label[find(i)] for i in range(n)], dtype=np.uint64).reshape(h.shape)


def oracle_fast(h, seeds, two_d=False):
    """The same forest by scipy: every edge weighs its rank in the order, and a
    root node is tied to every seeded voxel below all of them, so the spanning
    tree is unique; without the root, each of its trees holds one seed at most."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    h = np.asarray(h, dtype=np.float32)
    s = np.asarray(seeds).astype(np.uint64).ravel()
    n = s.size
    u, v, _ = ordered_edges(h, two_d)
    seeded = np.flatnonzero(s)
    rows = np.concatenate([np.full(seeded.size, n, dtype=np.int64), u])
    cols = np.concatenate([seeded, v])
    w = np.arange(1, rows.size + 1, dtype=np.float64)
    tree = minimum_spanning_tree(coo_matrix((w, (rows, cols)), shape=(n + 1, n + 1)).tocsr()).tocoo()
    keep = (tree.row != n) & (tree.col != n)
    forest = coo_matrix((np.ones(int(keep.sum())), (tree.row[keep], tree.col[keep])), shape=(n, n))
    _, comp = connected_components(forest, directed=False)
    lab = np.zeros(comp.max() + 1, dtype=np.uint64)
    assert np.unique(comp[seeded]).size == seeded.size   # one seed per tree
    lab[comp[seeded]] = s[seeded]
    return lab[comp].reshape(h.shape)


def size_filter(labels, h, limit, two_d=False):
    """elf's apply_size_filter as include/ctg.h restates it -> (labels, dropped)."""
    labels = np.asarray(labels, dtype=np.uint64)
    if limit <= 1:
        return labels.copy(), 0
    kept = labels.copy()
    dropped = 0
    for sl in ([slice(z, z + 1) for z in range(labels.shape[0])] if two_d else [slice(None)]):
        ids, counts = np.unique(kept[sl], return_counts=True)
        small = ids[(counts < limit) & (ids != 0)]
        dropped += small.size
        part = kept[sl]
        part[np.isin(part, small)] = 0
    if dropped == 0:
        return labels.copy(), 0
    return oracle_fast(h, kept, two_d), dropped


def oracle(h, seeds, limit=0, two_d=False):
    """What ctg_seeded_watershed returns: (labels, info)."""
    out = oracle_fast(h, seeds, two_d)
    out, dropped = size_filter(out, h, limit, two_d)
    return out, (int(out.max()) if out.size else 0, int((out == 0).sum()), dropped)


def round_bound(seeds):
    """ceil(log2(U + 1)) + 1 for U unseeded voxels."""
    unseeded = int((np.asarray(seeds) == 0).sum())
    return int(unseeded).bit_length() + 1


# --------------------------------------------------------------------------- pass heights and a flood
def _neighbours(shape, two_d):
    strides = (shape[1] * shape[2], shape[2], 1)

    def nb(i):
        c = (i // strides[0], (i // strides[1]) % shape[1], i % shape[2])
        for axis in range(1 if two_d else 0, 3):
            if c[axis] > 0:
                yield i - strides[axis]
            if c[axis] + 1 < shape[axis]:
                yield i + strides[axis]
    return nb


def pass_height(h, sources, two_d=False):
    """Per voxel, the smallest over the paths to a source of the largest k on the
    path (both ends included); -1 where no source is reachable."""
    k = key_u32(h).ravel().astype(np.int64)
    src = np.asarray(sources).ravel()
    nb = _neighbours(h.shape, two_d)
    best = np.full(k.size, -1, dtype=np.int64)
    heap = [(int(k[i]), int(i)) for i in np.flatnonzero(src)]
    heapq.heapify(heap)
    while heap:
        d, i = heapq.heappop(heap)
        if best[i] >= 0:
            continue
        best[i] = d
        for j in nb(i):
            if best[j] < 0:
                heapq.heappush(heap, (max(d, int(k[j])), j))
    return best.reshape(h.shape)


def tie_zone(h, seeds, two_d=False):
    """Where two labels or more attain the minimal pass height."""
    seeds = np.asarray(seeds)
    best = pass_height(h, seeds != 0, two_d)
    n = np.zeros(h.shape, dtype=np.int64)
    for lab in np.unique(seeds[seeds != 0]):
        n += pass_height(h, seeds == lab, two_d) == best
    return n >= 2


def fifo_flood(h, seeds, two_d=False):
    """A priority flood with FIFO ties: a voxel is labelled when it is first
    reached and queued at the level it was reached at."""
    k = key_u32(h).ravel().astype(np.int64)
    out = np.asarray(seeds).astype(np.uint64).ravel().copy()
    nb = _neighbours(h.shape, two_d)
    heap = []
    count = 0
    for i in np.flatnonzero(out):
        heap.append((int(k[i]), count, int(i)))
        count += 1
    heapq.heapify(heap)
    while heap:
        d, _, i = heapq.heappop(heap)
        for j in nb(i):
            if out[j] == 0:
                out[j] = out[i]
                heapq.heappush(heap, (max(d, int(k[j])), count, j))
                count += 1
    return out.reshape(h.shape)


# --------------------------------------------------------------------------- cases
def heights(kind, shape, seed=0):
    rng = np.random.default_rng(1000 + seed)
    n = int(np.prod(shape))
    if kind == 'distinct':
        return rng.permutation(n).astype(np.float32).reshape(shape) / np.float32(max(n, 1))
    if kind.startswith('levels'):
        return rng.integers(0, int(kind[6:]), size=shape).astype(np.float32)
    if kind == 'constant':
        return np.full(shape, 0.5, dtype=np.float32)
    if kind == 'ramp':
        return np.broadcast_to(np.arange(shape[2], dtype=np.float32), shape).copy()
    if kind == 'serpentine':
        # a one-voxel valley between walls: even rows of even slices, joined at alternating ends
        h = (1.0 + rng.random(shape)).astype(np.float32)
        low = (0.5 * rng.random(shape)).astype(np.float32)
        valley = np.zeros(shape, dtype=bool)
        valley[::2, ::2, :] = True
        for y in range(1, shape[1], 2):
            valley[::2, y, (shape[2] - 1) if (y // 2) % 2 == 0 else 0] = True
        valley[1::2, 0, 0] = True
        h[valley] = low[valley]
        return h
    if kind == 'special':
        pool = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 1e-45, -1e-45], dtype=np.float32)
        return pool[rng.integers(0, pool.size, size=shape)]
    raise ValueError(kind)


def seeds(kind, shape, seed=0, dtype=np.uint64):
    rng = np.random.default_rng(2000 + seed)
    n = int(np.prod(shape))
    s = np.zeros(n, dtype=np.uint64)
    if kind == 'none':
        pass
    elif kind == 'one':
        s[n // 2] = 7
    elif kind == 'all':
        s[:] = rng.integers(1, 50, size=n)
    elif kind in ('scattered', 'big'):
        m = max(1, n // 97)
        at = rng.choice(n, size=min(n, m), replace=False)
        s[at] = np.arange(1, at.size + 1, dtype=np.uint64) + (np.uint64(1 << 32) if kind == 'big' else np.uint64(0))
    elif kind == 'blobs':
        # every label on two blobs, far apart
        s = s.reshape(shape)
        m = max(1, n // 2000)
        for lab in range(1, m + 1):
            for _ in range(2):
                c = [int(rng.integers(0, d)) for d in shape]
                s[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 3] = lab
        s = s.ravel()
    else:
        raise ValueError(kind)
    return s.reshape(shape).astype(dtype)


def n_segments(labels):
    return int(np.unique(labels[labels != 0]).size)


def load_kats(path):
    import json
    with open(path) as f:
        kats = json.load(f)['cases']
    for c in kats:
        # ("-0", "inf" and "-inf" are strings: JSON has no such numbers)
        c['hmap'] = np.array([float(x) for x in c['hmap']], dtype=np.float32).reshape(c['shape'])
        c['seeds'] = np.array(c['seeds'], dtype=np.uint64).reshape(c['shape'])
        c['labels'] = np.array(c['labels'], dtype=np.uint64).reshape(c['shape'])
    return kats
