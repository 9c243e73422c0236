"""What the thresholded-components tests share (test_cc_host.py,
test_gpu_cc.py, test_gpu_cc_workflow.py): the labelling oracle, a dict
union-find, the golden fixture and the volumes with a known answer.

The oracle is a numpy min-propagation labelling.  Every foreground voxel
starts with its linear index; each sweep replaces it by the minimum over its
connectivity-c neighbourhood (shifted views of a padded array) until nothing
changes, so a voxel ends with the smallest index of its component; ranking the
distinct roots numbers the components 1 .. N in raster order of their first
voxels.  That is scipy.ndimage.label's numbering with
generate_binary_structure(3, c): test_cc_host.py asserts it where scipy is
installed."""
import itertools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def offsets(c):
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(v) for v in d) <= c]


def oracle_label(fg, c):
    """(labels uint64, n) of the boolean volume ``fg`` with connectivity c."""
    fg = np.asarray(fg, dtype=bool)
    big = np.iinfo(np.int64).max
    ids = np.where(fg, np.arange(fg.size, dtype=np.int64).reshape(fg.shape), big)
    nz, ny, nx = fg.shape
    while True:
        pad = np.pad(ids, 1, constant_values=big)
        best = ids
        for dz, dy, dx in offsets(c):
            best = np.minimum(best, pad[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
        best = np.where(fg, best, big)
        if np.array_equal(best, ids):
            break
        ids = best
    roots = np.unique(ids[fg])
    labels = np.zeros(fg.shape, dtype=np.uint64)
    labels[fg] = (np.searchsorted(roots, ids[fg]) + 1).astype(np.uint64)
    return labels, int(roots.size)


def normalize(x):
    """vu.normalize (utils/volume_utils.py:98-105), restated."""
    x = x.astype('float32')
    x -= x.min()
    mx = x.max()
    if mx > 0:
        x /= mx
    return x


def foreground(data, threshold, mode, normalized=True, mask=None):
    v = normalize(data) if normalized else data.astype(np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid='ignore'):
        fg = {'greater': v > t, 'less': v < t, 'equal': v == t}[mode]
    if mask is not None:
        fg = fg & (np.asarray(mask) != 0)
    return fg


def merge_table(pairs, n_labels):
    """(table, max_id) of rag.merge_assignments by a dict union-find: table[0]
    = 0, every other id -> 1 + the rank of its set's smallest member."""
    parent = list(range(n_labels))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in np.asarray(pairs, dtype=np.int64).reshape(-1, 2):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(i) for i in range(n_labels)], dtype=np.int64)
    table = np.searchsorted(np.unique(roots), roots).astype(np.uint64)
    return table, int(table.max()) if n_labels else 0


def merge_table_fast(pairs, n_labels):
    """merge_table for millions of ids: scipy's connected components of the pair
    graph give the sets; each id maps to the rank of its set's smallest member
    ({0} is the set of rank 0, so the others count from 1).
    tests/test_cc_host.py asserts it equal to merge_table."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n_labels, n_labels))
    n_sets, which = connected_components(graph, directed=False)
    smallest = np.full(n_sets, n_labels, dtype=np.int64)
    np.minimum.at(smallest, which, np.arange(n_labels, dtype=np.int64))
    rank = np.empty(n_sets, dtype=np.int64)
    rank[np.argsort(smallest)] = np.arange(n_sets)
    table = rank[which].astype(np.uint64)
    return table, int(table.max()) if n_labels else 0


# The caps past which a loop of ctg_cc.hip takes a second step or turn, mirrored here once;
# tests/test_cc_host.py (test_cap_mirrors) pins each against the plan function or the launch's own text.
SEG = 2048               # csrc/ctg_plan.h: CC_SEG, nodes a numbering segment (cc_segments)
SCAN_STEP = 1024         # csrc/ctg_cc.hip: k_uf_scan, segments a step of its one workgroup (`base += 1024`)
RANGE_ROWS = 4 * 2048    # csrc/ctg_cc.hip: launch_cc_range, 2048 workgroups of 4 waves, a row a wave and turn
BIG = (129, 128, 128)    # 2 113 536 voxels: 1032 segments (two scan steps), 16512 rows (three range turns), 288 tiles


def scan_steps(nodes):
    """Steps of k_uf_scan's loop over the numbering segments of ``nodes`` nodes."""
    return -(-(-(-nodes // SEG)) // SCAN_STEP)


def comb(shape=BIG):
    """The serpentine over the whole box: one path along x on every other row
    of every other plane -- it crosses every x seam on every row it takes and
    climbs through every y and z tile border."""
    return serpentine(shape)


def first_occurrence(labels):
    """The labelling renumbered 1 .. N by first occurrence in raster order, 0 kept."""
    flat = np.asarray(labels).ravel()
    ids, first = np.unique(flat, return_index=True)
    keep = ids != 0
    order = np.argsort(first[keep])
    new = np.zeros(ids.size, dtype=np.uint64)
    new[np.flatnonzero(keep)[order]] = np.arange(1, int(keep.sum()) + 1, dtype=np.uint64)
    return new[np.searchsorted(ids, flat)].reshape(np.shape(labels))


def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'cc_kat.json')) as f:
        g = json.load(f)
    shape = tuple(g['shape'])
    g['values'] = np.array(g['values'], dtype=np.float32).reshape(shape)
    g['normalized'] = np.array(g['normalized'], dtype=np.float32).reshape(shape)
    g['mask'] = np.array(g['mask'], dtype=np.uint8).reshape(shape)
    for case in g['cases']:
        case['labels'] = np.array(case['labels'], dtype=np.uint64).reshape(shape)
    return g


# --------------------------------------------------------------------------- volumes with a known answer
def random_fg(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def checkerboard(shape):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    return (z + y + x) % 2 == 0


def serpentine(shape=(3, 16, 130)):
    """A one-voxel path: along x on every other row of every other plane, the
    rows joined alternately at the two ends, the planes by one voxel below the
    last row's start -- one component (for every connectivity) that crosses
    the tile seams at x = 64, 128 on every row and at y = 8 on the way down."""
    nz, ny, nx = shape
    fg = np.zeros(shape, dtype=bool)
    rows = list(range(0, ny, 2))
    for z in range(0, nz, 2):
        for k, y in enumerate(rows):
            fg[z, y, :] = True
            if k + 1 < len(rows):
                fg[z, y + 1, nx - 1 if k % 2 == 0 else 0] = True
        if z + 2 < nz:
            fg[z + 1, rows[-1], 0] = True
    return fg


def u_shape(shape=(17, 9, 130)):
    """A 'U' lying in raster order: its first voxel sits in the last x tile of
    row 0, runs down that column to the last row, back along the last row into
    the first tile and up the first column to row 1 -- so the component's root
    (its first voxel) is found only across the seams."""
    fg = np.zeros(shape, dtype=bool)
    nz, ny, nx = shape
    fg[0, :, nx - 1] = True
    fg[0, ny - 1, :] = True
    fg[0, 1:, 0] = True
    return fg
