"""Every stream-taking call of include/ctg.h held to its stream, off the null
stream (the "Streams" paragraph of include/ctg.h).

The rest of the suite runs on the null stream, where a kernel, memset or copy
given 0 instead of the call's stream, a blocking hipMemcpy, or a pool block
handed on too early all go unseen.  Here every call runs on a torch side
stream (non-blocking) that is first shown to overlap the null stream, while
the null stream is held busy (tests/stream_cases.py):

Protocol A -- the call stays on its stream.  Per entry point: warm up on a
  *decoy* input (same shape and dtype, another seed) so that the pool and the
  workspace hold decoy-derived data; hold the null stream; stage the true
  input on the side stream behind a short delay (the tensors hold the decoy
  until then); call; read the result as product code does.  The result must be
  the oracle's answer for the true input, the null stream's hold must still be
  pending when the call returns and again after the read (so nothing waited
  for the null stream), and a call documented as synchronised must leave its
  stream idle.  One host-memory case per family passes numpy arrays and an
  explicit ``stream=``.
Protocol B -- two streams, one pool: alternating calls on two side streams,
  and a call on stream B that draws the pool block a distance transform on a
  held stream A used as scratch.
Protocol C -- a consumer queued on the stream of a call that returns with its
  work queued sees the finished output without any host synchronisation.

Every comparison uses the bar its family already has: exact where the family
is exact, check_features / check_stats for the edge statistics, the filters'
tolerance of tests/test_filters.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from cluster_tools_amd import _lib                    # noqa: E402
from cluster_tools_amd import dist as cdist           # noqa: E402
from cluster_tools_amd import fastfilters as F        # noqa: E402
from cluster_tools_amd import rag                     # noqa: E402
from cluster_tools_amd import synthetic as S          # noqa: E402
from oracle import filter_oracle as FO                # noqa: E402
from oracle import rag_oracle as O                    # noqa: E402

import stream_cases as SC                             # noqa: E402
from test_filters import FILTERS                      # noqa: E402
from test_gpu_blocks import _block_geometry, _expected_boundary      # noqa: E402
from test_gpu_filter_edges import assert_filter_close                # noqa: E402
from test_gpu_merge_helpers import _merge_case, _row_counts, check_merged_rows    # noqa: E402
from test_gpu_morphology import check_table as check_morphology      # noqa: E402
from test_gpu_overlaps import check_table as check_overlaps          # noqa: E402
from test_gpu_parity import check_features            # noqa: E402
from test_gpu_region_features import check_exact as check_region, grid_data       # noqa: E402
from test_gpu_stats_exact import check_stats          # noqa: E402
from test_gpu_take import oracle as take_oracle, value_of            # noqa: E402
from test_morphology_host import dense_rows as morph_dense_rows, morph_rows, morph_table   # noqa: E402
from test_overlaps_host import max_overlap, overlap_table            # noqa: E402
from test_region_features_host import (dense_rows as region_dense_rows, feature_rows, region_table,   # noqa: E402
                                       sum_rows)
from tests import cc_cases as C                       # noqa: E402
from tests import edt_cases as E                      # noqa: E402
from tests import exchange_cases as X                 # noqa: E402
from tests.exchange_sim import simulate               # noqa: E402

U64 = np.uint64
SCAN_SHAPE = (9, 37, 70)        # the face scan: off the tile grid on every axis, two tiles along x
DENSE_SHAPE = (5, 33, 129)      # labels from 2^40: the dense re-entry
EDT_SHAPE = (5, 33, 70)         # all three passes; the y pass past one LDS line (E.LDS_LINE = 32)
FILTER_SHAPE = (9, 33, 17)
TABLE_SHAPE = (9, 37, 70)       # overlaps, morphology, region features, components
BIG = U64(1) << U64(40)

# wall time and hold of every case of this process (the `side` fixture prints them on its way out)
TIMES = []


def handle_of(stream):
    return ctypes.c_void_p(stream.cuda_stream)


@pytest.fixture(scope='module')
def side(gpu):
    """The side stream of the file -- shown to overlap the null stream, or the tests fail by naming that.
    On the way out: the measured wall time and hold of the Protocol A cases (run with -s to read it)."""
    yield SC.side_stream()
    if TIMES:
        slow = max(TIMES, key=lambda x: x[1])
        print('\nProtocol A: %d cases, %.1f s in all; slowest %s %.2f s; holds %.0f .. %.0f ms'
              % (len(TIMES), sum(t for _, t, _ in TIMES), slow[0], slow[1], min(m for _, _, m in TIMES),
                 max(m for _, _, m in TIMES)))


# ===========================================================================
# Protocol A
# ===========================================================================
class Case:
    """One entry point under Protocol A.

    inputs(seed)   the numpy arrays that are staged (seed 0: the true input, 1: the decoy)
    call(args, sh) the call on the current stream, whose handle is sh; args: CUDA tensors
                   (device) or the numpy arrays themselves (host)
    read(result)   the result as numpy tables, read the way product code reads it
    check(got, true_arrays)
    synchronised   the call is documented to return with its stream idle"""
    synchronised = True
    host = False

    def read(self, result):
        return result


def clone_to_host(*tensors):
    """Queued-return calls: a clone queued on the current stream, then that stream is waited for."""
    clones = [t.clone() for t in tensors]
    torch.cuda.current_stream().synchronize()
    return [c.cpu().numpy() for c in clones]


def protocol_a(case, side):
    import time
    t_start = time.perf_counter()
    s, sh = side, handle_of(side)
    decoy, true = case.inputs(1), case.inputs(0)

    def once(args):
        with torch.cuda.stream(s):
            return case.read(case.call(args, sh))

    # 1. warm-up on the decoy, on the side stream: once for the kernels' code, once timed on the idle device
    args = decoy if case.host else SC.to_device(decoy, s)
    once(args)
    _, seconds = SC.timed(lambda: once(args))
    ms = SC.hold_ms_for(seconds)
    print('%s: the call takes %.2f ms on the idle device, the null stream is held for %.0f ms'
          % (type(case).__name__, seconds * 1e3, ms))
    # 2. - 5.
    with SC.null_busy(ms) as nb:
        args = true if case.host else SC.staged(decoy, true, s)
        with torch.cuda.stream(s):
            result = case.call(args, sh)
            pending_after_call = nb.still_pending()
            idle_after_call = s.query()
            got = case.read(result)
        pending_after_read = nb.still_pending()
    TIMES.append((type(case).__name__ + ('[host]' if case.host else ''), time.perf_counter() - t_start, ms))
    assert pending_after_call, ('the null stream\'s hold of %.0f ms was over when the call returned: the call '
                                'waited for the null stream, or the hold was too short' % ms)
    if case.synchronised:
        assert idle_after_call, 'a call documented as synchronised returned with work queued on its stream'
    assert pending_after_read, ('the null stream\'s hold of %.0f ms was over once the result was read: an accessor '
                                'waited for the null stream' % ms)
    case.check(got, true)


# ----------------------------------------------------------------- face scan
def scan_volume(shape, seed, cell=4):
    return S.generate(shape, cell=cell, seed=40 + seed)


class FaceScan(Case):
    """rag_features_handle: kind in graph / f32 / u8 / nn / lr / keep_stats / dense"""

    def __init__(self, kind, host=False):
        self.kind, self.host = kind, host
        self.offsets = {'nn': S.NN_OFFSETS, 'lr': S.LR_OFFSETS}.get(kind)
        self.keep = kind == 'keep_stats'
        self.shape = DENSE_SHAPE if kind == 'dense' else SCAN_SHAPE

    def inputs(self, seed):
        lab, bnd = scan_volume(self.shape, seed)
        if self.kind == 'graph':
            return [lab]
        if self.kind == 'dense':
            return [lab + BIG, bnd]
        if self.kind == 'u8':
            return [lab, np.clip(np.rint(bnd * 255.0), 0, 255).astype(np.uint8)]
        if self.offsets is not None:
            return [lab, S.affinities_from_boundary(bnd, self.offsets)]
        return [lab, bnd]

    def call(self, args, sh):
        data = args[1] if len(args) > 1 else None
        return rag.rag_features_handle(args[0], data, offsets=self.offsets, keep_stats=self.keep, stream=sh)

    def read(self, r):
        out = dict(edges=r.edges(), nodes=r.nodes())
        if self.kind != 'graph':
            out['features'] = r.features()
        if self.keep:
            out['sums'], out['records'] = r.stats()
        r.free()
        return out

    def check(self, got, true):
        lab = true[0]
        np.testing.assert_array_equal(got['nodes'], O.unique_labels(lab))
        if self.kind == 'graph':
            np.testing.assert_array_equal(got['edges'], O.rag_edges(lab))
            return
        if self.offsets is not None:
            e_ref, f_ref = O.affinity_features(lab, true[1], self.offsets)
        else:
            e_ref, f_ref, stats = O.boundary_features(lab, true[1], return_stats=True)
        np.testing.assert_array_equal(got['edges'], e_ref)
        check_features(got['features'], f_ref)
        if self.keep:
            check_stats(got, stats)


class SingleLabel(Case):
    """uint32 labels, one label: the node is widened after the reduce (widen_single_label)"""

    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return [np.full((5, 9, 70), 7 + 2 * seed, dtype=np.uint32)]

    def call(self, args, sh):
        return rag.rag_features_handle(args[0], stream=sh)

    def read(self, r):
        out = dict(edges=r.edges(), nodes=r.nodes())
        r.free()
        return out

    def check(self, got, true):
        assert got['edges'].shape == (0, 2)
        np.testing.assert_array_equal(got['nodes'], [int(true[0][0, 0, 0])])


class Blocks(Case):
    """rag_blocks_arena, two blocks with boundary features, the arenas on the device"""
    SHAPE, BLOCK = (9, 20, 70), (9, 20, 35)

    def __init__(self, host=False, front_end=False):
        self.host, self.front_end = host, front_end       # front_end: rag.rag_blocks (numpy arrays per block)
        self.geo = _block_geometry(self.SHAPE, self.BLOCK)
        assert len(self.geo) == 2

    def volume(self, seed):
        return scan_volume(self.SHAPE, 10 + seed)

    def inputs(self, seed):
        lab, bnd = self.volume(seed)
        return [np.concatenate([lab[g['roi']].ravel() for g in self.geo]),
                np.concatenate([bnd[g['roi']].ravel() for g in self.geo])]

    def call(self, args, sh):
        blocks, off = [], 0
        if self.front_end:
            shapes = [tuple(b - a for a, b in zip(g['rb'], g['re'])) for g in self.geo]
            cuts = np.cumsum([0] + [int(np.prod(sh_)) for sh_ in shapes])
            per = [[a[cuts[i]:cuts[i + 1]].reshape(shapes[i]) for i in range(len(shapes))] for a in args]
            return rag.rag_blocks(per[0], [g['own'] for g in self.geo], [g['graph'] for g in self.geo], data=per[1],
                                  stream=sh)
        for g in self.geo:
            shape = tuple(b - a for a, b in zip(g['rb'], g['re']))
            blocks.append(dict(label_offset=off, data_offset=off, shape=shape, own=g['own'], graph=g['graph']))
            off += int(np.prod(shape))
        return rag.rag_blocks_arena(args[0], blocks, args[1], stream=sh)

    def check(self, got, true):
        lab, bnd = self.volume(0)
        assert len(got) == 2
        for g, r in zip(self.geo, got):
            e_ref, f_ref = _expected_boundary(lab, bnd, g)
            np.testing.assert_array_equal(r['nodes'], np.unique(lab[g['inner']]))
            np.testing.assert_array_equal(r['edges'], e_ref)
            check_features(r['features'], f_ref)


# --------------------------------------------------------------- small calls
class UniqueLabels(Case):
    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return [scan_volume(SCAN_SHAPE, seed)[0]]

    def call(self, args, sh):
        return rag.unique_labels(args[0], stream=sh)

    def check(self, got, true):
        np.testing.assert_array_equal(got, np.unique(true[0]))


class UniqueValues(Case):
    def inputs(self, seed):
        rng = np.random.default_rng(60 + seed)
        pool = rng.integers(0, (1 << 64) - 1, size=1500, dtype=np.uint64, endpoint=True)
        return [pool[rng.integers(0, pool.size, size=4097)]]

    def call(self, args, sh):
        return rag.unique_values_handle(args[0], stream=sh)

    def read(self, r):
        out = r.nodes()
        r.free()
        return out

    def check(self, got, true):
        np.testing.assert_array_equal(got, np.unique(true[0]))


def pair_list(seed, n=3000, top=900):
    rng = np.random.default_rng(70 + seed)
    p = np.sort(rng.integers(1, top, size=(n, 2)), axis=1).astype(np.uint64)
    p[:, 1] += U64(1)                                # u < v
    return p


class UniquePairs(Case):
    host = True

    def inputs(self, seed):
        return [pair_list(seed)]

    def call(self, args, sh):
        return rag.unique_pairs(args[0], stream=sh)

    def check(self, got, true):
        np.testing.assert_array_equal(got[0], np.unique(true[0], axis=0))
        np.testing.assert_array_equal(got[1], np.unique(true[0]))


def lookup_inputs(seed):
    """A sorted unique edge table of 1000 rows and 512 queries, half of them rows of it."""
    rng = np.random.default_rng(80 + seed)
    t = np.unique(pair_list(100 + seed, 6000, 300), axis=0)
    assert t.shape[0] >= 1000
    t = t[:1000]
    q = np.concatenate([t[rng.integers(0, 1000, size=256)], pair_list(200 + seed, 256, 300)])
    return [t, q[rng.permutation(512)]]


class MapEdgeIdsHost(Case):
    host = True

    def inputs(self, seed):
        return lookup_inputs(seed)

    def call(self, args, sh):
        return rag.map_edge_ids(args[0], args[1], stream=sh)

    def check(self, got, true):
        ref = O.find_edges(true[0], true[1])
        assert (ref >= 0).sum() >= 256 and (ref < 0).sum() > 10
        np.testing.assert_array_equal(got, ref)


def map_edge_ids_device(table, query, sh):
    """ctg_map_edge_ids with CTG_MEM_DEVICE (no wrapper reaches it): returns with the kernel queued."""
    out = torch.full((query.shape[0],), -7, dtype=torch.int64, device='cuda')
    rc = _lib.load().ctg_map_edge_ids(ctypes.c_void_p(table.data_ptr()), table.shape[0],
                                      ctypes.c_void_p(query.data_ptr()), query.shape[0],
                                      ctypes.c_void_p(out.data_ptr()), _lib.CTG_MEM_DEVICE, sh)
    _lib.check(rc, 'ctg_map_edge_ids')
    return out


class MapEdgeIdsDevice(MapEdgeIdsHost):
    host = False
    synchronised = False

    def call(self, args, sh):
        return map_edge_ids_device(args[0], args[1], sh)

    def read(self, out):
        return clone_to_host(out)[0]


class MergeStats(Case):
    """ctg_merge_stats over two z-slabs' rows: the whole volume's statistics.  The decoy keeps the keys
    and takes every row's statistics from the row before it."""
    SHAPE = (12, 37, 44)

    def __init__(self, host=False):
        self.host = host
        self.lab, self.bnd = S.generate(self.SHAPE, cell=5, seed=14)
        self.rows = None

    def inputs(self, seed):
        if self.rows is None:       # (the slabs' rows come from the library, on the idle device)
            a = rag.rag_features(self.lab[:7], self.bnd[:7], keep_stats=True)
            b = rag.rag_features(self.lab[6:], self.bnd[6:], own_begin=(1, 0, 0), keep_stats=True)
            self.rows = [np.concatenate([a[k], b[k]]) for k in ('edges', 'sums', 'records')]
        keys, sums, rec = self.rows
        return [keys, np.roll(sums, seed, axis=0), np.roll(rec, seed, axis=0)]

    def call(self, args, sh):
        return rag.merge_stats_handle(args[0], args[1], args[2], keep_stats=True, stream=sh)

    def read(self, r):
        out = dict(edges=r.edges(), features=r.features())
        out['sums'], out['records'] = r.stats()
        r.free()
        return out

    def check(self, got, true):
        e_ref, f_ref, stats = O.boundary_features(self.lab, self.bnd, return_stats=True)
        np.testing.assert_array_equal(got['edges'], e_ref)
        check_stats(got, stats)
        check_features(got['features'], f_ref)


class MergeFeatureRows(Case):
    host = True
    E, ID0 = 257, 1000003

    def inputs(self, seed):
        ids, rows = _merge_case(self.E, self.ID0, 90 + seed, _row_counts(self.E, self.E))
        return [ids, rows]

    def call(self, args, sh):
        return rag.merge_feature_rows(args[0], args[1], self.ID0, self.ID0 + self.E, stream=sh)

    def check(self, got, true):
        check_merged_rows(got, true[0], true[1], self.ID0, self.ID0 + self.E)


# ------------------------------------------------------------------ overlaps
def two_labellings(seed):
    a = S.generate(TABLE_SHAPE, cell=4, seed=110 + seed, with_boundary=False)[0]
    b = S.generate(TABLE_SHAPE, cell=9, seed=120 + seed, with_boundary=False)[0]
    return a, b


class LabelOverlaps(Case):
    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return list(two_labellings(seed))

    def call(self, args, sh):
        return rag.label_overlaps_handle(args[0], args[1], stream=sh)

    def read(self, r):
        out = rag._overlap_tables(r)
        r.free()
        return out

    def check(self, got, true):
        check_overlaps(got, true[0], true[1])


def partial_overlaps(seed):
    """The overlap tables of two z-slabs, concatenated."""
    a, b = two_labellings(seed)
    parts = [overlap_table(a[:4], b[:4]), overlap_table(a[4:], b[4:])]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


class MergeOverlaps(Case):
    """The decoy keeps the pairs and takes every row's count from the row before it."""

    def inputs(self, seed):
        pairs, counts = partial_overlaps(0)
        return [pairs, np.roll(counts, seed)]

    def call(self, args, sh):
        return rag.merge_overlaps_handle(args[0], args[1], stream=sh)

    def read(self, r):
        out = rag._overlap_tables(r)
        r.free()
        return out

    def check(self, got, true):
        a, b = two_labellings(0)
        check_overlaps(got, a, b)


class MaxOverlaps(Case):
    """ctg_max_overlaps reads a handle: the table is merged on the stream, then the arg-max."""
    LB = 3

    def inputs(self, seed):
        pairs, counts = partial_overlaps(0)
        return [pairs, np.roll(counts, seed)]

    def call(self, args, sh):
        r = rag.merge_overlaps_handle(args[0], args[1], stream=sh)
        le = int(np.prod([(n + 3) // 4 for n in TABLE_SHAPE])) + 5      # past the largest label: rows of zeros
        out = rag.max_overlaps(r, self.LB, le, stream=sh)
        r.free()
        return out

    def check(self, got, true):
        a, b = two_labellings(0)
        pairs, counts = overlap_table(a, b)
        lab, cnt, tie = max_overlap(pairs, counts, self.LB, self.LB + got[0].shape[0])
        assert (cnt > 0).sum() > 100 and (cnt == 0).any()
        np.testing.assert_array_equal(got[1], cnt)
        np.testing.assert_array_equal(got[0], lab)      # (equal counts go to the smallest value, the oracle's rule too)


# ---------------------------------------------------------------- morphology
def fit_rows(rows, n):
    """rows cut or padded with zero rows (absent labels: they add nothing) to n rows"""
    out = np.zeros((n, rows.shape[1]), rows.dtype)
    k = min(n, rows.shape[0])
    out[:k] = rows[:k]
    return out


class Morphology(Case):
    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return [two_labellings(seed)[0]]

    def call(self, args, sh):
        return rag.morphology_handle(args[0], stream=sh)

    def read(self, r):
        out = rag._morphology_tables(r)
        r.free()
        return out

    def check(self, got, true):
        check_morphology(got, true[0])


def partial_morphology(seed):
    a = two_labellings(seed)[0]
    return np.concatenate([morph_rows(*morph_table(a[:4])), morph_rows(*morph_table(a[4:], (4, 0, 0)))])


class MergeMorphology(Case):
    def inputs(self, seed):
        true = partial_morphology(0)
        return [true if seed == 0 else fit_rows(partial_morphology(seed), true.shape[0])]

    def call(self, args, sh):
        return rag.merge_morphology_handle(args[0], stream=sh)

    def read(self, r):
        out = rag._morphology_tables(r)
        r.free()
        return out

    def check(self, got, true):
        check_morphology(got, two_labellings(0)[0])


class MorphologyRows(MergeMorphology):
    """ctg_morphology_rows' dense table over a label range, from a handle"""
    LB, LE = 5, 300

    def call(self, args, sh):
        r = rag.merge_morphology_handle(args[0], stream=sh)
        out = rag.morphology_rows(r, self.LB, self.LE, stream=sh)
        r.free()
        return out

    def read(self, out):
        return out

    def check(self, got, true):
        nodes, mom = morph_table(two_labellings(0)[0])
        assert int(nodes.max()) > self.LE > int(nodes.min())
        np.testing.assert_array_equal(got, morph_dense_rows(morph_rows(nodes, mom), self.LB, self.LE))


# ----------------------------------------------------------- region features
def region_inputs(seed):
    return two_labellings(seed)[0], grid_data(TABLE_SHAPE, 130 + seed)


class RegionFeatures(Case):
    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return list(region_inputs(seed))

    def call(self, args, sh):
        return rag.region_features_handle(args[0], args[1], stream=sh)

    def read(self, r):
        out = rag._region_tables(r, 1.0)
        r.free()
        return out

    def check(self, got, true):
        check_region(got, true[0], true[1])


def partial_region(seed):
    a, d = region_inputs(seed)
    return np.concatenate([sum_rows(region_table(a[:4], d[:4])), sum_rows(region_table(a[4:], d[4:]))])


class MergeRegionFeatures(Case):
    def inputs(self, seed):
        true = partial_region(0)
        return [true if seed == 0 else fit_rows(partial_region(seed), true.shape[0])]

    def call(self, args, sh):
        return rag.merge_region_features_handle(args[0], stream=sh)

    def read(self, r):
        out = rag._region_tables(r, 1.0)
        r.free()
        return out

    def check(self, got, true):
        check_region(got, *region_inputs(0))       # (k / 256 samples: exactly summable, every order the same bits)


class RegionFeatureRows(MergeRegionFeatures):
    LB, LE, NORM = 5, 300, 2.0

    def call(self, args, sh):
        r = rag.merge_region_features_handle(args[0], stream=sh)
        out = rag.region_feature_rows(r, self.LB, self.LE, 'features', self.NORM, stream=sh)
        r.free()
        return out

    def read(self, out):
        return out

    def check(self, got, true):
        t = region_table(*region_inputs(0))
        assert int(t['nodes'].max()) > self.LE > int(t['nodes'].min())
        np.testing.assert_array_equal(got, region_dense_rows(feature_rows(t, self.NORM), self.LB, self.LE))


# --------------------------------------------------------------------- write
N_TABLE = 5000


def take_labels():
    lab = np.random.default_rng(140).integers(0, N_TABLE, size=(3, 41, 70)).astype(np.uint64)
    lab[0, :3] = 0
    return lab


class AssignmentDense(Case):
    """The handle holds a copy of the table: it is read by applying it to fixed labels."""

    def __init__(self, host=False):
        self.host = host
        self.labels = take_labels()

    def inputs(self, seed):
        return [value_of(np.arange(N_TABLE) + 7919 * seed)]

    def oracle_kw(self, true):
        return dict(table=true[0])

    def call(self, args, sh):
        return rag.assignment_dense(args[0], stream=sh)

    def read(self, a):
        out, info = rag.apply_assignment(a, self.labels, stream=handle_of(torch.cuda.current_stream()))
        a.free()
        return out, info

    def check(self, got, true):
        want, nz, n_missing, first = take_oracle(self.labels, **self.oracle_kw(true))
        np.testing.assert_array_equal(np.asarray(got[0]).reshape(-1).view(np.uint64), want)
        np.testing.assert_array_equal(got[1]['nonzero'], nz)
        assert (got[1]['n_missing'], got[1]['first_missing']) == (n_missing, first) == (0, None)


class AssignmentSparse(AssignmentDense):
    def inputs(self, seed):
        keys = np.random.default_rng(150).permutation(N_TABLE).astype(np.uint64)
        return [keys, value_of(keys + U64(7919 * seed))]

    def oracle_kw(self, true):
        return dict(keys=true[0], values=true[1])

    def call(self, args, sh):
        return rag.assignment_sparse(args[0], args[1], stream=sh)


class ApplyAssignment(AssignmentDense):
    """ctg_apply_assignment on staged labels, into a new array or in place"""

    def __init__(self, in_place=False, host=False):
        self.in_place, self.host = in_place, host
        self.table = value_of(np.arange(N_TABLE))
        self.a = None

    def inputs(self, seed):
        lab = np.random.default_rng(160 + seed).integers(0, N_TABLE, size=(3, 41, 70)).astype(np.uint64)
        lab[0, :3] = 0
        return [lab]

    def call(self, args, sh):
        if self.a is None:
            self.a = rag.assignment_dense(self.table, stream=sh)
        labels = args[0]
        if self.in_place:       # (a copy, queued behind the staging: the inputs serve more than one call)
            labels = labels.copy() if self.host else labels.clone()
        return rag.apply_assignment(self.a, labels, out=labels if self.in_place else None, stream=sh)

    def read(self, result):
        out, info = result
        return (out.cpu().numpy() if torch.is_tensor(out) else out), info

    def check(self, got, true):
        self.labels = true[0]
        AssignmentDense.check(self, got, [self.table])
        self.a.free()
        self.a = None


# ---------------------------------------------------------------- components
class ThresholdComponents(Case):
    """normalised, so k_cc_range runs in front of the tiles"""
    THRESHOLD = 0.9         # a tenth of the voxels: hundreds of small components

    def __init__(self, host=False):
        self.host = host

    def inputs(self, seed):
        return [np.random.default_rng(170 + seed).random(TABLE_SHAPE).astype(np.float32)]

    def call(self, args, sh):
        return rag.threshold_components(args[0], self.THRESHOLD, normalize=True, connectivity=3, stream=sh)

    def read(self, result):
        out, n = result
        return (out.cpu().numpy().view(np.uint64) if torch.is_tensor(out) else out), n

    def check(self, got, true):
        want, n = C.oracle_label(C.foreground(true[0], self.THRESHOLD, 'greater', normalized=True), 3)
        assert n > 10 and got[1] == n
        np.testing.assert_array_equal(got[0], want)


class MergeAssignments(Case):
    N = 5000

    def inputs(self, seed):
        return [np.random.default_rng(180 + seed).integers(1, self.N, size=(2500, 2)).astype(np.uint64)]

    def call(self, args, sh):
        return rag.merge_assignments(args[0], self.N, stream=sh)

    def read(self, result):
        table, max_id = result
        return (table.cpu().numpy().view(np.uint64) if torch.is_tensor(table) else table), max_id

    def check(self, got, true):
        want, max_id = C.merge_table(true[0], self.N)
        assert got[1] == max_id
        np.testing.assert_array_equal(got[0], want)


# -------------------------------------------------------- distance transform
def edt_seeds(seed):
    return E.case(EDT_SHAPE, 'random_0.02' if seed == 0 else 'random_0.3', None)


def edt_without_info(src, out, sh):
    """ctg_distance_transform on device memory with info = NULL, which no wrapper passes"""
    shape = (ctypes.c_int64 * 3)(*src.shape)
    rc = _lib.load().ctg_distance_transform(ctypes.c_void_p(src.data_ptr()), _lib.CTG_EDT_SRC_NONZERO, 8, shape, None,
                                            None, 0.0, 0, None, 0, ctypes.c_void_p(out.data_ptr()),
                                            _lib.CTG_MEM_DEVICE, sh, None)
    _lib.check(rc, 'ctg_distance_transform')


class DistanceTransform(Case):
    def __init__(self, info=True, host=False):
        self.info, self.host = info, host

    def inputs(self, seed):
        return [np.ascontiguousarray(edt_seeds(seed)[0]).astype(np.uint8)]

    def call(self, args, sh):
        if self.info:
            return rag.distance_transform(args[0], stream=sh)
        out = torch.empty(EDT_SHAPE, dtype=torch.float32, device='cuda')
        edt_without_info(args[0], out, sh)
        return out, None

    def read(self, result):
        dist, info = result
        return (clone_to_host(dist)[0] if torch.is_tensor(dist) else dist), info

    def check(self, got, true):
        seeds, d2 = edt_seeds(0)
        if self.info:
            E.check(got[0], got[1], seeds, None, False, d2)
        else:
            np.testing.assert_array_equal(got[0].view(np.uint32), E.expected(d2, seeds)[0].view(np.uint32))


# ------------------------------------------------------------------- filters
class Filter(Case):
    """A filter of fastfilters on a tensor: every launch on the current stream, returned with its work queued"""
    synchronised = False

    def __init__(self, name, host=False):
        self.name, self.host = name, host
        self.synchronised = host        # numpy in, numpy out: the copy back is waited for

    def inputs(self, seed):
        return [np.random.default_rng(190 + seed).random(FILTER_SHAPE).astype(np.float32)]

    def call(self, args, sh):
        return getattr(F, self.name)(args[0], 1.0)

    def read(self, out):
        return clone_to_host(out)[0] if torch.is_tensor(out) else out

    def check(self, got, true):
        assert_filter_close(got, getattr(FO, self.name)(true[0].astype(np.float64), 1.0))


# ------------------------------------------------------------ synthetic data
class SynthVolume(Case):
    """No input to stage: the seed is the input, the decoy another seed (the warm-up's output is what
    torch's allocator hands back for the outputs)."""
    synchronised = False
    host = True
    SHAPE = (9, 33, 70)

    def inputs(self, seed):
        return [200 + seed]

    def call(self, args, sh):
        return rag.synth_volume(self.SHAPE, cell=5, seed=args[0])

    def read(self, result):
        lab, bnd = clone_to_host(*result)
        return lab.view(np.uint64), bnd

    def check(self, got, true):
        lab, bnd = S.generate(self.SHAPE, cell=5, seed=200)
        np.testing.assert_array_equal(got[0], lab)
        np.testing.assert_array_equal(got[1], bnd)


class SynthAffinities(Case):
    synchronised = False

    def inputs(self, seed):
        return [scan_volume(SCAN_SHAPE, seed)[1]]

    def call(self, args, sh):
        return rag.synth_affinities(args[0], S.LR_OFFSETS)

    def read(self, out):
        return clone_to_host(out)[0]

    def check(self, got, true):
        np.testing.assert_array_equal(got, S.affinities_from_boundary(true[0], S.LR_OFFSETS))


# ------------------------------------------------------------------ exchange
class Exchange(Case):
    """Two ranks of one exchange case through tests/exchange_sim.py: the local calls, sample, split,
    pack and merge, all on the stream the backend takes once (dist.py: the call's stream)."""

    def inputs(self, seed):
        name = 'columns' if seed == 0 else 'reversed'
        return [np.array(X.case(name).labels), np.array(X.case_data(name))]

    def call(self, args, sh):
        return simulate(cdist.HipBackend(defer_stats=False), args[0], args[1], 2)

    def read(self, shards):
        try:
            return (np.concatenate([x.edges() for x in shards]), np.concatenate([x.features() for x in shards]),
                    np.concatenate([x.nodes() for x in shards]))
        finally:
            for x in shards:
                x.free()

    def check(self, got, true):
        e_ref, f_ref = O.boundary_features(true[0], true[1])
        np.testing.assert_array_equal(got[0], e_ref)
        check_features(got[1], f_ref)
        np.testing.assert_array_equal(got[2], O.unique_labels(true[0]))


DEVICE_CASES = [
    ('scan_graph', lambda: FaceScan('graph')), ('scan_f32', lambda: FaceScan('f32')),
    ('scan_u8', lambda: FaceScan('u8')), ('scan_nn_offsets', lambda: FaceScan('nn')),
    ('scan_lr_offsets', lambda: FaceScan('lr')), ('scan_keep_stats', lambda: FaceScan('keep_stats')),
    ('scan_dense_reentry', lambda: FaceScan('dense')), ('scan_single_label_u32', SingleLabel),
    ('rag_blocks', Blocks),
    ('unique_labels', UniqueLabels), ('unique_values', UniqueValues), ('map_edge_ids_device', MapEdgeIdsDevice),
    ('merge_stats', MergeStats),
    ('label_overlaps', LabelOverlaps), ('merge_overlaps', MergeOverlaps), ('max_overlaps', MaxOverlaps),
    ('morphology', Morphology), ('merge_morphology', MergeMorphology), ('morphology_rows', MorphologyRows),
    ('region_features', RegionFeatures), ('merge_region_features', MergeRegionFeatures),
    ('region_feature_rows', RegionFeatureRows),
    ('assignment_dense', AssignmentDense), ('assignment_sparse', AssignmentSparse),
    ('apply_assignment', ApplyAssignment), ('apply_assignment_in_place', lambda: ApplyAssignment(in_place=True)),
    ('threshold_components', ThresholdComponents), ('merge_assignments', MergeAssignments),
    ('distance_transform', DistanceTransform), ('distance_transform_no_info', lambda: DistanceTransform(info=False)),
] + [('filter_' + n, (lambda n=n: Filter(n))) for n in FILTERS] + [
    ('synth_volume', SynthVolume), ('synth_affinities', SynthAffinities),
    ('exchange', Exchange),
]

# numpy inputs and an explicit stream: one per family, and the wrappers that take host memory only.  The
# dense re-entry and the single-label fix have a host path like any face scan (the volumes are staged, then
# the same code runs).  Two families have none: the exchange steps (ctg_mgpu_*) and the synthetic-data calls
# take device memory only.
HOST_CASES = [
    ('scan_f32', lambda: FaceScan('f32', host=True)), ('scan_dense_reentry', lambda: FaceScan('dense', host=True)),
    ('scan_single_label_u32', lambda: SingleLabel(host=True)),
    ('rag_blocks_arena', lambda: Blocks(host=True)), ('rag_blocks', lambda: Blocks(host=True, front_end=True)),
    ('unique_labels', lambda: UniqueLabels(host=True)), ('unique_pairs', UniquePairs),
    ('map_edge_ids_host', MapEdgeIdsHost), ('merge_stats', lambda: MergeStats(host=True)),
    ('merge_feature_rows', MergeFeatureRows),
    ('label_overlaps', lambda: LabelOverlaps(host=True)), ('morphology', lambda: Morphology(host=True)),
    ('region_features', lambda: RegionFeatures(host=True)),
    ('assignment_dense', lambda: AssignmentDense(host=True)),
    ('apply_assignment_in_place', lambda: ApplyAssignment(in_place=True, host=True)),
    ('threshold_components', lambda: ThresholdComponents(host=True)),
    ('distance_transform', lambda: DistanceTransform(host=True)),
    ('filter_gaussianSmoothing', lambda: Filter('gaussianSmoothing', host=True)),
]


@pytest.mark.parametrize('name,make', DEVICE_CASES, ids=[n for n, _ in DEVICE_CASES])
def test_call_stays_on_its_stream(side, name, make):
    protocol_a(make(), side)


@pytest.mark.parametrize('name,make', HOST_CASES, ids=[n for n, _ in HOST_CASES])
def test_host_memory_call_stays_on_its_stream(side, name, make):
    protocol_a(make(), side)


# ===========================================================================
# Protocol B: two streams, one pool
# ===========================================================================
def test_alternating_calls_on_two_streams(side):
    """region_features on stream A and label_overlaps on stream B, six calls whose inputs change
    every time: the pool hands the blocks of one call to the next, on the other stream."""
    rag.trim_cache()
    a, b = side, SC.second_stream(side)
    live = []
    for k in range(6):
        if k % 2 == 0:
            lab, data = region_inputs(10 + k)
            with torch.cuda.stream(a):
                lt, dt = SC.to_device([lab, data], a)
                r = rag.region_features_handle(lt, dt, stream=handle_of(a))
                live.append((r, lambda r=r: rag._region_tables(r, 1.0), lambda got, lab=lab, data=data:
                             check_region(got, lab, data)))
        else:
            u, v = two_labellings(10 + k)
            with torch.cuda.stream(b):
                ut, vt = SC.to_device([u, v], b)
                r = rag.label_overlaps_handle(ut, vt, stream=handle_of(b))
                live.append((r, lambda r=r: rag._overlap_tables(r), lambda got, u=u, v=v: check_overlaps(got, u, v)))
        if len(live) > 2:                      # two handles stay live: their blocks must survive the later calls
            r, read, check = live.pop(0)
            got = read()
            r.free()
            check(got)
    for r, read, check in live:
        got = read()
        r.free()
        check(got)


def test_a_block_of_a_queued_call_is_not_handed_on(side):
    """A distance transform without info on a held stream A, then unique_values on stream B whose node
    table is of the size class of the transform's x-pass scratch (V uint16 distances; the pool was
    trimmed, so that block is the one the table draws if it is back in the pool).  B's table must not
    change once A's work runs, and A's output is the oracle's.  ctg_distance_transform therefore returns
    only once its stream is idle (csrc/ctg_api_edt.hip: EdtScratch)."""
    import time
    a, b = side, SC.second_stream(side)
    V = int(np.prod(EDT_SHAPE))
    n = V // 4
    assert SC.same_block_class(V * 2, n * 8), 'the node table would not draw the x pass\'s block'
    seeds, d2 = edt_seeds(0)
    src = SC.to_device([np.ascontiguousarray(seeds).astype(np.uint8)], a)[0]
    out = torch.empty(EDT_SHAPE, dtype=torch.float32, device='cuda')
    values = np.random.default_rng(5).integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)
    vt = SC.to_device([values], b)[0]
    torch.cuda.synchronize()
    rag.trim_cache()
    ms = SC.HOLD_MIN_MS
    SC.hold(a, ms)                                                  # 1.
    t0 = time.perf_counter()
    edt_without_info(src, out, handle_of(a))                        # 2.
    waited = (time.perf_counter() - t0) * 1e3
    print('ctg_distance_transform without info returned after %.1f ms of a %.0f ms hold on its stream' % (waited, ms))
    with torch.cuda.stream(b):                                      # 3.
        r = rag.unique_values_handle(vt, stream=handle_of(b))
        first = r.nodes()                                           # 4.
    a.synchronize()                                                 # 5.
    second = r.nodes()                                              # 6.
    r.free()
    np.testing.assert_array_equal(first, np.unique(values))
    np.testing.assert_array_equal(second, first)
    with torch.cuda.stream(a):                                      # 7.
        got = out.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), E.expected(d2, seeds)[0].view(np.uint32))
    assert a.query() and waited >= 0.5 * ms, 'documented as synchronised: it returns once its stream is idle'


# ===========================================================================
# Protocol C: consumers on the stream of a queued-return call
# ===========================================================================
def queued_calls():
    lab, bnd = scan_volume(SCAN_SHAPE, 0)
    table, query = lookup_inputs(0)
    img = np.random.default_rng(190).random(FILTER_SHAPE).astype(np.float32)
    return [
        ('map_edge_ids_device', [table, query], lambda t, sh: map_edge_ids_device(t[0], t[1], sh),
         lambda got: np.testing.assert_array_equal(got, O.find_edges(table, query))),
        ('synth_affinities', [bnd], lambda t, sh: rag.synth_affinities(t[0], S.NN_OFFSETS),
         lambda got: np.testing.assert_array_equal(got, S.affinities_from_boundary(bnd, S.NN_OFFSETS))),
        ('synth_volume', [], lambda t, sh: rag.synth_volume(SCAN_SHAPE, cell=4, seed=40)[0],
         lambda got: np.testing.assert_array_equal(got.view(np.uint64), lab)),
        # ctg_filter_conv_axis and ctg_sym_eigenvalues
        ('filter', [img], lambda t, sh: F.hessianOfGaussianEigenvalues(t[0], 1.0),
         lambda got: assert_filter_close(got, FO.hessianOfGaussianEigenvalues(img.astype(np.float64), 1.0))),
        # ctg_filter_conv_axis and ctg_filter_combine
        ('filter_combine', [img], lambda t, sh: F.gaussianGradientMagnitude(t[0], 1.0),
         lambda got: assert_filter_close(got, FO.gaussianGradientMagnitude(img.astype(np.float64), 1.0))),
    ]


QUEUED = ['map_edge_ids_device', 'synth_affinities', 'synth_volume', 'filter', 'filter_combine']


@pytest.mark.parametrize('k', range(len(QUEUED)), ids=QUEUED)
def test_consumer_on_the_stream_sees_the_output(side, k):
    """The call is queued behind a hold on its stream, a consumer (a clone) behind the call, and nothing
    is waited for in between: the consumer's copy is the finished output."""
    name, arrays, call, check = queued_calls()[k]
    s, sh = side, handle_of(side)
    tensors = SC.to_device(arrays, s)
    with torch.cuda.stream(s):
        call(tensors, sh)                                            # (the kernels' code)
    torch.cuda.synchronize()
    SC.hold(s, SC.HOLD_MIN_MS)
    with torch.cuda.stream(s):
        out = call(tensors, sh)
        consumer = out.clone()
        queued = not s.query()
    assert queued, 'the hold on the stream was over before the consumer was queued: nothing was shown'
    s.synchronize()
    check(consumer.cpu().numpy())


def test_consumers_behind_sample_split_and_pack(side):
    """ctg_mgpu_sample, ctg_mgpu_split and ctg_mgpu_pack of two ranks, queued behind a hold on their
    stream.  The consumers are the exchange's own: torch.stack of the samples into split, and (after the
    one host read the exchange needs, the count matrix) the slices and torch.cat of the send buffers into
    merge.  Nothing is waited for between a step and its consumer; the shards are the oracle's table."""
    s = side
    lab, data = np.array(X.case('columns').labels), np.array(X.case_data('columns'))
    world, Z = 2, lab.shape[0]
    be = cdist.HipBackend(defer_stats=False)
    locs, shards = [], []
    try:
        with torch.cuda.stream(s):
            lt, dt = SC.to_device([lab, data], s)
            for r in range(world):
                rd, own, end = cdist.slab_plan(Z, world, r, None)
                locs.append(be.local(lt[rd:end].contiguous(), dt[rd:end].contiguous(), None, (own - rd, 0, 0), None,
                                     False, (0.0, 1.0)))
            be.split(locs[0], torch.stack([be.sample(x) for x in locs]), world)      # (the kernels' code)
        torch.cuda.synchronize()
        SC.hold(s, SC.HOLD_MIN_MS)
        with torch.cuda.stream(s):
            meta_all = torch.stack([be.sample(x) for x in locs])
            counts = torch.stack([be.split(x, meta_all, world) for x in locs])
            queued = not s.query()
            counts_all = counts.cpu().numpy()
        assert queued, 'the hold was over before split was queued behind sample: nothing was shown'
        words = [cdist.segment_words(counts_all, world, r)[0] for r in range(world)]
        assert all(sum(w) for w in words), 'the case must make both ranks send'
        SC.hold(s, SC.HOLD_MIN_MS)
        with torch.cuda.stream(s):
            sends = [be.pack(locs[r], counts_all, world, r, int(sum(words[r]))) for r in range(world)]
            recvs = []
            for r in range(world):
                parts = [sends[q][int(sum(words[q][:r])):int(sum(words[q][:r])) + words[q][r]]
                         for q in range(world) if q != r and words[q][r]]
                recvs.append(torch.cat(parts))
            queued = not s.query()
            for r in range(world):
                shards.append(be.merge(locs[r], recvs[r], counts_all, world, r, (0.0, 1.0)))
        assert queued, 'the hold was over before the receive buffers were queued behind pack: nothing was shown'
        got = [np.concatenate([getattr(x, t)() for x in shards]) for t in ('edges', 'features', 'nodes')]
    finally:
        for x in shards + locs:
            x.free()
    e_ref, f_ref = O.boundary_features(lab, data)
    np.testing.assert_array_equal(got[0], e_ref)
    check_features(got[1], f_ref)
    np.testing.assert_array_equal(got[2], O.unique_labels(lab))
