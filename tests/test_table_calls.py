"""What the label-table calls of rag.py hand to the library, without one: L.load
returns a stand-in that records (name, arguments) of every call, writes a fresh
non-zero value through each handle out-pointer, and returns 0 -- or a chosen
status for one chosen function.  For every creating call, reader and accessor on
1 x 1 x 2 volumes and 2-row tables: the sequence of library calls, every
integer, float and enum argument, which pointers are null, that an input that
needs no conversion goes in at its own address, the memory kind, and that the
stream reaches the library as it was given.  Then the dicts of the host
conveniences, and that every handle the stand-in gave out is freed exactly once
-- after a call that returns and after one whose accessor fails -- and a
borrowed one never.

The count getters (ctg_result_num_edges / _nodes) are checked for their handle
and left out of the sequences: how often a table's size is asked is not pinned."""
import ctypes
import gc
import weakref

import numpy as np
import pytest

from cluster_tools_amd import _lib, rag

HOST, DEVICE = _lib.CTG_MEM_HOST, _lib.CTG_MEM_DEVICE
F32, U8, NONE = _lib.CTG_DATA_F32, _lib.CTG_DATA_U8, _lib.CTG_DATA_NONE
N_EDGES, N_NODES = 2, 3
OUT = 'out-pointer'
PTR = 'a non-null pointer'
FREES = ('ctg_free', 'ctg_assignment_free')
COUNTS_OF = ('ctg_result_num_edges', 'ctg_result_num_nodes')
CREATING = ('ctg_rag_features', 'ctg_rag_blocks', 'ctg_unique_labels', 'ctg_merge_stats', 'ctg_unique_values',
            'ctg_unique_pairs', 'ctg_label_overlaps', 'ctg_merge_overlaps', 'ctg_morphology', 'ctg_merge_morphology',
            'ctg_region_features', 'ctg_merge_region_features', 'ctg_assignment_dense', 'ctg_assignment_sparse')


class Library:
    """The recording stand-in of libctg.so."""

    def __init__(self):
        self.calls = []        # (name, raw arguments)
        self.given = []        # handle values written through out-pointers
        self.fail = {}         # name -> status

    def __getattr__(self, name):
        if not name.startswith('ctg_'):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name == 'ctg_last_error':
                return b'made to fail'
            if name in COUNTS_OF:
                return N_EDGES if name.endswith('edges') else N_NODES
            if name in FREES:
                return None
            if name in self.fail:
                return self.fail[name]
            if name in CREATING:
                self.given.append(0x1000 + 16 * len(self.given))
                args[-1]._obj.value = self.given[-1]
            if name == 'ctg_result_info':
                args[1]._obj.value, args[2]._obj.value = 7, 5
            if name == 'ctg_assignment_info':
                args[1]._obj.value, args[2]._obj.value, args[3]._obj.value = 2, 9, _lib.CTG_ASSIGN_SPARSE
            return 0
        return call

    def freed(self):
        return sorted(a[0].value for n, a in self.calls if n in FREES)

    def sequence(self):
        """The calls without the count getters, arguments in a comparable form."""
        return [(n, [plain(x) for x in a]) for n, a in self.calls if n not in COUNTS_OF]


def plain(x):
    if x is None or isinstance(x, (int, float)):
        return x
    if isinstance(x, ctypes.c_void_p):
        return ('ptr', x.value)
    if isinstance(x, ctypes.Array):
        return list(x)
    if hasattr(x, '_obj'):
        return OUT
    raise AssertionError('an argument of type %s' % type(x))


def at(x):
    """The pointer form of an array's (tensor's) own address."""
    return ('ptr', x.data_ptr() if hasattr(x, 'data_ptr') else x.ctypes.data)


def matches(got, want):
    if want is PTR:
        return isinstance(got, tuple) and got[0] == 'ptr' and got[1]
    return type(got) is type(want) and got == want


def check_sequence(lib, want):
    got = lib.sequence()
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, g), (_, w) in zip(got, want):
        assert len(g) == len(w), (name, g, w)
        for k, (a, b) in enumerate(zip(g, w)):
            assert matches(a, b), '%s argument %d: got %r, want %r' % (name, k, a, b)
    for n, a in lib.calls:
        if n in COUNTS_OF:
            assert len(a) == 1 and a[0].value in lib.given + [BORROWED]


@pytest.fixture
def lib(monkeypatch):
    lib = Library()
    monkeypatch.setattr(rag.L, 'load', lambda: lib)
    monkeypatch.setattr(rag.L, 'init_device', lambda device=None: 0)
    made = weakref.WeakSet()
    for cls in (rag.Result, rag.Assignment):
        def init(self, *a, _init=cls.__init__, **kw):
            made.add(self)
            _init(self, *a, **kw)
        monkeypatch.setattr(cls, '__init__', init)
    yield lib
    # no wrapper of a stand-in handle may outlive the stand-in (a failed test's traceback can hold one)
    for obj in list(made):
        obj.handle = None


BORROWED = 0x77
LAB = np.array([[[1, 2]]], np.uint64)
LAB32 = np.array([[[3, 3]]], np.uint32)
DAT = np.array([[[0.25, 0.5]]], np.float32)
DAT8 = np.array([[[4, 200]]], np.uint8)
SHAPE = [1, 1, 2]
PAIRS = np.array([[1, 3], [2, 3]], np.uint64)
COUNTS = np.array([1, 1], np.uint64)
SUMS = np.zeros((2, 2), np.float64)
RECS = np.zeros((2, rag.WIDE_WORDS), np.uint32)
MORPH = np.zeros((2, 11), np.float64)
REGION = np.zeros((2, 5), np.float64)
FEATS = np.zeros((2, 10), np.float64)
BLOCK = [dict(label_offset=0, shape=SHAPE, own=([0, 0, 0], SHAPE), graph=([0, 0, 0], SHAPE))]
STREAMS = {'null': None, 'given': ctypes.c_void_p(5)}


def stream_arg(s):
    return None if s is None else ('ptr', s.value)


# name -> (the call of a stream, the library calls it makes given the stream's plain form and the handle)
def creating_calls():
    h = ('ptr', 0x1000)
    info = ('ctg_assignment_info', [h, OUT, OUT, OUT])
    return {
        'rag_features': (
            lambda s: rag.rag_features_handle(LAB, DAT, stream=s),
            lambda s: [('ctg_rag_features', [at(LAB), 64, at(DAT), F32, 0, None, SHAPE, None, None, 0, 0.0, 1.0, 0,
                                             HOST, s, OUT])]),
        'rag_features_flags': (
            lambda s: rag.rag_features_handle(LAB32, None, own_begin=(0, 0, 0), own_end=(1, 1, 1), ignore_label=True,
                                              hist_range=(-1, 3), keep_stats=True, stream=s, no_adj_filter=True,
                                              defer_stats=True),
            lambda s: [('ctg_rag_features', [at(LAB32), 32, None, NONE, 0, None, SHAPE, [0, 0, 0], [1, 1, 1], 1,
                                             -1.0, 3.0, 11, HOST, s, OUT])]),
        'rag_features_affinities': (
            lambda s: rag.rag_features_handle(LAB, DAT8[None], offsets=[[0, 0, -1]], stream=s),
            lambda s: [('ctg_rag_features', [at(LAB), 64, at(DAT8), U8, 1, PTR, SHAPE, None, None, 0, 0.0, 1.0, 0,
                                             HOST, s, OUT])]),
        'unique_values': (
            lambda s: rag.unique_values_handle(COUNTS, stream=s),
            lambda s: [('ctg_unique_values', [at(COUNTS), 2, HOST, s, OUT])]),
        'merge_stats': (
            lambda s: rag.merge_stats_handle(PAIRS, SUMS, RECS, (0.5, 2), True, stream=s),
            lambda s: [('ctg_merge_stats', [at(PAIRS), at(SUMS), at(RECS), 2, 0.5, 2.0, 1, HOST, s, OUT])]),
        'label_overlaps': (
            lambda s: rag.label_overlaps_handle(LAB, LAB32, stream=s),
            lambda s: [('ctg_label_overlaps', [at(LAB), 64, at(LAB32), 32, SHAPE, None, None, 0, 0, HOST, s, OUT])]),
        'label_overlaps_box_ignore_zero': (
            lambda s: rag.label_overlaps_handle(LAB32, LAB, (0, 0, 1), (1, 1, 2), 0, stream=s),
            lambda s: [('ctg_label_overlaps', [at(LAB32), 32, at(LAB), 64, SHAPE, [0, 0, 1], [1, 1, 2], 1, 0, HOST, s,
                                               OUT])]),
        'label_overlaps_ignore_top': (
            lambda s: rag.label_overlaps_handle(LAB, LAB, None, (1, 1, 1), (1 << 64) - 1, stream=s),
            lambda s: [('ctg_label_overlaps', [at(LAB), 64, at(LAB), 64, SHAPE, None, [1, 1, 1], 1, (1 << 64) - 1,
                                               HOST, s, OUT])]),
        'merge_overlaps': (
            lambda s: rag.merge_overlaps_handle(PAIRS, COUNTS, stream=s),
            lambda s: [('ctg_merge_overlaps', [at(PAIRS), at(COUNTS), 2, HOST, s, OUT])]),
        'morphology': (
            lambda s: rag.morphology_handle(LAB, stream=s),
            lambda s: [('ctg_morphology', [at(LAB), 64, SHAPE, None, None, None, HOST, s, OUT])]),
        'morphology_box_origin': (
            lambda s: rag.morphology_handle(LAB32, (0, 0, 1), (1, 1, 2), (5, 6, 7), stream=s),
            lambda s: [('ctg_morphology', [at(LAB32), 32, SHAPE, [0, 0, 1], [1, 1, 2], [5, 6, 7], HOST, s, OUT])]),
        'morphology_origin_alone': (
            lambda s: rag.morphology_handle(LAB, origin=(5, 6, 7), stream=s),
            lambda s: [('ctg_morphology', [at(LAB), 64, SHAPE, None, None, [5, 6, 7], HOST, s, OUT])]),
        'merge_morphology': (
            lambda s: rag.merge_morphology_handle(MORPH, stream=s),
            lambda s: [('ctg_merge_morphology', [at(MORPH), 2, HOST, s, OUT])]),
        'merge_morphology_flat': (
            lambda s: rag.merge_morphology_handle(MORPH.reshape(-1), stream=s),
            lambda s: [('ctg_merge_morphology', [at(MORPH), 2, HOST, s, OUT])]),
        'region_features': (
            lambda s: rag.region_features_handle(LAB, DAT, stream=s),
            lambda s: [('ctg_region_features', [at(LAB), 64, at(DAT), F32, SHAPE, None, None, 0, 0, HOST, s, OUT])]),
        'region_features_u8_box_ignore': (
            lambda s: rag.region_features_handle(LAB32, DAT8, (0, 0, 0), (1, 1, 1), 3, stream=s),
            lambda s: [('ctg_region_features', [at(LAB32), 32, at(DAT8), U8, SHAPE, [0, 0, 0], [1, 1, 1], 1, 3, HOST,
                                                s, OUT])]),
        'merge_region_features': (
            lambda s: rag.merge_region_features_handle(REGION, stream=s),
            lambda s: [('ctg_merge_region_features', [at(REGION), 2, HOST, s, OUT])]),
        'assignment_dense': (
            lambda s: rag.assignment_dense(COUNTS, stream=s),
            lambda s: [('ctg_assignment_dense', [at(COUNTS), 2, HOST, s, OUT]), info]),
        'assignment_sparse': (
            lambda s: rag.assignment_sparse(COUNTS, PAIRS[:, 0].copy(), stream=s),
            lambda s: [('ctg_assignment_sparse', [at(COUNTS), PTR, 2, HOST, s, OUT]), info]),
    }


@pytest.mark.parametrize('stream', sorted(STREAMS))
@pytest.mark.parametrize('name', sorted(creating_calls()))
def test_creating_call(lib, name, stream):
    call, want = creating_calls()[name]
    s = STREAMS[stream]
    r = call(s)
    assert type(r) is (rag.Assignment if name.startswith('assignment') else rag.Result)
    assert r.handle.value == 0x1000 and r.device == 0
    check_sequence(lib, want(stream_arg(s)))
    for n, a in lib.calls:                                    # the very object, not a copy of its value
        if n in CREATING:
            assert a[-2] is s
    if name.startswith('assignment'):
        assert (r.n, r.max_value, r.kind) == (2, 9, 'sparse')
    r.free()
    r.free()                                                  # idempotent
    assert lib.freed() == [0x1000] and r.handle is None


def test_converted_inputs_are_copies(lib):
    """Signed labels keep their width and address; other integers and strided arrays are converted."""
    signed = LAB.view(np.int64)
    rag.morphology_handle(signed).free()
    small = np.array([[[1, 2]]], np.uint16)
    rag.morphology_handle(small).free()
    strided = np.zeros((1, 1, 4), np.uint64)[:, :, ::2]
    rag.morphology_handle(strided).free()
    a, b, c = [x for n, x in lib.sequence() if n == 'ctg_morphology']
    assert a[:2] == [at(signed), 64]
    assert b[1] == 64 and b[0] != at(small) and b[0][1]
    assert c[1] == 64 and c[0] != at(strided) and c[0][1]


# ------------------------------------- the calls that free their handle themselves
def test_unique_labels(lib):
    for s, (b, e) in zip(STREAMS.values(), ((None, None), ((0, 0, 1), (1, 1, 2)))):
        lib.calls.clear()
        got = rag.unique_labels(LAB, b, e, stream=s)
        h = ('ptr', lib.given[-1])
        assert got.dtype == np.uint64 and got.shape == (N_NODES,)
        check_sequence(lib, [('ctg_unique_labels', [at(LAB), SHAPE, b and list(b), e and list(e), HOST,
                                                    stream_arg(s), OUT]),
                             ('ctg_result_copy_nodes', [h, at(got), HOST]), ('ctg_free', [h])])
        assert lib.calls[0][1][-2] is s


@pytest.mark.parametrize('stream', sorted(STREAMS))
def test_raw_stream_calls(lib, stream):
    s = STREAMS[stream]
    edges, nodes = rag.unique_pairs(PAIRS, stream=s)
    h = ('ptr', 0x1000)
    assert (edges.dtype, edges.shape, nodes.dtype, nodes.shape) == (np.uint64, (N_EDGES, 2), np.uint64, (N_NODES,))
    check_sequence(lib, [('ctg_unique_pairs', [at(PAIRS), 2, HOST, stream_arg(s), OUT]),
                         ('ctg_result_copy_edges', [h, at(edges), HOST]),
                         ('ctg_result_copy_nodes', [h, at(nodes), HOST]), ('ctg_free', [h])])
    assert lib.calls[0][1][-2] is s
    lib.calls.clear()
    rows = rag.merge_feature_rows(COUNTS, FEATS, 4, 7, stream=s)
    assert rows.dtype == np.float64 and rows.shape == (3, 10)
    check_sequence(lib, [('ctg_merge_feature_rows', [at(COUNTS), at(FEATS), 2, 4, 7, at(rows), HOST, stream_arg(s)])])
    assert lib.calls[0][1][-1] is s
    lib.calls.clear()
    ids = rag.map_edge_ids(PAIRS, PAIRS[:1], stream=s)
    assert ids.dtype == np.int64 and ids.shape == (1,)
    check_sequence(lib, [('ctg_map_edge_ids', [at(PAIRS), 2, at(PAIRS), 1, at(ids), HOST, stream_arg(s)])])
    assert lib.calls[0][1][-1] is s


def test_rag_blocks_arena(lib):
    for s in STREAMS.values():
        lib.calls.clear()
        out = rag.rag_blocks_arena(LAB.reshape(-1), BLOCK, DAT.reshape(-1), keep_stats=True, nodes=False, stream=s)
        h = ('ptr', lib.given[-1])
        check_sequence(lib, [
            ('ctg_rag_blocks', [at(LAB), 64, at(DAT), F32, 0, None, PTR, 1, 2, 2, 0, 0.0, 1.0,
                                _lib.CTG_KEEP_STATS | _lib.CTG_NO_NODES, HOST, stream_arg(s), OUT]),
            ('ctg_result_block_offsets', [h, PTR, PTR]), ('ctg_result_copy_edges', [h, PTR, HOST]),
            ('ctg_result_copy_nodes', [h, PTR, HOST]), ('ctg_result_copy_features', [h, PTR, HOST]),
            ('ctg_result_copy_stats', [h, PTR, PTR, HOST]), ('ctg_free', [h])])
        assert lib.calls[0][1][-2] is s
        assert len(out) == 1 and sorted(out[0]) == ['edges', 'features', 'nodes', 'records', 'sums']
        assert out[0]['edges'].shape == (0, 2) and out[0]['records'].shape == (0, rag.WIDE_WORDS)
    lib.calls.clear()
    out = rag.rag_blocks_arena(LAB32.reshape(-1), BLOCK, ignore_label=True)
    assert lib.sequence()[0][1][:14] == [at(LAB32), 32, None, NONE, 0, None, lib.sequence()[0][1][6], 1, 2, 0, 1,
                                         0.0, 1.0, 0]
    assert [n for n, _ in lib.sequence()] == ['ctg_rag_blocks', 'ctg_result_block_offsets', 'ctg_result_copy_edges',
                                              'ctg_result_copy_nodes', 'ctg_free']
    assert sorted(out[0]) == ['edges', 'nodes']


# ---------------------------------------------------------------- readers
def borrowed():
    return rag.Result(ctypes.c_void_p(BORROWED), 0)


def readers():
    """name -> (the reader of (handle or tables, stream), the tables to merge first, the merge's library call,
    the reader's library call given the handle and the stream, the shapes and dtype of what comes back)"""
    sums, feats = _lib.CTG_REGION_SUMS, _lib.CTG_REGION_FEATURES
    return {
        'max_overlaps': (
            lambda x, s: rag.max_overlaps(x, 1, 4, stream=s), dict(pairs=PAIRS, counts=COUNTS),
            lambda s: ('ctg_merge_overlaps', [at(PAIRS), at(COUNTS), 2, HOST, s, OUT]),
            lambda h, s: ('ctg_max_overlaps', [h, 1, 4, PTR, PTR, HOST, s]), [(3,), (3,)], np.uint64),
        'morphology_rows': (
            lambda x, s: rag.morphology_rows(x, 1, 4, stream=s), dict(rows=MORPH),
            lambda s: ('ctg_merge_morphology', [at(MORPH), 2, HOST, s, OUT]),
            lambda h, s: ('ctg_morphology_rows', [h, 1, 4, PTR, None, HOST, s]), [(3, 11)], np.float64),
        'region_feature_rows': (
            lambda x, s: rag.region_feature_rows(x, 1, 4, stream=s), dict(rows=REGION),
            lambda s: ('ctg_merge_region_features', [at(REGION), 2, HOST, s, OUT]),
            lambda h, s: ('ctg_region_rows', [h, 1, 4, feats, 1.0, PTR, None, HOST, s]), [(3, 5)], np.float64),
        'region_feature_rows_sums_norm': (
            lambda x, s: rag.region_feature_rows(x, 0, 0, 'sums', 255, stream=s), dict(rows=REGION),
            lambda s: ('ctg_merge_region_features', [at(REGION), 2, HOST, s, OUT]),
            lambda h, s: ('ctg_region_rows', [h, 0, 0, sums, 255.0, PTR, None, HOST, s]), [(0, 5)], np.float64),
    }


def null_or(got, s):
    """A handle reader's stream: ``s`` itself; for None the null stream -- None, or the handle of torch's current
    stream where an earlier test of the process has started torch on the GPU."""
    if s is not None:
        return got is s
    return got is None or (isinstance(got, ctypes.c_void_p) and _torch_started())


def _torch_started():
    import sys
    torch = sys.modules.get('torch')
    return torch is not None and torch.cuda.is_initialized()


def check_reader_sequence(lib, want, s):
    """check_sequence, the last argument of every handle reader compared by null_or."""
    got = lib.sequence()
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, raw), (_, g), (_, w) in zip([c for c in lib.calls if c[0] not in COUNTS_OF], got, want):
        if name in ('ctg_max_overlaps', 'ctg_morphology_rows', 'ctg_region_rows'):
            assert null_or(raw[-1], s), (name, raw[-1])
            g, w = g[:-1], w[:-1]
        assert len(g) == len(w), (name, g, w)
        for k, (a, b) in enumerate(zip(g, w)):
            assert matches(a, b), '%s argument %d: got %r, want %r' % (name, k, a, b)


def shapes_of(got):
    return [(x.shape, x.dtype) for x in (got if isinstance(got, tuple) else (got,))]


@pytest.mark.parametrize('stream', sorted(STREAMS))
@pytest.mark.parametrize('name', sorted(readers()))
def test_reader_of_a_borrowed_handle(lib, name, stream):
    read, _, _, want, shapes, dtype = readers()[name]
    s = STREAMS[stream]
    r = borrowed()
    got = read(r, s)
    assert shapes_of(got) == [(sh, dtype) for sh in shapes]
    check_reader_sequence(lib, [want(('ptr', BORROWED), stream_arg(s))], s)
    assert r.handle.value == BORROWED and lib.freed() == []


@pytest.mark.parametrize('stream', sorted(STREAMS))
@pytest.mark.parametrize('name', sorted(readers()))
def test_reader_of_tables(lib, name, stream):
    read, tables, merge, want, shapes, dtype = readers()[name]
    s = STREAMS[stream]
    got = read(tables, s)
    assert shapes_of(got) == [(sh, dtype) for sh in shapes]
    h = ('ptr', 0x1000)
    check_reader_sequence(lib, [merge(stream_arg(s)), want(h, stream_arg(s)), ('ctg_free', [h])], s)
    assert lib.calls[0][1][-2] is s


def accessors():
    """name -> (the accessor of a Result, the library call after the count getters given the handle -- PTR where
    the fresh output goes --, the shapes and dtypes of what comes back)"""
    E, N = N_EDGES, N_NODES
    u64, f64 = np.dtype(np.uint64), np.dtype(np.float64)
    return {
        'edges': (lambda r: r.edges(), 'ctg_result_copy_edges', [PTR, HOST], [((E, 2), u64)]),
        'nodes': (lambda r: r.nodes(), 'ctg_result_copy_nodes', [PTR, HOST], [((N,), u64)]),
        'features': (lambda r: r.features(), 'ctg_result_copy_features', [PTR, HOST], [((E, 10), f64)]),
        'stats': (lambda r: r.stats(), 'ctg_result_copy_stats', [PTR, PTR, HOST],
                  [((E, 2), f64), ((E, rag.WIDE_WORDS), np.dtype(np.uint32))]),
        'counts': (lambda r: r.counts(), 'ctg_result_copy_counts', [PTR, HOST], [((E,), u64)]),
        'moments': (lambda r: r.moments(), 'ctg_result_copy_moments', [PTR, HOST], [((N, 10), u64)]),
        'region_moments': (lambda r: r.region_moments(), 'ctg_result_copy_region', [PTR, PTR, PTR, HOST],
                           [((N,), u64), ((N,), f64), ((N, 2), np.dtype(np.float32))]),
    }


@pytest.mark.parametrize('name', sorted(accessors()))
def test_host_accessor(lib, name):
    read, fn, args, shapes = accessors()[name]
    r = borrowed()
    got = read(r)
    assert shapes_of(got) == shapes
    check_sequence(lib, [(fn, [('ptr', BORROWED)] + args)])
    outs = got if isinstance(got, tuple) else (got,)
    assert [plain(x) for x in lib.calls[-1][1][1:-1]] == [at(x) for x in outs]


@pytest.mark.parametrize('stream', sorted(STREAMS))
def test_host_row_accessors(lib, stream):
    s = STREAMS[stream]
    r = borrowed()
    h = ('ptr', BORROWED)
    rows = r.morph_rows(stream=s)
    assert shapes_of(rows) == [((N_NODES, 11), np.float64)]
    check_reader_sequence(lib, [('ctg_morphology_rows', [h, 0, 0, None, at(rows), HOST, stream_arg(s)])], s)
    for kw, form, norm in ((dict(), _lib.CTG_REGION_SUMS, 1.0),
                           (dict(form='features', norm=255), _lib.CTG_REGION_FEATURES, 255.0)):
        lib.calls.clear()
        rows = r.region_rows(stream=s, **kw)
        assert shapes_of(rows) == [((N_NODES, 5), np.float64)]
        check_reader_sequence(lib, [('ctg_region_rows', [h, 0, 0, form, norm, None, at(rows), HOST, stream_arg(s)])],
                              s)
    with pytest.raises(ValueError) as e:
        r.region_rows('mean')
    assert str(e.value) == "form must be 'sums' or 'features', got 'mean'"
    lib.calls.clear()
    assert (r.n_edges, r.n_nodes, r.info()) == (N_EDGES, N_NODES, (7, 5))
    check_sequence(lib, [('ctg_result_info', [h, OUT, OUT])])


# ----------------------------------------------------- the conveniences' dicts
def conveniences():
    """name -> (the call, the library function that makes its handle, an accessor's function to make fail, the
    (key, shape, dtype) entries of its dict -- None for an int)"""
    E, N = N_EDGES, N_NODES
    u64, f64, u32, f32 = np.uint64, np.float64, np.uint32, np.float32
    info = [('n_records', None, None), ('n_direct', None, None)]
    overlaps = [('pairs', (E, 2), u64), ('counts', (E,), u64), ('nodes', (N,), u64)]
    morph = [('nodes', (N,), u64), ('moments', (N, 10), u64), ('rows', (N, 11), f64)]
    region = [('nodes', (N,), u64), ('counts', (N,), u64), ('sums', (N,), f64), ('minmax', (N, 2), f32),
              ('rows', (N, 5), f64), ('features', (N, 5), f64)]
    stats = [('sums', (E, 2), f64), ('records', (E, rag.WIDE_WORDS), u32)]
    return {
        'rag_features': (lambda: rag.rag_features(LAB, DAT, keep_stats=True), 'ctg_result_copy_nodes',
                         [('edges', (E, 2), u64), ('nodes', (N,), u64), ('features', (E, 10), f64)] + stats + info),
        'rag_features_labels_only': (lambda: rag.rag_features(LAB, keep_stats=True), 'ctg_result_info',
                                     [('edges', (E, 2), u64), ('nodes', (N,), u64)] + info),
        'merge_stats': (lambda: rag.merge_stats(PAIRS, SUMS, RECS), 'ctg_result_copy_features',
                        [('edges', (E, 2), u64), ('features', (E, 10), f64)]),
        'merge_stats_kept': (lambda: rag.merge_stats(PAIRS, SUMS, RECS, keep_stats=True), 'ctg_result_copy_stats',
                             [('edges', (E, 2), u64), ('features', (E, 10), f64)] + stats),
        'label_overlaps': (lambda: rag.label_overlaps(LAB, LAB32), 'ctg_result_copy_counts', overlaps + info),
        'merge_overlaps': (lambda: rag.merge_overlaps(PAIRS, COUNTS), 'ctg_result_copy_nodes', overlaps),
        'morphology': (lambda: rag.morphology(LAB), 'ctg_result_copy_moments', morph + info),
        'merge_morphology': (lambda: rag.merge_morphology(MORPH), 'ctg_morphology_rows', morph),
        'region_features': (lambda: rag.region_features(LAB, DAT8), 'ctg_region_rows', region + info),
        'merge_region_features': (lambda: rag.merge_region_features(REGION, 2.0), 'ctg_result_copy_region', region),
    }


@pytest.mark.parametrize('name', sorted(conveniences()))
def test_convenience_dict(lib, name):
    call, _, entries = conveniences()[name]
    out = call()
    assert list(out) == [k for k, _, _ in entries]
    for key, shape, dtype in entries:
        if shape is None:
            assert type(out[key]) is int
        else:
            assert isinstance(out[key], np.ndarray) and (out[key].shape, out[key].dtype) == (shape, dtype), key
    assert lib.freed() == lib.given == [0x1000]
    assert lib.calls[-1][0] == 'ctg_free'
    if 'n_records' in out:
        assert (out['n_records'], out['n_direct']) == (7, 5)


def test_region_features_default_norm(lib):
    """None: 255 for uint8 data and 1 otherwise, in the feature form only."""
    for data, norm in ((DAT8, 255.0), (DAT, 1.0)):
        lib.calls.clear()
        rag.region_features(LAB, data)
        forms = [(a[3], a[4]) for n, a in lib.sequence() if n == 'ctg_region_rows']
        assert forms == [(_lib.CTG_REGION_SUMS, 1.0), (_lib.CTG_REGION_FEATURES, norm)]
    lib.calls.clear()
    rag.region_features(LAB, DAT8, norm=3)
    assert [a[4] for n, a in lib.sequence() if n == 'ctg_region_rows'] == [1.0, 3.0]


# ------------------------------------------------------------ handle lifetime
def lifetimes():
    """name -> (the call, the library function to make fail): every call that makes a handle and frees it."""
    out = {k: (v[0], v[1]) for k, v in conveniences().items()}
    out['unique_labels'] = (lambda: rag.unique_labels(LAB), 'ctg_result_copy_nodes')
    out['unique_pairs'] = (lambda: rag.unique_pairs(PAIRS), 'ctg_result_copy_nodes')
    out['rag_blocks_arena'] = (lambda: rag.rag_blocks_arena(LAB.reshape(-1), BLOCK), 'ctg_result_block_offsets')
    out['rag_blocks_arena_accessor'] = (lambda: rag.rag_blocks_arena(LAB.reshape(-1), BLOCK), 'ctg_result_copy_edges')
    for name, (read, tables, _, want, _, _) in readers().items():
        out[name + '_of_tables'] = (lambda read=read, tables=tables: read(tables, None), want(None, None)[0])
    return out


def _fails(call):
    """The call raises CtgError; the exception (whose traceback holds the call's frames) ends here."""
    with pytest.raises(_lib.CtgError, match='made to fail'):
        call()


@pytest.mark.parametrize('name', sorted(lifetimes()))
def test_handle_is_freed_once(lib, name):
    call, fail = lifetimes()[name]
    call()
    assert lib.freed() == lib.given == [0x1000]
    lib.fail[fail] = -2
    _fails(call)
    gc.collect()
    assert lib.given == [0x1000, 0x1010] and lib.freed() == lib.given


@pytest.mark.parametrize('name', sorted(readers()))
def test_borrowed_handle_is_not_freed(lib, name):
    read, _, _, want, _, _ = readers()[name]
    r = borrowed()
    read(r, None)
    lib.fail[want(None, None)[0]] = -2
    _fails(lambda: read(r, None))
    gc.collect()
    assert lib.freed() == [] and lib.given == [] and r.handle.value == BORROWED


def test_a_failed_creating_call_leaves_no_handle(lib):
    lib.fail['ctg_morphology'] = -1
    _fails(lambda: rag.morphology(LAB))
    lib.fail = {'ctg_assignment_dense': -1}
    _fails(lambda: rag.assignment_dense(COUNTS))
    gc.collect()
    assert lib.given == [] and lib.freed() == []


# ------------------------------------------------------ tensors on the device
def torch_accessors(torch):
    """name -> (the accessor, its library function, the arguments between handle and memory kind that are not the
    new tensors, shapes, dtype)"""
    E, N = N_EDGES, N_NODES
    i64, f64 = torch.int64, torch.float64
    return {
        'edges_torch_i64': (lambda r: r.edges_torch_i64(), 'ctg_result_copy_edges', [(E, 2)], i64),
        'nodes_torch': (lambda r: r.nodes_torch(), 'ctg_result_copy_nodes', [(N,)], i64),
        'features_torch': (lambda r: r.features_torch(), 'ctg_result_copy_features', [(E, 10)], f64),
        'counts_torch': (lambda r: r.counts_torch(), 'ctg_result_copy_counts', [(E,)], i64),
        'moments_torch': (lambda r: r.moments_torch(), 'ctg_result_copy_moments', [(N, 10)], i64),
    }


@pytest.mark.gpu
def test_device_tensors_reach_the_library(gpu, lib, monkeypatch):
    """CUDA tensors of 1 x 1 x 2 voxels and 2 rows through the stand-in (no kernel runs): every creating call
    passes CTG_MEM_DEVICE, the tensor's own pointer and -- inside torch.cuda.stream(side) -- the side stream's
    handle; every *_torch accessor CTG_MEM_DEVICE and its new tensor's pointer, after _before_device_copy."""
    import torch
    dev = torch.device('cuda:0')
    lab, lab32 = torch.tensor(LAB.astype(np.int64), device=dev), torch.tensor(LAB32.astype(np.int32), device=dev)
    dat, dat8 = torch.tensor(DAT, device=dev), torch.tensor(DAT8, device=dev)
    pairs, counts = torch.tensor(PAIRS.astype(np.int64), device=dev), torch.tensor(COUNTS.astype(np.int64), device=dev)
    sums, recs = torch.tensor(SUMS, device=dev), torch.tensor(RECS.astype(np.int32), device=dev)
    morph, region = torch.tensor(MORPH, device=dev), torch.tensor(REGION, device=dev)
    side = torch.cuda.Stream()
    calls = {
        'ctg_rag_features': (lambda: rag.rag_features_handle(lab, dat), [at(lab), 64, at(dat), F32]),
        'ctg_rag_blocks': (lambda: rag.rag_blocks_arena(lab.reshape(-1), BLOCK, dat8.reshape(-1)),
                           [at(lab), 64, at(dat8), U8]),
        'ctg_unique_labels': (lambda: rag.unique_labels(lab), [at(lab)]),
        'ctg_merge_stats': (lambda: rag.merge_stats_handle(pairs, sums, recs), [at(pairs), at(sums), at(recs), 2]),
        'ctg_unique_values': (lambda: rag.unique_values_handle(counts), [at(counts), 2]),
        'ctg_label_overlaps': (lambda: rag.label_overlaps_handle(lab, lab32), [at(lab), 64, at(lab32), 32]),
        'ctg_merge_overlaps': (lambda: rag.merge_overlaps_handle(pairs, counts), [at(pairs), at(counts), 2]),
        'ctg_morphology': (lambda: rag.morphology_handle(lab32), [at(lab32), 32]),
        'ctg_merge_morphology': (lambda: rag.merge_morphology_handle(morph), [at(morph), 2]),
        'ctg_region_features': (lambda: rag.region_features_handle(lab, dat8), [at(lab), 64, at(dat8), U8]),
        'ctg_merge_region_features': (lambda: rag.merge_region_features_handle(region), [at(region), 2]),
        'ctg_assignment_dense': (lambda: rag.assignment_dense(counts), [at(counts), 2]),
        'ctg_assignment_sparse': (lambda: rag.assignment_sparse(counts, pairs[:, 0].contiguous()), [at(counts)]),
    }
    assert sorted(calls) == sorted(set(CREATING) - {'ctg_unique_pairs'})      # (unique_pairs takes host pairs only)
    with torch.cuda.stream(side):
        assert side.cuda_stream != 0
        for fn, (call, head) in sorted(calls.items()):
            lib.calls.clear()
            r = call()
            name, args = lib.sequence()[0]
            assert name == fn and args[:len(head)] == head, (fn, args)
            assert args[-3:] == [DEVICE, ('ptr', side.cuda_stream), OUT], (fn, args)
            if hasattr(r, 'free'):
                r.free()
        # a reader of a handle without a stream of its own: torch's current one
        lib.calls.clear()
        rag.morphology_rows(borrowed(), 0, 2)
        assert lib.sequence()[0][1][-1] == ('ptr', side.cuda_stream)
    order = []
    monkeypatch.setattr(rag.Result, '_before_device_copy', staticmethod(lambda: order.append('sync')))
    r = borrowed()
    r.device = 0
    for name, (read, fn, shapes, dtype) in sorted(torch_accessors(torch).items()):
        lib.calls.clear()
        del order[:]
        t = read(r)
        assert (tuple(t.shape), t.dtype, t.device) == (shapes[0], dtype, dev), name
        assert lib.sequence() == [(fn, [('ptr', BORROWED), at(t), DEVICE])] and order == ['sync'], name
    lib.calls.clear()
    del order[:]
    e = r.edges_torch()
    assert e.dtype == (torch.uint64 if hasattr(torch, 'uint64') else torch.int64) and tuple(e.shape) == (N_EDGES, 2)
    assert lib.sequence() == [('ctg_result_copy_edges', [('ptr', BORROWED), at(e), DEVICE])] and order == ['sync']
    lib.calls.clear()
    del order[:]
    s, w = r.stats_torch()
    assert (tuple(s.shape), s.dtype, tuple(w.shape), w.dtype) == ((N_EDGES, 2), torch.float64,
                                                                   (N_EDGES, rag.WIDE_WORDS), torch.int32)
    assert lib.sequence() == [('ctg_result_copy_stats', [('ptr', BORROWED), at(s), at(w), DEVICE])]
    assert order == ['sync']
    five = ctypes.c_void_p(5)
    for read, want in ((lambda: r.morph_rows_torch(stream=five), lambda t: ('ctg_morphology_rows',
                                                                            [('ptr', BORROWED), 0, 0, None, at(t),
                                                                             DEVICE, ('ptr', 5)])),
                       (lambda: r.region_rows_torch('features', 255, stream=five),
                        lambda t: ('ctg_region_rows', [('ptr', BORROWED), 0, 0, _lib.CTG_REGION_FEATURES, 255.0, None,
                                                       at(t), DEVICE, ('ptr', 5)]))):
        lib.calls.clear()
        t = read()
        assert t.dtype == torch.float64 and t.device == dev and t.shape[0] == N_NODES
        assert lib.sequence() == [want(t)]
        assert lib.calls[-1][1][-1] is five
