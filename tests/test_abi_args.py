"""The argument errors of the C ABI that are decided before any GPU work:
status and message of every such return, called through the built library
with small numpy buffers (no GPU: each call returns at its argument checks).
Where two errors apply at once the case pins which one is reported.  A failing
call leaves *out null."""
import ctypes

import numpy as np
import pytest

from cluster_tools_amd import _lib

ARG, UNSUPPORTED = -1, -4
SENTINEL = 0xDEAD0


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def i64(*v):
    return np.array(v, dtype=np.int64)


def fails(lib, rc, status, text, out=None):
    msg = lib.ctg_last_error().decode()
    assert rc == status, (rc, msg)
    assert text in msg, msg
    if out is not None:
        assert not out.value, 'a failing call left *out set'


LABELS = np.zeros(64, dtype=np.uint64)
DATA = np.zeros(64, dtype=np.float32)
SHAPE = i64(4, 4, 4)
NN = np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.int32)


# ---------------------------------------------------------------------------
# ctg_rag_features
# ---------------------------------------------------------------------------
def rag_features(lib, labels=LABELS, label_bits=64, data=None, data_kind=_lib.CTG_DATA_NONE, n_channels=0,
                 offsets=None, shape=SHAPE, own_begin=None, own_end=None, hist=(0.0, 1.0), out=True, start=SENTINEL):
    o = ctypes.c_void_p(start)
    rc = lib.ctg_rag_features(ptr(labels), label_bits, ptr(data), data_kind, n_channels, ptr(offsets), ptr(shape),
                              ptr(own_begin), ptr(own_end), 0, hist[0], hist[1], 0, _lib.CTG_MEM_HOST, None,
                              ctypes.byref(o) if out else None)
    return rc, (o if out else None)


# the first check returns before *out is cleared: those calls start from null
RAG_FEATURES_ERRORS = [
    (dict(out=False), 'ctg_rag_features: null argument'),
    (dict(labels=None, start=0), 'ctg_rag_features: null argument'),
    (dict(shape=None, start=0), 'ctg_rag_features: null argument'),
    (dict(label_bits=16), 'ctg_rag_features: label_bits must be 32 or 64'),
    (dict(n_channels=-1), 'ctg_rag_features: bad channel/offset arguments'),
    (dict(n_channels=_lib.CTG_MAX_CHANNELS + 1, offsets=NN), 'ctg_rag_features: bad channel/offset arguments'),
    (dict(data=DATA, data_kind=_lib.CTG_DATA_F32, n_channels=3), 'ctg_rag_features: bad channel/offset arguments'),
    (dict(data=DATA, data_kind=7), 'ctg_rag_features: data_kind must be CTG_DATA_F32 or CTG_DATA_U8'),
    (dict(data=DATA, data_kind=_lib.CTG_DATA_NONE), 'ctg_rag_features: data_kind must be CTG_DATA_F32 or CTG_DATA_U8'),
    (dict(hist=(1.0, 1.0)), 'ctg_rag_features: hist_hi must be > hist_lo'),
    (dict(hist=(0.0, float('nan'))), 'ctg_rag_features: hist_hi must be > hist_lo'),
    (dict(shape=i64(4, -1, 4)), 'ctg_rag_features: negative shape/own_begin/own_end'),
    (dict(own_begin=i64(0, 0, -1)), 'ctg_rag_features: negative shape/own_begin/own_end'),
    (dict(own_end=i64(-2, 4, 4)), 'ctg_rag_features: negative shape/own_begin/own_end'),
    # two errors at once: the checks run in the order above
    (dict(label_bits=16, n_channels=-1), 'label_bits must be 32 or 64'),
    (dict(n_channels=-1, data=DATA, data_kind=7), 'bad channel/offset arguments'),
    (dict(data=DATA, data_kind=7, hist=(1.0, 0.0)), 'data_kind must be'),
    (dict(hist=(1.0, 0.0), shape=i64(-1, 4, 4)), 'hist_hi must be > hist_lo'),
]


@pytest.mark.parametrize('kw,text', RAG_FEATURES_ERRORS)
def test_rag_features_argument_errors(lib, kw, text):
    rc, out = rag_features(lib, **kw)
    fails(lib, rc, ARG, text, out)


# ---------------------------------------------------------------------------
# ctg_rag_blocks
# ---------------------------------------------------------------------------
def block(shape=(2, 4, 8), label_offset=0, data_offset=0, own_begin=(0, 0, 0), own_end=None, graph_begin=(0, 0, 0),
          graph_end=None):
    return dict(shape=shape, label_offset=label_offset, data_offset=data_offset, own_begin=own_begin,
                own_end=shape if own_end is None else own_end, graph_begin=graph_begin,
                graph_end=shape if graph_end is None else graph_end)


def rag_blocks(lib, blocks=(block(),), labels=LABELS, label_bits=64, data=None, data_kind=_lib.CTG_DATA_NONE,
               n_channels=0, offsets=None, n_blocks=None, labels_len=64, data_len=0, hist=(0.0, 1.0), out=True,
               descs=True, start=SENTINEL):
    arr = (_lib.BlockDesc * max(len(blocks), 1))()
    for d, b in zip(arr, blocks):
        d.label_offset, d.data_offset = b['label_offset'], b['data_offset']
        for k in range(3):
            d.shape[k], d.own_begin[k], d.own_end[k] = b['shape'][k], b['own_begin'][k], b['own_end'][k]
            d.graph_begin[k], d.graph_end[k] = b['graph_begin'][k], b['graph_end'][k]
    o = ctypes.c_void_p(start)
    rc = lib.ctg_rag_blocks(ptr(labels), label_bits, ptr(data), data_kind, n_channels, ptr(offsets),
                            ctypes.cast(arr, ctypes.c_void_p) if descs else None,
                            len(blocks) if n_blocks is None else n_blocks, labels_len, data_len, 0, hist[0], hist[1],
                            0, _lib.CTG_MEM_HOST, None, ctypes.byref(o) if out else None)
    return rc, (o if out else None)


# "bad arguments" is the first check: *out is not cleared yet
RAG_BLOCKS_BAD = [dict(out=False), dict(labels=None), dict(descs=False), dict(n_blocks=0), dict(n_blocks=-1),
                  dict(n_blocks=(1 << 20) + 1), dict(labels_len=-1), dict(label_bits=16),
                  dict(data=DATA, data_kind=7, data_len=64), dict(n_channels=-1),
                  dict(n_channels=_lib.CTG_MAX_CHANNELS + 1, offsets=NN), dict(n_channels=3),
                  dict(hist=(1.0, 1.0))]


@pytest.mark.parametrize('kw', RAG_BLOCKS_BAD)
def test_rag_blocks_bad_arguments(lib, kw):
    rc, out = rag_blocks(lib, start=0, **kw)
    fails(lib, rc, ARG, 'ctg_rag_blocks: bad arguments', out)


OUTSIDE = [block(shape=(2, -4, 8)), block(own_begin=(0, -1, 0)), block(own_end=(3, 4, 8)),
           block(own_end=(2, 4, 9)), block(graph_begin=(-1, 0, 0)), block(graph_end=(2, 5, 8)),
           block(shape=(1, 1, 1 << 31), own_end=(0, 0, 0), graph_end=(0, 0, 0))]    # x past the widest array


@pytest.mark.parametrize('bad', OUTSIDE)
def test_rag_blocks_box_outside_its_array(lib, bad):
    rc, out = rag_blocks(lib, blocks=[bad])
    fails(lib, rc, ARG, 'ctg_rag_blocks: block 0: box outside its array', out)
    rc, out = rag_blocks(lib, blocks=[block(), block(), bad])
    fails(lib, rc, ARG, 'ctg_rag_blocks: block 2: box outside its array', out)


def test_rag_blocks_array_outside_the_arena(lib):
    for bad in (block(label_offset=-1), block(label_offset=1), block(shape=(2, 4, 9))):   # 64 / 72 voxels of 64
        rc, out = rag_blocks(lib, blocks=[block(), bad])
        fails(lib, rc, ARG, 'ctg_rag_blocks: block 1: array outside the arena', out)
    # the data arena: boundary map (one value a voxel), affinities (n_channels a voxel)
    for kw in (dict(blocks=[block(data_offset=-1)], data_len=64), dict(blocks=[block()], data_len=63),
               dict(blocks=[block()], data_len=191, n_channels=3, offsets=NN)):
        rc, out = rag_blocks(lib, data=DATA, data_kind=_lib.CTG_DATA_F32, **kw)
        fails(lib, rc, ARG, 'ctg_rag_blocks: block 0: array outside the arena', out)


def test_rag_blocks_error_order(lib):
    # bad arguments before any block; within a block the box before the arena; blocks in order
    rc, out = rag_blocks(lib, blocks=[block(own_end=(3, 4, 8))], label_bits=16, start=0)
    fails(lib, rc, ARG, 'ctg_rag_blocks: bad arguments', out)
    rc, out = rag_blocks(lib, blocks=[block(own_end=(3, 4, 8), label_offset=-1)])
    fails(lib, rc, ARG, 'block 0: box outside its array', out)
    rc, out = rag_blocks(lib, blocks=[block(label_offset=1), block(own_end=(3, 4, 8))])
    fails(lib, rc, ARG, 'block 0: array outside the arena', out)


# ---------------------------------------------------------------------------
# unique / merge / map entry points
# ---------------------------------------------------------------------------
def with_out(fn, *args, start=SENTINEL, out=True):
    o = ctypes.c_void_p(start)
    return fn(*args, ctypes.byref(o) if out else None), (o if out else None)


def test_unique_labels_argument_errors(lib):
    f = lib.ctg_unique_labels
    for args, kw in (((None, ptr(SHAPE), None, None, 0, None), dict(start=0)),
                     ((ptr(LABELS), None, None, None, 0, None), dict(start=0)),
                     ((ptr(LABELS), ptr(SHAPE), None, None, 0, None), dict(out=False))):
        rc, out = with_out(f, *args, **kw)
        fails(lib, rc, ARG, 'ctg_unique_labels: null argument', out)
    for b, e in ((i64(0, -1, 0), None), (None, i64(4, 4, 5)), (i64(0, 3, 0), i64(4, 2, 4))):
        rc, out = with_out(f, ptr(LABELS), ptr(SHAPE), ptr(b), ptr(e), 0, None)
        fails(lib, rc, ARG, 'ctg_unique_labels: box outside the array', out)
    # a negative extent: the default end lies below the default begin
    rc, out = with_out(f, ptr(LABELS), ptr(i64(4, -1, 4)), None, None, 0, None)
    fails(lib, rc, ARG, 'ctg_unique_labels: box outside the array', out)


def test_unique_values_and_pairs_argument_errors(lib):
    for name in ('ctg_unique_values', 'ctg_unique_pairs'):
        f = getattr(lib, name)
        for args, kw in (((ptr(LABELS), 4, 0, None), dict(out=False)), ((ptr(LABELS), -1, 0, None), dict(start=0)),
                         ((None, 4, 0, None), dict(start=0))):
            rc, out = with_out(f, *args, **kw)
            fails(lib, rc, ARG, name + ': bad arguments', out)


def test_merge_stats_argument_errors(lib):
    k, s, r = ptr(LABELS), ptr(np.zeros(8)), ptr(np.zeros(64, dtype=np.uint32))
    for args, kw in (((k, s, r, 1), dict(out=False)), ((k, s, r, -1), dict(start=0)), ((None, s, r, 1), dict(start=0)),
                     ((k, None, r, 1), dict(start=0)), ((k, s, None, 1), dict(start=0))):
        rc, out = with_out(lib.ctg_merge_stats, *args, 0.0, 1.0, 0, 0, None, **kw)
        fails(lib, rc, ARG, 'ctg_merge_stats: bad arguments', out)


def test_merge_feature_rows_argument_errors(lib):
    f = lib.ctg_merge_feature_rows
    ids, rows, out = ptr(LABELS), ptr(np.zeros(40)), ptr(np.zeros(40))
    for args in ((ids, rows, -1, 0, 4, out), (ids, rows, 4, 5, 4, out), (None, rows, 4, 0, 4, out),
                 (ids, None, 4, 0, 4, out), (ids, rows, 4, 0, 4, None)):
        fails(lib, f(*args, 0, None), ARG, 'ctg_merge_feature_rows: bad arguments')
    for args in ((ids, rows, 4, 0, 1 << 32, out), (ids, rows, 1 << 32, 0, 4, out)):
        fails(lib, f(*args, 0, None), UNSUPPORTED, 'ctg_merge_feature_rows: more than 2^32 edges or rows in one call')
    # both at once: the argument check comes first
    fails(lib, f(ids, rows, -1, 0, 1 << 32, out, 0, None), ARG, 'ctg_merge_feature_rows: bad arguments')
    assert f(ids, rows, 0, 7, 7, None, 0, None) == 0      # an empty id range: nothing to do


def test_map_edge_ids_argument_errors(lib):
    f = lib.ctg_map_edge_ids
    g, q, o = ptr(LABELS), ptr(LABELS), ptr(np.zeros(4, dtype=np.int64))
    for args in ((g, -1, q, 2, o), (g, 2, q, -1, o), (g, 2, None, 2, o), (g, 2, q, 2, None)):
        fails(lib, f(*args, 0, None), ARG, 'ctg_map_edge_ids: bad arguments')
    assert f(g, 2, None, 0, None, 0, None) == 0           # no query


# ---------------------------------------------------------------------------
# label overlaps and morphology
# ---------------------------------------------------------------------------
HUGE = i64(1 << 11, 1 << 11, 1 << 10)    # 2^32 voxels: never read, the box check comes first


def test_label_overlaps_argument_errors(lib):
    def call(labels=LABELS, lbits=64, values=LABELS, vbits=64, shape=SHAPE, begin=None, end=None, **kw):
        return with_out(lib.ctg_label_overlaps, ptr(labels), lbits, ptr(values), vbits, ptr(shape), ptr(begin),
                        ptr(end), 0, 0, 0, None, **kw)
    for kw in (dict(labels=None, start=0), dict(values=None, start=0), dict(shape=None, start=0), dict(out=False)):
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_label_overlaps: null argument', out)
    for kw in (dict(lbits=16), dict(vbits=8), dict(lbits=16, begin=i64(0, 0, -1))):    # the bits before the box
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_label_overlaps: label_bits and value_bits must be 32 or 64', out)
    for kw in (dict(shape=i64(4, -4, 4)), dict(begin=i64(-1, 0, 0)), dict(end=i64(4, 4, 5)),
               dict(begin=i64(0, 2, 0), end=i64(4, 1, 4)), dict(shape=HUGE, end=i64(1 << 11, 1 << 11, (1 << 10) + 1))):
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_label_overlaps: box outside the array', out)
    # 2^32 voxels, and the smallest refused box: 3 * 5 * 286331153 = 2^32 - 1 (a smaller one would go on to the GPU)
    for shape in (HUGE, i64(3, 5, 286331153)):
        rc, out = call(shape=shape)
        fails(lib, rc, UNSUPPORTED, 'ctg_label_overlaps: boxes of 2^32 voxels or more are not supported', out)


def test_merge_overlaps_and_morphology_argument_errors(lib):
    p, c = ptr(LABELS), ptr(LABELS)
    for args, kw in (((p, c, 2), dict(out=False)), ((p, c, -1), dict(start=0)), ((None, c, 2), dict(start=0)),
                     ((p, None, 2), dict(start=0))):
        rc, out = with_out(lib.ctg_merge_overlaps, *args, 0, None, **kw)
        fails(lib, rc, ARG, 'ctg_merge_overlaps: bad arguments', out)
    rc, out = with_out(lib.ctg_merge_overlaps, p, c, (1 << 32) - 1, 0, None)
    fails(lib, rc, UNSUPPORTED, 'ctg_merge_overlaps: 2^32 rows or more in one call', out)
    rows = ptr(np.zeros(_lib.CTG_MORPH_COLS))
    for args, kw in (((rows, 1), dict(out=False)), ((rows, -1), dict(start=0)), ((None, 1), dict(start=0))):
        rc, out = with_out(lib.ctg_merge_morphology, *args, 0, None, **kw)
        fails(lib, rc, ARG, 'ctg_merge_morphology: bad arguments', out)
    rc, out = with_out(lib.ctg_merge_morphology, rows, (1 << 32) - 1, 0, None)
    fails(lib, rc, UNSUPPORTED, 'ctg_merge_morphology: 2^32 rows or more in one call', out)


def test_morphology_argument_errors(lib):
    def call(labels=LABELS, bits=64, shape=SHAPE, begin=None, end=None, origin=None, **kw):
        return with_out(lib.ctg_morphology, ptr(labels), bits, ptr(shape), ptr(begin), ptr(end), ptr(origin), 0, None,
                        **kw)
    for kw in (dict(labels=None, start=0), dict(shape=None, start=0), dict(out=False)):
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_morphology: null argument', out)
    for kw in (dict(bits=16), dict(bits=16, end=i64(4, 4, 5))):
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_morphology: label_bits must be 32 or 64', out)
    # the whole box is checked before the origin: a call wrong in both names the box
    for kw in (dict(shape=i64(-4, 4, 4)), dict(begin=i64(0, -1, 0)), dict(end=i64(5, 4, 4)),
               dict(begin=i64(3, 0, 0), end=i64(2, 4, 4)), dict(end=i64(4, 4, 5), origin=i64(-1, 0, 0))):
        rc, out = call(**kw)
        fails(lib, rc, ARG, 'ctg_morphology: box outside the array', out)
    rc, out = call(shape=HUGE)
    fails(lib, rc, UNSUPPORTED, 'ctg_morphology: boxes of 2^32 voxels or more are not supported', out)
    rc, out = call(shape=HUGE, origin=i64(-1, 0, 0))       # the box size before the origin, too
    fails(lib, rc, UNSUPPORTED, 'ctg_morphology: boxes of 2^32 voxels or more are not supported', out)
    for origin in (i64(-1, 0, 0), i64(0, 1 << 31, 0), i64(0, 0, (1 << 31) - 4)):
        rc, out = call(origin=origin)
        fails(lib, rc, ARG, 'ctg_morphology: origin + end must stay below 2^31 on every axis (origin >= 0)', out)


def test_table_readers_without_a_result(lib):
    """ctg_max_overlaps and ctg_morphology_rows refuse a null handle (their
    other checks need a result, so a GPU)."""
    o = ptr(np.zeros(4, dtype=np.uint64))
    fails(lib, lib.ctg_max_overlaps(None, 0, 4, o, o, 0, None), ARG, 'ctg_max_overlaps: bad arguments')
    d = ptr(np.zeros(4 * _lib.CTG_MORPH_COLS))
    fails(lib, lib.ctg_morphology_rows(None, 0, 4, d, None, 0, None), ARG, 'ctg_morphology_rows: bad arguments')


# ---------------------------------------------------------------------------
# multi-GPU exchange
# ---------------------------------------------------------------------------
def test_mgpu_slab_argument_errors(lib):
    f = lib.ctg_mgpu_slab
    out = np.zeros(3, dtype=np.int64)
    off = np.array([[-2, 0, 0], [0, -1, 0]], dtype=np.int64)
    for args in ((0, 2, 0, ptr(off), 2, ptr(out)), (8, 0, 0, ptr(off), 2, ptr(out)), (8, 2, -1, ptr(off), 2, ptr(out)),
                 (8, 2, 2, ptr(off), 2, ptr(out)), (8, 2, 0, ptr(off), 2, None), (8, 2, 0, ptr(off), -1, ptr(out)),
                 (8, 2, 0, None, 2, ptr(out)), (1, 2, 5, None, 0, ptr(out))):     # the last: also more ranks than planes
        fails(lib, f(*args), ARG, 'ctg_mgpu_slab: invalid arguments')
    fails(lib, f(3, 4, 0, ptr(off), 2, ptr(out)), ARG, 'ctg_mgpu_slab: more ranks than z planes')
    up = np.array([[1, 0, 0]], dtype=np.int64)
    fails(lib, f(8, 2, 0, ptr(up), 1, ptr(out)), UNSUPPORTED,
          'ctg_mgpu_slab: positive z offsets need an upper halo, which the z-slab layout does not have')
    fails(lib, f(1, 2, 0, ptr(up), 1, ptr(out)), ARG, 'ctg_mgpu_slab: more ranks than z planes')   # ranks first
    assert f(8, 1, 0, ptr(up), 1, ptr(out)) == 0 and list(out) == [0, 0, 8]      # one rank needs no halo
    assert f(8, 2, 1, ptr(off), 2, ptr(out)) == 0 and list(out) == [2, 4, 8]     # halo of 2 planes below z0 = 4


def test_mgpu_calls_without_a_table(lib):
    """The checks of the exchange that need no result handle: a null table (and,
    with it, whatever else is wrong) is "bad arguments" with the world range."""
    buf = ptr(np.zeros(64, dtype=np.int64))
    tail = ': bad arguments (world size must be 1..%d)' % _lib.CTG_MGPU_MAX_WORLD
    fails(lib, lib.ctg_mgpu_sample(None, buf, None), ARG, 'ctg_mgpu_sample' + tail)
    fails(lib, lib.ctg_mgpu_split(None, buf, 2, buf, None), ARG, 'ctg_mgpu_split' + tail)
    fails(lib, lib.ctg_mgpu_split(None, buf, 0, buf, None), ARG, 'ctg_mgpu_split' + tail)
    fails(lib, lib.ctg_mgpu_pack(None, buf, 2, 0, buf, None), ARG, 'ctg_mgpu_pack' + tail)
    fails(lib, lib.ctg_mgpu_pack(None, buf, _lib.CTG_MGPU_MAX_WORLD + 1, 0, buf, None), ARG, 'ctg_mgpu_pack' + tail)
    rc, out = with_out(lib.ctg_mgpu_merge, None, buf, buf, 2, 0, 0.0, 1.0, None, start=0)
    fails(lib, rc, ARG, 'ctg_mgpu_merge' + tail, out)
