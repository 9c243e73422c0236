"""Region features without a GPU: the numpy oracle the GPU tests compare with
(pinned by a hand-computed case), the block-chunk format of
cluster_tools_amd.features, the summation bound the inexact comparisons use, and
every argument error of the C ABI, which precedes any GPU work."""
import ctypes
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import _lib, features, n5, rag
from tests import chunk_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -53


# ------------------------------------------------------------------- oracle
def region_table(labels, data, ignore_label=None):
    """dict(nodes (N,) uint64, counts (N,) uint64, sums (N,) float64, minmax
    (N,2) float32, abs_sums (N,) float64) of a label array over a data array
    (float32 or uint8): np.unique with inverse after the ignore mask,
    np.bincount with float64 weights, np.minimum.at / np.maximum.at.  Voxels
    whose label equals ``ignore_label`` are not counted."""
    lab = np.asarray(labels).astype(np.uint64).ravel()
    x = np.asarray(data).ravel()
    assert x.dtype in (np.float32, np.uint8) and x.shape == lab.shape
    if ignore_label is not None:
        keep = lab != np.uint64(ignore_label)
        lab, x = lab[keep], x[keep]
    nodes, inv = np.unique(lab, return_inverse=True)
    inv = inv.ravel()
    n = nodes.shape[0]
    xf = x.astype(np.float32)
    mn, mx = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
    np.minimum.at(mn, inv, xf)
    np.maximum.at(mx, inv, xf)
    w = x.astype(np.float64)
    return dict(nodes=nodes, counts=np.bincount(inv, minlength=n).astype(np.uint64),
                sums=np.bincount(inv, weights=w, minlength=n).astype(np.float64),
                minmax=np.stack([mn, mx], 1).reshape(n, 2),
                abs_sums=np.bincount(inv, weights=np.abs(w), minlength=n).astype(np.float64))


def sum_rows(t):
    """(N,5) float64 rows [id, count, sum, min, max]."""
    return np.column_stack([t['nodes'].astype(np.float64), t['counts'].astype(np.float64), t['sums'],
                            t['minmax'].astype(np.float64)]).reshape(-1, 5)


def feature_rows(t, norm):
    """(N,5) float64 rows [id, count, mean, minimum, maximum]: mean =
    (sum / count) / norm, the two divisions the library makes, in its order."""
    n = t['counts'].astype(np.float64)
    return np.column_stack([t['nodes'].astype(np.float64), n, (t['sums'] / n) / norm,
                            t['minmax'].astype(np.float64) / norm]).reshape(-1, 5)


def dense_rows(rows, label_begin, label_end):
    """Rows scattered by id over [label_begin, label_end), zeros elsewhere."""
    out = np.zeros((label_end - label_begin, 5), np.float64)
    ids = rows[:, 0].astype(np.int64)
    sel = (ids >= label_begin) & (ids < label_end)
    out[ids[sel] - label_begin] = rows[sel]
    return out


def sum_bound(counts, abs_sums):
    """Largest difference of two summation orders of n float64 terms:
    2 (n - 1) 2^-53 sum|x| (each order is within (n - 1) 2^-53 sum|x| of the
    true sum to first order)."""
    return 2.0 * (counts.astype(np.float64) - 1.0) * U * abs_sums


@pytest.fixture(scope='module')
def kat():
    with open(os.path.join(GOLD, 'region_features_kat.json')) as fh:
        return json.load(fh)


def kat_inputs(kat, variant):
    labels = np.array(kat['labels'], np.uint64)
    k = np.array(kat['data_eighths'])
    data = (k * kat['u8_factor']).astype(np.uint8) if variant.startswith('u8') else (k / 8.0).astype(np.float32)
    return labels, data, (kat['ignore_label'] if variant.endswith('ignore') else None)


def check_against_kat(t, rows, feats, want):
    np.testing.assert_array_equal(t['nodes'], np.array(want['nodes'], np.uint64))
    np.testing.assert_array_equal(t['counts'], np.array(want['counts'], np.uint64))
    np.testing.assert_array_equal(t['sums'], np.array(want['sums'], np.float64))
    np.testing.assert_array_equal(t['minmax'], np.array(want['minmax'], np.float32))
    np.testing.assert_array_equal(rows, np.array(want['rows'], np.float64))
    np.testing.assert_array_equal(feats, np.array(want['features'], np.float64))


@pytest.mark.parametrize('variant', ['f32', 'f32_ignore', 'u8', 'u8_ignore'])
def test_oracle_matches_hand_computed_case(kat, variant):
    labels, data, ignore = kat_inputs(kat, variant)
    assert labels.shape == (2, 3, 4)
    want = kat[variant]
    t = region_table(labels, data, ignore)
    check_against_kat(t, sum_rows(t), feature_rows(t, want['norm']), want)
    assert t['nodes'][0] == 0 and t['counts'][1] == 1                     # label 0 has a row; the single voxel
    assert (t['minmax'][1, 0] == t['minmax'][1, 1]) and t['sums'][1] == t['minmax'][1, 0]
    assert int(t['counts'].sum()) == labels.size - (7 if ignore is not None else 0)
    assert (kat['ignore_label'] in t['nodes'].tolist()) == (ignore is None)
    if variant.startswith('f32'):
        key = 'dense_features_' + variant
        np.testing.assert_array_equal(dense_rows(feature_rows(t, 1.0), *kat['label_range']),
                                      np.array(kat[key], np.float64))
        assert not np.array(kat[key])[0].any() and np.array(kat[key])[1, 1] == 1


def test_oracle_of_nothing():
    t = region_table(np.zeros((2, 2, 2), np.uint64), np.ones((2, 2, 2), np.float32), ignore_label=0)
    assert t['nodes'].shape == (0,) and t['minmax'].shape == (0, 2) and sum_rows(t).shape == (0, 5)


# ------------------------------------------------------------- chunk format
def test_chunk_words_of_hand_computed_case(kat):
    rows = np.array(kat['f32']['rows'], np.float64)
    words = features.encode_region_chunk(rows)
    assert words.dtype == np.float64 and words.ndim == 1
    np.testing.assert_array_equal(words, np.array(kat['chunk_f32'], np.float64))
    np.testing.assert_array_equal(features.decode_region_chunk(words), rows)
    np.testing.assert_array_equal(features.encode_region_chunk(np.array(kat['u8_ignore']['rows'])),
                                  np.array(kat['chunk_u8_ignore'], np.float64))
    assert features.encode_region_chunk(np.zeros((0, 5))).size == 0
    assert features.decode_region_chunk(np.zeros(0)).shape == (0, 5)
    with pytest.raises(RuntimeError, match='truncated'):
        features.decode_region_chunk(words[:-1])
    with pytest.raises(ValueError, match='columns'):
        features.encode_region_chunk(np.zeros((3, 4)))
    assert features.FEATURE_NAMES == ['count', 'mean', 'minimum', 'maximum']


def test_chunk_round_trip_through_n5(tmp_path, kat):
    rows = np.array(kat['f32']['rows'], np.float64)
    rows[0, 0] = 2.0 ** 40 + 1                                            # an id and a count no float32 holds
    rows[0, 1] = 2.0 ** 24 + 1
    path = str(tmp_path / 'r.n5')
    with n5.file_reader(path) as f:
        ds = f.require_dataset('block_feats', shape=(40, 48, 140), chunks=(16, 24, 70), dtype='float64',
                               compression='gzip')
        ds.write_chunk((2, 1, 0), features.encode_region_chunk(rows), True)
        ds.attrs['feature_names'] = features.FEATURE_NAMES
        ds.attrs['norm'] = 255.0
    with n5.file_reader(path, 'r') as f:
        ds = f['block_feats']
        got = ds.read_chunks([(2, 1, 0), (0, 0, 0)])
        assert ds.attrs['feature_names'] == ['count', 'mean', 'minimum', 'maximum'] and ds.attrs['norm'] == 255.0
        raw = ds.read_chunk((2, 1, 0))
    np.testing.assert_array_equal(features.decode_region_chunk(got[0]), rows)
    assert got[1] is None
    with pytest.raises(RuntimeError, match='truncated'):
        features.decode_region_chunk(raw[:-2])


# ------------------------------------------------------ the summation bound
def test_summation_orders_stay_within_the_bound():
    """10^4 seeded sets of 1 .. 4096 float32 samples in [0,1]: the float64 sum
    in forward, reversed and pairwise order differs by no more than
    2 (n - 1) 2^-53 sum|x|."""
    rng = np.random.default_rng(31)
    sizes = rng.integers(1, 4097, size=10000)
    sizes[:4] = [1, 2, 4096, 4095]
    worst = 0.0
    for n in sizes:
        # (fourth powers: exponents down to 2^-60 or so -- uniform float32 draws are multiples of
        # 2^-24, whose sums are exact)
        x = (rng.random(int(n)) ** 4).astype(np.float32).astype(np.float64)
        assert 0.0 <= x.min() and x.max() <= 1.0
        fwd = float(np.cumsum(x)[-1])                                     # strictly left to right
        rev = float(np.cumsum(x[::-1])[-1])
        pair = float(np.sum(x))                                           # numpy's pairwise sum
        bound = 2.0 * (n - 1) * U * float(np.abs(x).sum())
        for a, b in ((fwd, rev), (fwd, pair), (rev, pair)):
            assert abs(a - b) <= bound, (n, a, b, bound)
            worst = max(worst, abs(a - b) / bound if bound else 0.0)
    assert 0.0 < worst <= 1.0


def test_exactly_summable_data_has_one_sum():
    """k / 256 samples, k in [0, 256]: every partial sum of 2^32 of them is a
    multiple of 2^-8 below 2^53 2^-8, so every order gives the same bits."""
    rng = np.random.default_rng(32)
    x = (rng.integers(0, 257, size=4096) / 256.0).astype(np.float32).astype(np.float64)
    assert float(np.cumsum(x)[-1]) == float(np.cumsum(x[::-1])[-1]) == float(np.sum(x))


# --------------------------------------------------- checks before the device
def _lib_or_skip():
    return _lib.load()


def _err():
    return _lib.load().ctg_last_error().decode()


def _arr3(v):
    return (ctypes.c_int64 * 3)(*v)


def test_c_abi_argument_errors_need_no_gpu():
    """Every argument error of ctg_region_features, ctg_merge_region_features,
    ctg_region_rows and ctg_result_copy_region: its status, its message, and
    *out null."""
    lib = _lib_or_skip()
    lab = np.zeros((2, 3, 4), np.uint64)
    dat = np.zeros((2, 3, 4), np.float32)
    pl, pd = lab.ctypes.data_as(ctypes.c_void_p), dat.ctypes.data_as(ctypes.c_void_p)
    shape = _arr3(lab.shape)
    ARG, UNSUP = -1, -4

    def region(labels=pl, bits=64, data=pd, kind=_lib.CTG_DATA_F32, shp=shape, begin=None, end=None, mem=0,
               no_out=False):
        h = ctypes.c_void_p(0xDEAD)
        rc = lib.ctg_region_features(labels, bits, data, kind, shp, begin, end, 0, 0, mem, None,
                                     None if no_out else ctypes.byref(h))
        return rc, h.value, _err()

    for kw, status, text in (
            (dict(labels=None), ARG, 'null'), (dict(data=None), ARG, 'null'), (dict(shp=None), ARG, 'null'),
            (dict(bits=16), ARG, 'label_bits'), (dict(kind=_lib.CTG_DATA_NONE), ARG, 'data_kind'),
            (dict(kind=7), ARG, 'data_kind'), (dict(mem=5), ARG, 'mem'),
            (dict(end=_arr3((3, 3, 4))), ARG, 'outside'), (dict(begin=_arr3((1, 0, 0)), end=_arr3((0, 3, 4))), ARG,
                                                           'outside'),
            (dict(begin=_arr3((0, -1, 0))), ARG, 'outside'),
            (dict(shp=_arr3((1 << 11, 1 << 11, 1 << 10))), UNSUP, '2^32')):
        rc, h, msg = region(**kw)
        assert rc == status and text in msg and 'ctg_region_features' in msg, (kw, rc, msg)
        assert h is None, kw                                              # *out = NULL
    rc, _, msg = region(no_out=True)
    assert rc == ARG and 'null' in msg

    def merge(rows, n, no_out=False):
        h = ctypes.c_void_p(0xDEAD)
        rc = lib.ctg_merge_region_features(rows, n, 0, None, None if no_out else ctypes.byref(h))
        return rc, h.value, _err()

    r5 = np.zeros((1, 5))
    p5 = r5.ctypes.data_as(ctypes.c_void_p)
    for args, status, text in (((p5, -1), ARG, 'bad arguments'), ((None, 3), ARG, 'bad arguments'),
                               ((p5, 0xFFFFFFFF), UNSUP, '2^32 rows')):
        rc, h, msg = merge(*args)
        assert rc == status and text in msg and 'ctg_merge_region_features' in msg, (args, rc, msg)
        assert h is None
    rc, _, msg = merge(p5, 1, no_out=True)
    assert rc == ARG and 'bad arguments' in msg

    out = np.zeros((4, 5))
    po = out.ctypes.data_as(ctypes.c_void_p)
    blank = ctypes.create_string_buffer(4096)                             # a handle of nothing: all its tables null
    hb = ctypes.cast(blank, ctypes.c_void_p)
    for args, text in (((None, 0, 4, 1, 1.0), 'bad arguments'), ((hb, 5, 4, 1, 1.0), 'bad arguments'),
                       ((hb, 0, 4, 2, 1.0), 'form'), ((hb, 0, 4, -1, 1.0), 'form'),
                       ((hb, 0, 4, 1, 0.0), 'norm'), ((hb, 0, 4, 1, -255.0), 'norm'),
                       ((hb, 0, 4, 1, float('nan')), 'norm'), ((hb, 0, 4, 0, float('inf')), 'norm'),
                       ((hb, 0, 4, 1, 1.0), 'not a region-features result'),
                       ((hb, 0, (1 << 40) + 1, 1, 1.0), 'not a region-features result')):
        rc = lib.ctg_region_rows(*args, po, None, 0, None)
        assert rc == ARG and text in _err() and 'ctg_region_rows' in _err(), (args, rc, _err())
    assert not out.any()
    assert lib.ctg_result_copy_region(hb, None, None, None, 0) == ARG and 'region' in _err()
    assert lib.ctg_result_copy_region(None, None, None, None, 0) == ARG and 'region' in _err()


def test_python_argument_checks():
    a = np.zeros((2, 3, 4), np.uint64)
    d = np.zeros((2, 3, 4), np.float32)
    with pytest.raises(ValueError, match='3-D'):
        rag.region_features(a[0], d[0])
    with pytest.raises(TypeError, match='integer'):
        rag.region_features(a.astype(np.float32), d)
    with pytest.raises(TypeError, match='float32 or uint8'):
        rag.region_features(a, d.astype(np.float64))
    with pytest.raises(ValueError, match='data shape'):
        rag.region_features(a, d[:, :, :3])
    with pytest.raises(ValueError, match='3 entries'):
        rag.region_features(a, d, begin=(0, 0))
    with pytest.raises(ValueError, match='ignore_label'):
        rag.region_features(a, d, ignore_label=-1)
    with pytest.raises(ValueError, match='columns'):
        rag.merge_region_features(np.zeros((3, 4)))
    with pytest.raises(ValueError, match='columns'):
        rag.merge_region_features(np.zeros(12))
    with pytest.raises(ValueError, match='label_begin'):
        rag.region_feature_rows(dict(rows=np.zeros((0, 5))), 5, 4)
    with pytest.raises(ValueError, match='form'):
        rag.region_feature_rows(dict(rows=np.zeros((0, 5))), 0, 4, form='mean')
    with pytest.raises(ValueError, match='norm'):
        rag.region_feature_rows(dict(rows=np.zeros((0, 5))), 0, 4, norm=0.0)
    with pytest.raises(ValueError, match='Invalid feature name'):
        features.mergeAndSerializeRegionFeatures('x', 'y', 'z', 'w', 0, 4, featureNames=('count', 'variance'))


# ------------------------------------------------- the chunk loop of the merge
def _rows_of(ids):
    """One row per id, told apart by its count column."""
    rows = np.zeros((len(ids), 5), np.float64)
    rows[:, 0] = ids
    rows[:, 1] = 100 + np.arange(len(ids))
    return rows


@pytest.fixture
def region_chunks(tmp_path):
    path = str(tmp_path / 'r.n5')
    K.block_dataset(path, 'blocks', 'float64', lambda ids: features.encode_region_chunk(_rows_of(ids)))
    K.output_dataset(path, 'out', (K.N_OUT, 2), 'float32')
    return path


@pytest.mark.parametrize('norm', [None, 255.0])
def test_merge_reads_the_rows_of_its_range_and_writes_the_slice(region_chunks, monkeypatch, norm):
    if norm is not None:
        with n5.file_reader(region_chunks) as f:
            f['blocks'].attrs['norm'] = norm
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_region_features_handle', handle)
    dense = np.arange(4 * 5, dtype=np.float64).reshape(4, 5) + 0.5
    read = K.capture(monkeypatch, rag, 'region_feature_rows', dense)
    features.mergeAndSerializeRegionFeatures(region_chunks, 'blocks', region_chunks, 'out', K.BEGIN, K.END,
                                             featureNames=('maximum', 'count'), numberOfThreads=2)
    ((rows,), kw), = merged
    mixed = _rows_of(K.MIXED_IDS)
    assert not kw and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, mixed[[K.MIXED_IDS.index(a) for a in K.IN_RANGE]])
    (args, kw), = read
    assert args[0] is handle and list(args[1:]) + list(kw.values()) == [K.BEGIN, K.END, 'features', norm or 1.0]
    assert handle.freed == 1
    out = np.zeros((K.N_OUT, 2), np.float32)
    out[K.BEGIN:K.END] = dense[:, [4, 1]].astype(np.float32)
    got = K.read_output(region_chunks, 'out')
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, out)


def test_merge_of_an_empty_range_gets_an_empty_table(region_chunks, monkeypatch):
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_region_features_handle', handle)
    K.capture(monkeypatch, rag, 'region_feature_rows', np.zeros((0, 5)))
    features.mergeAndSerializeRegionFeatures(region_chunks, 'blocks', region_chunks, 'out', 12, 12)
    ((rows,), _), = merged
    assert rows.shape == (0, 5) and rows.dtype == np.float64 and handle.freed == 1


def test_block_features_write_their_chunk_unless_empty_and_always_the_attributes(tmp_path, monkeypatch):
    rows = _rows_of([4, 5])
    lab = np.zeros((1, 1, 2), np.uint64)
    for k, (handle, data, norm, ignore) in enumerate((
            (K.Handle(n_nodes=2, region_rows=rows), np.zeros((1, 1, 2), np.uint8), 255.0, 0),
            (K.Handle(n_nodes=0), np.zeros((1, 1, 2), np.uint8), 255.0, None),
            (K.Handle(n_nodes=0), np.zeros((1, 1, 2), np.float32), 1.0, None))):
        path = str(tmp_path / ('b%d.n5' % k))
        K.output_dataset(path, 'blocks', (1, 1, 3), 'float64', chunks=(1, 1, 1))
        made = K.capture(monkeypatch, rag, 'region_features_handle', handle)
        features.computeAndSerializeRegionFeatures(lab, data, path, 'blocks', (0, 0, 1), ignoreLabel=ignore)
        (args, kw), = made
        assert args[0] is lab and args[1] is data and list(args[2:]) + list(kw.values()) == [ignore]
        assert handle.freed == 1
        with n5.file_reader(path, 'r') as f:
            assert f['blocks'].attrs['feature_names'] == features.FEATURE_NAMES and f['blocks'].attrs['norm'] == norm
        got = K.chunk_of(path, 'blocks', (0, 0, 1))
        if handle.n_nodes:
            np.testing.assert_array_equal(got, rows.reshape(-1))
        else:
            assert got is None
