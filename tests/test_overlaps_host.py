"""Label overlaps without a GPU: the numpy oracle the GPU tests compare with
(checked here against a hand-computed case), the overlap-chunk format of the
ndist mirror, and the argument checks the Python layer makes before it touches
the device."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import n5, ndist, rag
from tests import chunk_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ------------------------------------------------------------------- oracle
def overlap_table(a, b, ignore_label=None):
    """(pairs (E,2), counts (E,)) of the voxelwise pairs (a[p], b[p]), sorted;
    voxels with b == ignore_label left out."""
    a = np.asarray(a).astype(np.uint64).ravel()
    b = np.asarray(b).astype(np.uint64).ravel()
    if ignore_label is not None:
        keep = b != np.uint64(ignore_label)
        a, b = a[keep], b[keep]
    if a.size == 0:
        return np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)
    pairs, counts = np.unique(np.stack([a, b], 1), axis=0, return_counts=True)
    return pairs, counts.astype(np.uint64)


def max_overlap(pairs, counts, label_begin, label_end):
    """Per label in [label_begin, label_end): (value of the largest count --
    the smallest such value, count, tie flag), zeros for labels without rows."""
    n = label_end - label_begin
    lab, cnt, tie = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, bool)
    for (a, b), c in zip(pairs.tolist(), counts.tolist()):   # rows ascend in (a, b)
        if not label_begin <= a < label_end:
            continue
        k = a - label_begin
        if c > cnt[k]:
            lab[k], cnt[k], tie[k] = b, c, False
        elif c == cnt[k]:
            tie[k] = True
    return lab, cnt, tie


def table_dict(pairs, counts):
    out = {}
    for (a, b), c in zip(np.asarray(pairs).tolist(), np.asarray(counts).tolist()):
        out.setdefault(a, {})[b] = c
    return out


@pytest.fixture(scope='module')
def kat():
    with open(os.path.join(GOLD, 'overlaps_kat.json')) as fh:
        return json.load(fh)


def test_oracle_matches_hand_computed_case(kat):
    a, b = np.array(kat['labels'], np.uint64), np.array(kat['values'], np.uint64)
    assert a.shape == b.shape == (2, 2, 3)
    pairs, counts = overlap_table(a, b)
    np.testing.assert_array_equal(pairs, np.array(kat['pairs'], np.uint64))
    np.testing.assert_array_equal(counts, np.array(kat['counts'], np.uint64))
    assert int(counts.sum()) == a.size
    np.testing.assert_array_equal(np.unique(pairs[:, 0]), kat['nodes'])
    lab, cnt, tie = max_overlap(pairs, counts, *kat['label_range'])
    np.testing.assert_array_equal(lab, kat['max_labels'])
    np.testing.assert_array_equal(cnt, kat['max_counts'])
    np.testing.assert_array_equal(np.flatnonzero(tie) + kat['label_range'][0], kat['tie_nodes'])
    # the tie of node 1 (values 5 and 6, two voxels each) goes to the smaller value
    assert lab[1] == 5 and tie[1]
    pairs, counts = overlap_table(a, b, kat['ignore_label'])
    np.testing.assert_array_equal(pairs, np.array(kat['pairs_ignore'], np.uint64))
    np.testing.assert_array_equal(counts, np.array(kat['counts_ignore'], np.uint64))


def test_oracle_label_range_above_zero(kat):
    pairs, counts = np.array(kat['pairs'], np.uint64), np.array(kat['counts'], np.uint64)
    lab, cnt, _ = max_overlap(pairs, counts, 2, 9)
    np.testing.assert_array_equal(lab, [5, 7, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(cnt, [2, 3, 1, 0, 0, 0, 0])


# ------------------------------------------------------------- chunk format
def test_chunk_words_of_hand_computed_case(kat):
    pairs, counts = np.array(kat['pairs'], np.uint64), np.array(kat['counts'], np.uint64)
    words = ndist.encode_overlap_chunk(pairs, counts)
    assert words.dtype == np.uint64
    np.testing.assert_array_equal(words, kat['chunk'])
    p2, c2 = ndist.decode_overlap_chunk(words)
    np.testing.assert_array_equal(p2, pairs)
    np.testing.assert_array_equal(c2, counts)
    assert ndist.encode_overlap_chunk(np.zeros((0, 2), np.uint64), np.zeros(0, np.uint64)).size == 0
    p0, c0 = ndist.decode_overlap_chunk(np.zeros(0, np.uint64))
    assert p0.shape == (0, 2) and c0.shape == (0,)
    with pytest.raises(RuntimeError, match='truncated'):
        ndist.decode_overlap_chunk(words[:-1])


def test_chunk_round_trip_through_n5(tmp_path):
    """encode -> varlen N5 chunk -> deserializeOverlapChunk, with labels and
    counts past 2^32, in the three-argument form, the two-argument
    (dataset path, chunkId) form and for a chunk that does not exist."""
    big = 1 << 40
    pairs = np.array([[0, 7], [3, 1], [3, big + 2], [9, 0], [big, 5], [(1 << 63) + 1, (1 << 63) + 2]], np.uint64)
    counts = np.array([4, 1, 3 * 10 ** 9, 2, 6 * 10 ** 9, 1], np.uint64)
    path = str(tmp_path / 'ol.n5')
    with n5.file_reader(path) as f:
        ds = f.require_dataset('tmp/label_overlaps_', shape=(40, 60, 70), chunks=(32, 32, 32), dtype='uint64',
                               compression='gzip')
        ds.write_chunk((1, 0, 2), ndist.encode_overlap_chunk(pairs, counts), True)
    want = table_dict(pairs, counts)
    got, max_node = ndist.deserializeOverlapChunk(path, 'tmp/label_overlaps_', (1, 0, 2))
    assert got == want and max_node == (1 << 63) + 1
    assert all(isinstance(k, int) for k in got)
    got2, _ = ndist.deserializeOverlapChunk(os.path.join(path, 'tmp', 'label_overlaps_'), (1, 0, 2))
    assert got2 == want
    assert ndist.deserializeOverlapChunk(path, 'tmp/label_overlaps_', [0, 0, 0]) == ({}, 0)
    assert ndist.deserializeOverlapChunk(os.path.join(path, 'tmp', 'label_overlaps_'), (0, 1, 1)) == ({}, 0)


# --------------------------------------------------- checks before the device
def test_label_overlaps_argument_checks():
    a = np.zeros((2, 3, 4), np.uint64)
    with pytest.raises(ValueError, match='3-D'):
        rag.label_overlaps(a[0], a[0])
    with pytest.raises(ValueError, match='shape'):
        rag.label_overlaps(a, a[:, :, :3])
    with pytest.raises(TypeError, match='integer'):
        rag.label_overlaps(a, a.astype(np.float32))
    with pytest.raises(TypeError, match='integer'):
        rag.label_overlaps(a.astype(np.float64), a)
    with pytest.raises(ValueError, match='ignore_label'):
        rag.label_overlaps(a, a, ignore_label=-1)
    with pytest.raises(ValueError, match='ignore_label'):
        rag.label_overlaps(a, a, ignore_label=1 << 64)
    with pytest.raises(ValueError, match='3 entries'):
        rag.label_overlaps(a, a, begin=(0, 0))
    with pytest.raises(ValueError, match='3 entries'):
        rag.label_overlaps(a, a, end=(1, 1, 1, 1))


def test_merge_and_max_overlaps_argument_checks():
    with pytest.raises(ValueError, match='pairs for'):
        rag.merge_overlaps(np.zeros((3, 2), np.uint64), np.zeros(2, np.uint64))
    with pytest.raises(ValueError):
        rag.merge_overlaps(np.zeros(3, np.uint64), np.zeros(3, np.uint64))   # not (n, 2)
    tables = dict(pairs=np.zeros((1, 2), np.uint64), counts=np.ones(1, np.uint64))
    with pytest.raises(ValueError, match='label_begin'):
        rag.max_overlaps(tables, 5, 4)
    with pytest.raises(ValueError, match='label_begin'):
        rag.max_overlaps(tables, -1, 4)


# ------------------------------------------------- the chunk loop of the merge
def _overlap_rows(ids):
    """Two rows per node: (node, 10 + node) once and (node, 20 + node) twice."""
    pairs = np.array([[a, k + a] for a in ids for k in (10, 20)], np.uint64).reshape(-1, 2)
    return pairs, np.array([1, 2] * len(ids), np.uint64)


def _overlap_words(ids):
    return np.array([w for a in ids for w in (a, 2, 10 + a, 1, 20 + a, 2)], np.uint64)


@pytest.fixture
def overlap_chunks(tmp_path):
    path = str(tmp_path / 'ol.n5')
    K.block_dataset(path, 'blocks', 'uint64', _overlap_words)
    p, c = ndist.decode_overlap_chunk(_overlap_words(K.MIXED_IDS))
    np.testing.assert_array_equal(p, _overlap_rows(K.MIXED_IDS)[0])
    np.testing.assert_array_equal(c, _overlap_rows(K.MIXED_IDS)[1])
    return path


def _merged_inputs(calls):
    (args, kw), = calls
    assert not kw and len(args) == 2
    return args


@pytest.mark.parametrize('serialize_count', [False, True])
def test_merge_reads_the_rows_of_its_range_and_writes_the_maxima(overlap_chunks, monkeypatch, serialize_count):
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_overlaps_handle', handle)
    best, n_best = np.arange(40, 44, dtype=np.uint64), np.arange(50, 54, dtype=np.uint64)
    read = K.capture(monkeypatch, rag, 'max_overlaps', (best, n_best))
    shape = (K.N_OUT, 2) if serialize_count else (K.N_OUT,)
    K.output_dataset(overlap_chunks, 'out', shape, 'uint64')
    ndist.mergeAndSerializeOverlaps(overlap_chunks, 'blocks', overlap_chunks, 'out', True, K.BEGIN, K.END,
                                    numberOfThreads=2, serializeCount=serialize_count)
    pairs, counts = _merged_inputs(merged)
    want = _overlap_rows(K.IN_RANGE)
    assert pairs.dtype == counts.dtype == np.uint64
    np.testing.assert_array_equal(pairs, want[0])
    np.testing.assert_array_equal(counts, want[1])
    assert read == [((handle, K.BEGIN, K.END), {})] and handle.freed == 1
    out = np.zeros(shape, np.uint64)
    out[K.BEGIN:K.END] = np.stack([best, n_best], axis=1) if serialize_count else best
    np.testing.assert_array_equal(K.read_output(overlap_chunks, 'out'), out)


def test_merge_of_an_empty_range_gets_empty_tables(overlap_chunks, monkeypatch):
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_overlaps_handle', handle)
    K.capture(monkeypatch, rag, 'max_overlaps', (np.zeros(2, np.uint64), np.zeros(2, np.uint64)))
    K.output_dataset(overlap_chunks, 'out', (16,), 'uint64')
    ndist.mergeAndSerializeOverlaps(overlap_chunks, 'blocks', overlap_chunks, 'out', True, 12, 14)
    pairs, counts = _merged_inputs(merged)
    assert (pairs.shape, pairs.dtype, counts.shape, counts.dtype) == ((0, 2), np.uint64, (0,), np.uint64)
    assert handle.freed == 1


def test_merge_without_max_overlap_writes_the_merged_chunk(overlap_chunks, monkeypatch):
    pairs, counts = _overlap_rows([4, 5])
    handle = K.Handle(n_edges=4, edges=pairs, counts=counts)
    merged = K.capture(monkeypatch, rag, 'merge_overlaps_handle', handle)
    read = K.capture(monkeypatch, rag, 'max_overlaps', None)
    K.output_dataset(overlap_chunks, 'out', (K.N_OUT,), 'uint64', chunks=(4,))
    ndist.mergeAndSerializeOverlaps(overlap_chunks, 'blocks', overlap_chunks, 'out', False, K.BEGIN, K.END)
    np.testing.assert_array_equal(_merged_inputs(merged)[0], _overlap_rows(K.IN_RANGE)[0])
    assert read == [] and handle.freed == 1
    np.testing.assert_array_equal(K.chunk_of(overlap_chunks, 'out', (1,)), ndist.encode_overlap_chunk(pairs, counts))
    assert K.chunk_of(overlap_chunks, 'out', (0,)) is None and K.chunk_of(overlap_chunks, 'out', (2,)) is None
    # an empty merged table writes no chunk
    empty = K.Handle(n_edges=0)
    monkeypatch.setattr(rag, 'merge_overlaps_handle', lambda *a: empty)
    ndist.mergeAndSerializeOverlaps(overlap_chunks, 'blocks', overlap_chunks, 'out', False, 8, 12)
    assert K.chunk_of(overlap_chunks, 'out', (2,)) is None and empty.freed == 1


def test_block_overlaps_write_their_chunk_unless_empty(tmp_path, monkeypatch):
    path = str(tmp_path / 'b.n5')
    K.output_dataset(path, 'blocks', (1, 1, 3), 'uint64', chunks=(1, 1, 1))
    pairs, counts = _overlap_rows([4, 5])
    lab = np.zeros((1, 1, 2), np.uint64)
    for handle, ignore, want in ((K.Handle(n_edges=4, edges=pairs, counts=counts), (True, 7), 7),
                                 (K.Handle(n_edges=0), (False, 7), None)):
        made = K.capture(monkeypatch, rag, 'label_overlaps_handle', handle)
        pos = (0, 0, 1) if handle.n_edges else (0, 0, 2)
        ndist.computeAndSerializeLabelOverlaps(lab, lab, path, 'blocks', pos, *ignore)
        (args, kw), = made
        assert args[0] is lab and args[1] is lab and list(args[2:]) + list(kw.values()) == [want]
        assert handle.freed == 1
    np.testing.assert_array_equal(K.chunk_of(path, 'blocks', (0, 0, 1)), ndist.encode_overlap_chunk(pairs, counts))
    assert K.chunk_of(path, 'blocks', (0, 0, 2)) is None
