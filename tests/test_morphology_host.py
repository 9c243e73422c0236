"""Segment morphology without a GPU: the numpy oracle the GPU tests compare
with (pinned by a hand-computed case), the morphology-chunk format of the ndist
mirror, the exactness premise of the merge, and the argument checks the Python
layer makes before it touches the device."""
import json
import os

import numpy as np
import pytest

from cluster_tools_amd import n5, ndist, rag
from tests import chunk_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


# ------------------------------------------------------------------- oracle
def morph_table(labels, origin=(0, 0, 0)):
    """(nodes (N,), moments (N,10) uint64) of a (Z,Y,X) label array whose first
    voxel sits at ``origin``: per distinct label [n, sum z, sum y, sum x,
    min z, min y, min x, max z, max y, max x] over integer coordinates (max
    inclusive).  Label 0 is a label like any other."""
    labels = np.asarray(labels).astype(np.uint64)
    if labels.size == 0:
        return np.zeros(0, np.uint64), np.zeros((0, 10), np.uint64)
    nodes, inv = np.unique(labels.ravel(), return_inverse=True)
    inv = inv.ravel()
    mom = np.zeros((nodes.shape[0], 10), np.uint64)
    mom[:, 0] = np.bincount(inv, minlength=nodes.shape[0]).astype(np.uint64)
    mom[:, 4:7] = np.iinfo(np.uint64).max
    grids = np.meshgrid(*[np.arange(s, dtype=np.uint64) + np.uint64(o) for s, o in zip(labels.shape, origin)],
                        indexing='ij')
    for c, g in enumerate(grids):
        g = g.ravel()
        np.add.at(mom[:, 1 + c], inv, g)
        np.minimum.at(mom[:, 4 + c], inv, g)
        np.maximum.at(mom[:, 7 + c], inv, g)
    return nodes, mom


def morph_rows(nodes, mom):
    """(N,11) float64 rows [id, size, com z y x, min z y x, max z y x]: the one
    division, of the same integers the library divides."""
    rows = np.zeros((nodes.shape[0], 11), np.float64)
    rows[:, 0] = nodes.astype(np.float64)
    rows[:, 1] = mom[:, 0].astype(np.float64)
    rows[:, 2:5] = mom[:, 1:4].astype(np.float64) / mom[:, :1].astype(np.float64)
    rows[:, 5:] = mom[:, 4:].astype(np.float64)
    return rows


def dense_rows(rows, label_begin, label_end):
    """Rows scattered by id over [label_begin, label_end), zeros elsewhere."""
    out = np.zeros((label_end - label_begin, 11), np.float64)
    ids = rows[:, 0].astype(np.int64)
    sel = (ids >= label_begin) & (ids < label_end)
    out[ids[sel] - label_begin] = rows[sel]
    return out


@pytest.fixture(scope='module')
def kat():
    with open(os.path.join(GOLD, 'morphology_kat.json')) as fh:
        return json.load(fh)


def test_oracle_matches_hand_computed_case(kat):
    labels = np.array(kat['labels'], np.uint64)
    assert labels.shape == (2, 3, 4)
    nodes, mom = morph_table(labels)
    np.testing.assert_array_equal(nodes, np.array(kat['nodes'], np.uint64))
    np.testing.assert_array_equal(mom, np.array(kat['moments'], np.uint64))
    assert int(mom[:, 0].sum()) == labels.size and nodes[0] == 0          # label 0 has a row
    assert (mom[1, 0] == 1) and (mom[1, 4:7] == mom[1, 7:]).all()         # the single voxel
    rows = morph_rows(nodes, mom)
    np.testing.assert_array_equal(rows, np.array(kat['rows'], np.float64))
    assert rows[2, 2] == 1.0 / 3.0 and rows[2, 3] == 5.0 / 3.0            # a third: rounded once
    nodes_o, mom_o = morph_table(labels, kat['origin'])
    np.testing.assert_array_equal(nodes_o, nodes)
    np.testing.assert_array_equal(mom_o, np.array(kat['moments_at_origin'], np.uint64))
    np.testing.assert_array_equal(dense_rows(rows, *kat['label_range']), np.array(kat['dense_rows'], np.float64))


def test_oracle_origin_shifts_sums_and_boxes():
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 9, size=(4, 5, 6)).astype(np.uint64)
    origin = np.array([7, 11, 13], np.uint64)
    nodes, mom = morph_table(labels)
    nodes_o, mom_o = morph_table(labels, origin)
    np.testing.assert_array_equal(nodes_o, nodes)
    np.testing.assert_array_equal(mom_o[:, 1:4], mom[:, 1:4] + mom[:, :1] * origin)
    np.testing.assert_array_equal(mom_o[:, 4:7], mom[:, 4:7] + origin)
    np.testing.assert_array_equal(mom_o[:, 7:], mom[:, 7:] + origin)
    assert morph_table(np.zeros((0, 3, 3), np.uint64))[1].shape == (0, 10)


# ------------------------------------------------------------- chunk format
def test_chunk_words_of_hand_computed_case(kat):
    rows = np.array(kat['rows'], np.float64)
    words = ndist.encode_morphology_chunk(rows)
    assert words.dtype == np.float64 and words.ndim == 1
    np.testing.assert_array_equal(words, np.array(kat['chunk'], np.float64))
    np.testing.assert_array_equal(ndist.decode_morphology_chunk(words), rows)
    assert ndist.encode_morphology_chunk(np.zeros((0, 11))).size == 0
    assert ndist.decode_morphology_chunk(np.zeros(0)).shape == (0, 11)
    with pytest.raises(RuntimeError, match='truncated'):
        ndist.decode_morphology_chunk(words[:-1])
    with pytest.raises(ValueError, match='columns'):
        ndist.encode_morphology_chunk(np.zeros((3, 10)))


def test_chunk_round_trip_through_n5(tmp_path, kat):
    rows = np.array(kat['rows'], np.float64)
    path = str(tmp_path / 'm.n5')
    with n5.file_reader(path) as f:
        ds = f.require_dataset('tmp/morphology_', shape=(24, 40, 72), chunks=(10, 16, 32), dtype='float64',
                               compression='gzip')
        ds.write_chunk((2, 1, 0), ndist.encode_morphology_chunk(rows), True)
    with n5.file_reader(path, 'r') as f:
        ds = f['tmp/morphology_']
        got = ds.read_chunks([(2, 1, 0), (0, 0, 0)])
    np.testing.assert_array_equal(ndist.decode_morphology_chunk(got[0]), rows)
    assert got[1] is None


# --------------------------------------------------- the merge's premise
def test_merge_recovers_integer_sums_below_2_51():
    """ctg_merge_morphology recovers a row's integer coordinate sum S from its
    centre of mass fl(S / n) as rint(fl(S / n) * n).  Two roundings of relative
    error 2^-53 each leave |fl(S / n) * n - S| <= S * 2^-52 < 1/2 for S < 2^51:
    checked on 10^5 seeded (S, n), the extremes always among them."""
    rng = np.random.default_rng(20)
    s = rng.integers(0, 1 << 51, size=100000, dtype=np.uint64)
    n = rng.integers(1, (1 << 32) + 1, size=100000, dtype=np.uint64)
    s[:6] = (1 << 51) - 1
    n[:3] = [1, 3, 1 << 32]
    s[3:6] = [0, 1, (1 << 51) - 2]
    n[3:6] = [1 << 32, 3, 3]
    n[6:9] = [1, 3, 1 << 32]
    assert s.max() == (1 << 51) - 1 and n.min() == 1 and n.max() == 1 << 32
    sf, nf = s.astype(np.float64), n.astype(np.float64)
    assert (sf.astype(np.uint64) == s).all()
    np.testing.assert_array_equal(np.rint((sf / nf) * nf), sf)


# --------------------------------------------------- checks before the device
def test_morphology_argument_checks():
    a = np.zeros((2, 3, 4), np.uint64)
    with pytest.raises(ValueError, match='3-D'):
        rag.morphology(a[0])
    with pytest.raises(TypeError, match='integer'):
        rag.morphology(a.astype(np.float32))
    with pytest.raises(ValueError, match='3 entries'):
        rag.morphology(a, begin=(0, 0))
    with pytest.raises(ValueError, match='3 entries'):
        rag.morphology(a, origin=(1, 1, 1, 1))
    with pytest.raises(ValueError, match='columns'):
        rag.merge_morphology(np.zeros((3, 10)))
    with pytest.raises(ValueError, match='columns'):
        rag.merge_morphology(np.zeros(12))
    with pytest.raises(ValueError, match='label_begin'):
        rag.morphology_rows(dict(rows=np.zeros((0, 11))), 5, 4)
    with pytest.raises(ValueError, match='label_begin'):
        rag.morphology_rows(dict(rows=np.zeros((0, 11))), -1, 4)


# ------------------------------------------------- the chunk loop of the merge
def _rows_of(ids):
    """One row per id, told apart by its size column."""
    rows = np.zeros((len(ids), 11), np.float64)
    rows[:, 0] = ids
    rows[:, 1] = 100 + np.arange(len(ids))
    return rows


@pytest.fixture
def morph_chunks(tmp_path):
    path = str(tmp_path / 'm.n5')
    K.block_dataset(path, 'blocks', 'float64', lambda ids: ndist.encode_morphology_chunk(_rows_of(ids)))
    K.output_dataset(path, 'out', (K.N_OUT, 11), 'float64')
    return path


def test_merge_reads_the_rows_of_its_range_and_writes_the_slice(morph_chunks, monkeypatch):
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_morphology_handle', handle)
    dense = np.arange(4 * 11, dtype=np.float64).reshape(4, 11) + 0.5
    read = K.capture(monkeypatch, rag, 'morphology_rows', dense)
    ndist.mergeAndSerializeMorphology(morph_chunks, 'blocks', morph_chunks, 'out', K.BEGIN, K.END, numberOfThreads=2)
    ((rows,), kw), = merged
    mixed = _rows_of(K.MIXED_IDS)
    assert not kw and rows.dtype == np.float64
    np.testing.assert_array_equal(rows, mixed[[K.MIXED_IDS.index(a) for a in K.IN_RANGE]])
    assert read == [((handle, K.BEGIN, K.END), {})] and handle.freed == 1
    out = np.zeros((K.N_OUT, 11))
    out[K.BEGIN:K.END] = dense
    np.testing.assert_array_equal(K.read_output(morph_chunks, 'out'), out)


def test_merge_of_an_empty_range_gets_an_empty_table(morph_chunks, monkeypatch):
    handle = K.Handle()
    merged = K.capture(monkeypatch, rag, 'merge_morphology_handle', handle)
    K.capture(monkeypatch, rag, 'morphology_rows', np.zeros((0, 11)))
    ndist.mergeAndSerializeMorphology(morph_chunks, 'blocks', morph_chunks, 'out', 12, 12)
    ((rows,), _), = merged
    assert rows.shape == (0, 11) and rows.dtype == np.float64 and handle.freed == 1


def test_block_morphology_writes_its_chunk_unless_empty(tmp_path, monkeypatch):
    path = str(tmp_path / 'b.n5')
    K.output_dataset(path, 'blocks', (1, 1, 3), 'float64', chunks=(1, 1, 1))
    rows = _rows_of([4, 5])
    lab = np.zeros((1, 1, 2), np.uint64)
    for handle, pos in ((K.Handle(n_nodes=2, morph_rows=rows), (0, 0, 1)), (K.Handle(n_nodes=0), (0, 0, 2))):
        made = K.capture(monkeypatch, rag, 'morphology_handle', handle)
        ndist.computeAndSerializeMorphology(lab, np.array([3, 4, 5]), path, 'blocks', pos)
        (args, kw), = made
        assert args[0] is lab and list(args[1:]) + list(kw.values()) == [[3, 4, 5]] and handle.freed == 1
    np.testing.assert_array_equal(K.chunk_of(path, 'blocks', (0, 0, 1)), rows.reshape(-1))
    assert K.chunk_of(path, 'blocks', (0, 0, 2)) is None
