"""The argument checks of the label-table calls (rag.py: the three volume calls,
the three merges, the three dense-row readers and the two assignment uploads):
one table of single-fault bad arguments on 1 x 2 x 3 numpy volumes and 2-row
tables, the exception type and the whole message of each.  Every case raises
before the library is loaded (no GPU, no library): loading it fails the test.
Which of two simultaneous faults wins is not pinned here."""
import numpy as np
import pytest

from cluster_tools_amd import rag

LAB = np.zeros((1, 2, 3), np.uint64)
DAT = np.zeros((1, 2, 3), np.float32)
MORPH = np.zeros((2, 11))
REGION = np.zeros((2, 5))
PAIRS = np.zeros((2, 2), np.uint64)
COUNTS = np.ones(2, np.uint64)
RANGE = 'need 0 <= label_begin <= label_end, got [%d, %d)'
IGNORE = 'ignore_label must be a uint64 value or None, got %d'
BOX2 = 'begin / end must have 3 entries'
BOX3 = 'begin / end / origin must have 3 entries'
MORPH_MSG = 'morphology rows have 11 columns, got %s'
REGION_MSG = 'region-feature rows have 5 columns, got %s'


def _overlaps(labels=LAB, values=LAB, **kw):
    return rag.label_overlaps_handle(labels, values, **kw)


def _morphology(labels=LAB, **kw):
    return rag.morphology_handle(labels, **kw)


def _region(labels=LAB, data=DAT, **kw):
    return rag.region_features_handle(labels, data, **kw)


def _max_overlaps(lb=0, le=4, pairs=PAIRS, counts=COUNTS):
    return rag.max_overlaps(dict(pairs=pairs, counts=counts), lb, le)


def _morphology_rows(lb=0, le=4, rows=MORPH):
    return rag.morphology_rows(dict(rows=rows), lb, le)


def _region_rows(lb=0, le=4, rows=REGION, **kw):
    return rag.region_feature_rows(dict(rows=rows), lb, le, **kw)


def _odd_pairs_message():
    with pytest.raises(ValueError) as e:
        np.zeros(3, np.uint64).reshape(-1, 2)
    return str(e.value)


# name -> (the call, its keywords, the exception, the whole message)
CASES = {
    'overlaps_not_3d': (_overlaps, dict(labels=LAB[0], values=LAB[0]), ValueError,
                        'labels must be 3-D, got shape (2, 3)'),
    'overlaps_unequal_shapes': (_overlaps, dict(values=LAB[:, :, :2]), ValueError,
                                'values shape (1, 2, 2) != labels shape (1, 2, 3)'),
    'overlaps_float_labels': (_overlaps, dict(labels=DAT), TypeError, 'labels must hold integer labels, got float32'),
    'overlaps_float_values': (_overlaps, dict(values=LAB.astype(np.float64)), TypeError,
                              'values must hold integer labels, got float64'),
    'overlaps_begin_short': (_overlaps, dict(begin=(0, 0)), ValueError, BOX2),
    'overlaps_begin_long': (_overlaps, dict(begin=(0, 0, 0, 0)), ValueError, BOX2),
    'overlaps_end_short': (_overlaps, dict(end=(1, 2)), ValueError, BOX2),
    'overlaps_end_long': (_overlaps, dict(end=(1, 2, 3, 1)), ValueError, BOX2),
    'overlaps_ignore_negative': (_overlaps, dict(ignore_label=-1), ValueError, IGNORE % -1),
    'overlaps_ignore_2_64': (_overlaps, dict(ignore_label=1 << 64), ValueError, IGNORE % (1 << 64)),
    'morphology_not_3d': (_morphology, dict(labels=LAB[0]), ValueError, 'labels must be 3-D, got shape (2, 3)'),
    'morphology_float_labels': (_morphology, dict(labels=DAT), TypeError,
                                'labels must hold integer labels, got float32'),
    'morphology_begin_short': (_morphology, dict(begin=(0, 0)), ValueError, BOX3),
    'morphology_begin_long': (_morphology, dict(begin=(0, 0, 0, 0)), ValueError, BOX3),
    'morphology_end_short': (_morphology, dict(end=(1, 2)), ValueError, BOX3),
    'morphology_end_long': (_morphology, dict(end=(1, 2, 3, 1)), ValueError, BOX3),
    'morphology_origin_short': (_morphology, dict(origin=(5,)), ValueError, BOX3),
    'morphology_origin_long': (_morphology, dict(origin=(1, 1, 1, 1)), ValueError, BOX3),
    'region_not_3d': (_region, dict(labels=LAB[0], data=DAT[0]), ValueError, 'labels must be 3-D, got shape (2, 3)'),
    'region_unequal_shapes': (_region, dict(data=DAT[:, :, :2]), ValueError,
                              'data shape (1, 2, 2) != labels shape (1, 2, 3)'),
    'region_float_labels': (_region, dict(labels=DAT), TypeError, 'labels must hold integer labels, got float32'),
    'region_float64_data': (_region, dict(data=DAT.astype(np.float64)), TypeError,
                            'data must be float32 or uint8, got float64'),
    'region_integer_data': (_region, dict(data=LAB), TypeError, 'data must be float32 or uint8, got uint64'),
    'region_begin_short': (_region, dict(begin=(0, 0)), ValueError, BOX2),
    'region_begin_long': (_region, dict(begin=(0, 0, 0, 0)), ValueError, BOX2),
    'region_end_short': (_region, dict(end=(1, 2)), ValueError, BOX2),
    'region_end_long': (_region, dict(end=(1, 2, 3, 1)), ValueError, BOX2),
    'region_ignore_negative': (_region, dict(ignore_label=-1), ValueError, IGNORE % -1),
    'region_ignore_2_64': (_region, dict(ignore_label=1 << 64), ValueError, IGNORE % (1 << 64)),
    'merge_overlaps_unequal': (rag.merge_overlaps_handle, dict(pairs=PAIRS, counts=np.ones(3, np.uint64)),
                               ValueError, '2 pairs for 3 counts'),
    'merge_overlaps_odd_size': (rag.merge_overlaps_handle, dict(pairs=np.zeros(3, np.uint64), counts=COUNTS),
                                ValueError, _odd_pairs_message()),
    'merge_morphology_flat_size': (rag.merge_morphology_handle, dict(rows=np.zeros(12)), ValueError,
                                   MORPH_MSG % '(12,)'),
    'merge_morphology_narrow': (rag.merge_morphology_handle, dict(rows=np.zeros((2, 10))), ValueError,
                                MORPH_MSG % '(2, 10)'),
    'merge_morphology_transposed': (rag.merge_morphology_handle, dict(rows=np.zeros((11, 2))), ValueError,
                                    MORPH_MSG % '(11, 2)'),
    'merge_region_flat_size': (rag.merge_region_features_handle, dict(rows=np.zeros(12)), ValueError,
                               REGION_MSG % '(12,)'),
    'merge_region_narrow': (rag.merge_region_features_handle, dict(rows=np.zeros((2, 4))), ValueError,
                            REGION_MSG % '(2, 4)'),
    'merge_region_transposed': (rag.merge_region_features_handle, dict(rows=np.zeros((5, 2))), ValueError,
                                REGION_MSG % '(5, 2)'),
    'max_overlaps_negative_begin': (_max_overlaps, dict(lb=-1), ValueError, RANGE % (-1, 4)),
    'max_overlaps_end_before_begin': (_max_overlaps, dict(lb=5), ValueError, RANGE % (5, 4)),
    'max_overlaps_unequal_tables': (_max_overlaps, dict(counts=np.ones(3, np.uint64)), ValueError,
                                    '2 pairs for 3 counts'),
    'morphology_rows_negative_begin': (_morphology_rows, dict(lb=-1), ValueError, RANGE % (-1, 4)),
    'morphology_rows_end_before_begin': (_morphology_rows, dict(lb=5), ValueError, RANGE % (5, 4)),
    'morphology_rows_narrow_table': (_morphology_rows, dict(rows=np.zeros((2, 10))), ValueError,
                                     MORPH_MSG % '(2, 10)'),
    'region_rows_negative_begin': (_region_rows, dict(lb=-1), ValueError, RANGE % (-1, 4)),
    'region_rows_end_before_begin': (_region_rows, dict(lb=5), ValueError, RANGE % (5, 4)),
    'region_rows_narrow_table': (_region_rows, dict(rows=np.zeros((2, 4))), ValueError, REGION_MSG % '(2, 4)'),
    'region_rows_bad_form': (_region_rows, dict(form='mean'), ValueError,
                             "form must be 'sums' or 'features', got 'mean'"),
    'region_rows_norm_zero': (_region_rows, dict(norm=0.0), ValueError, 'norm must be finite and positive, got 0.0'),
    'region_rows_norm_inf': (_region_rows, dict(norm=float('inf')), ValueError,
                             'norm must be finite and positive, got inf'),
    'region_rows_norm_nan': (_region_rows, dict(norm=float('nan')), ValueError,
                             'norm must be finite and positive, got nan'),
    'dense_not_1d': (rag.assignment_dense, dict(table=PAIRS), ValueError, 'table must be 1-D, got shape (2, 2)'),
    'dense_float_table': (rag.assignment_dense, dict(table=np.zeros(2)), TypeError,
                          'table must hold integers, got float64'),
    'dense_negative': (rag.assignment_dense, dict(table=np.array([0, -1])), ValueError, 'table holds negative values'),
    'sparse_unequal': (rag.assignment_sparse, dict(keys=COUNTS, values=np.ones(3, np.uint64)), ValueError,
                       '2 keys for 3 values'),
    'sparse_float_values': (rag.assignment_sparse, dict(keys=COUNTS, values=np.ones(2)), TypeError,
                            'values must hold integers, got float64'),
    'sparse_keys_not_1d': (rag.assignment_sparse, dict(keys=PAIRS, values=COUNTS), ValueError,
                           'keys must be 1-D, got shape (2, 2)'),
}


def _tensor_cases():
    """numpy mixed with a tensor, and a tensor that is not on the device."""
    import torch
    lab, dat = torch.zeros((1, 2, 3), dtype=torch.int64), torch.zeros((1, 2, 3))
    rows, vec = torch.zeros((2, 11), dtype=torch.float64), torch.zeros(2, dtype=torch.int64)
    kinds = '%s must both be numpy arrays or both CUDA tensors'
    return {
        'overlaps_tensor_values': (_overlaps, dict(values=lab), ValueError, kinds % 'labels and values'),
        'overlaps_tensor_labels': (_overlaps, dict(labels=lab), ValueError, kinds % 'labels and values'),
        'region_tensor_data': (_region, dict(data=dat), ValueError, kinds % 'labels and data'),
        'merge_overlaps_tensor_counts': (rag.merge_overlaps_handle, dict(pairs=PAIRS, counts=vec), ValueError,
                                         kinds % 'pairs and counts'),
        'morphology_host_tensor': (_morphology, dict(labels=lab), ValueError,
                                   'labels must be a contiguous CUDA tensor of 32- or 64-bit integers'),
        'merge_morphology_host_tensor': (rag.merge_morphology_handle, dict(rows=rows), ValueError,
                                         'rows must be a contiguous float64 CUDA tensor'),
        'merge_region_host_tensor': (rag.merge_region_features_handle, dict(rows=rows), ValueError,
                                     'rows must be a contiguous float64 CUDA tensor'),
        'dense_host_tensor': (rag.assignment_dense, dict(table=vec), ValueError,
                              'table must be a contiguous 1-D CUDA tensor of 64-bit integers'),
    }


TENSOR_CASES = ('overlaps_tensor_values', 'overlaps_tensor_labels', 'region_tensor_data',
                'merge_overlaps_tensor_counts', 'morphology_host_tensor', 'merge_morphology_host_tensor',
                'merge_region_host_tensor', 'dense_host_tensor')


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def loaded(*a, **kw):
        raise AssertionError('the library was loaded before the argument check')
    monkeypatch.setattr(rag.L, 'load', loaded)
    monkeypatch.setattr(rag.L, 'init_device', loaded)


def _raises(fn, kw, exc, msg):
    with pytest.raises(exc) as e:
        fn(**kw)
    assert type(e.value) is exc and str(e.value) == msg


@pytest.mark.parametrize('case', sorted(CASES))
def test_bad_argument(case):
    _raises(*CASES[case])


@pytest.mark.parametrize('case', TENSOR_CASES)
def test_bad_tensor_argument(case):
    pytest.importorskip('torch')
    _raises(*_tensor_cases()[case])


def test_the_tensor_table_is_whole():
    pytest.importorskip('torch')
    assert sorted(_tensor_cases()) == sorted(TENSOR_CASES)
