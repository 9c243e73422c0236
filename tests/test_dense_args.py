"""The begin / end / out checks that threshold_components, distance_transform
and seeded_watershed share (rag.py: _box, _dense_out): one table of bad
arguments through all three on 2 x 3 x 4 numpy inputs, the exception type and
the whole message of each.  Every case raises before the library is loaded
(no GPU, no library): loading it fails the test."""
import numpy as np
import pytest

from cluster_tools_amd import rag

SHAPE = (2, 3, 4)
INT_OUT = 'out must be a contiguous 64-bit integer array of the shape of the box (2, 3, 4)'


def _cc(**kw):
    return rag.threshold_components(np.zeros(SHAPE, np.float32), 0.5, **kw)


def _edt(**kw):
    return rag.distance_transform(np.zeros(SHAPE, np.uint8), **kw)


def _edt_squared(**kw):
    return rag.distance_transform(np.zeros(SHAPE, np.uint8), squared=True, **kw)


def _ws(**kw):
    return rag.seeded_watershed(np.zeros(SHAPE, np.float32), np.zeros(SHAPE, np.uint64), **kw)


# name -> (the call, what its messages call the input, a good out dtype, a wrong one, the message of a bad out)
CALLS = {
    'components': (_cc, 'data', np.uint64, np.float32, INT_OUT),
    'distance': (_edt, 'src', np.float32, np.float64,
                 'out must be a contiguous float32 array of the shape of the box (2, 3, 4)'),
    'distance_squared': (_edt_squared, 'src', np.float64, np.float32,
                         'out must be a contiguous float64 array of the shape of the box (2, 3, 4)'),
    'watershed': (_ws, 'hmap', np.uint64, np.uint32, INT_OUT),
}


def _outside(b, e):
    return 'box [%s, %s) outside the array of shape (2, 3, 4)' % (list(b), list(e))


# name -> (keywords, message); the box cases are the same for every call
BOX_CASES = {
    'begin_too_short': (dict(begin=(0, 0)), 'begin / end must have 3 entries'),
    'end_too_long': (dict(end=(2, 3, 4, 1)), 'begin / end must have 3 entries'),
    'length_before_range': (dict(begin=(-1, 0), end=(9, 9, 9)), 'begin / end must have 3 entries'),
    'negative_begin': (dict(begin=(-1, 0, 0)), _outside((-1, 0, 0), (2, 3, 4))),
    'negative_end': (dict(end=(2, -1, 4)), _outside((0, 0, 0), (2, -1, 4))),
    'begin_past_end': (dict(begin=(1, 2, 3), end=(1, 1, 4)), _outside((1, 2, 3), (1, 1, 4))),
    'end_past_shape': (dict(end=(2, 3, 5)), _outside((0, 0, 0), (2, 3, 5))),
    'begin_past_shape': (dict(begin=(3, 0, 0)), _outside((3, 0, 0), (2, 3, 4))),
}


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def loaded(*a, **kw):
        raise AssertionError('the library was loaded before the argument check')
    monkeypatch.setattr(rag.L, 'load', loaded)
    monkeypatch.setattr(rag.L, 'init_device', loaded)


@pytest.mark.parametrize('call', sorted(CALLS))
@pytest.mark.parametrize('case', sorted(BOX_CASES))
def test_bad_box(call, case):
    kw, msg = BOX_CASES[case]
    with pytest.raises(ValueError) as e:
        CALLS[call][0](**kw)
    assert str(e.value) == msg


@pytest.mark.parametrize('call', sorted(CALLS))
def test_box_is_checked_before_out(call):
    fn, _, good, _, _ = CALLS[call]
    with pytest.raises(ValueError) as e:
        fn(end=(2, 3, 5), out=np.zeros((9,), good))
    assert str(e.value) == _outside((0, 0, 0), (2, 3, 5))


def _bad_outs(good, wrong):
    return {
        'wrong_dtype': np.zeros(SHAPE, wrong),
        'wrong_shape': np.zeros((2, 3, 5), good),
        'box_shape_not_array_shape': np.zeros((1, 3, 4), good),
        'flat': np.zeros(24, good),
        'non_contiguous': np.zeros((2, 3, 8), good)[:, :, ::2],
        'a_list': [[[0] * 4] * 3] * 2,
    }


@pytest.mark.parametrize('call', sorted(CALLS))
@pytest.mark.parametrize('case', sorted(_bad_outs(np.uint64, np.float32)))
def test_bad_out(call, case):
    fn, _, good, wrong, msg = CALLS[call]
    out = _bad_outs(good, wrong)[case]
    with pytest.raises(ValueError) as e:
        fn(out=out)
    assert str(e.value) == msg


@pytest.mark.parametrize('call', sorted(CALLS))
def test_out_of_a_box_has_the_box_shape(call):
    """An out of the array's shape does not fit a smaller box, and the message names the box's shape."""
    fn, _, good, _, msg = CALLS[call]
    with pytest.raises(ValueError) as e:
        fn(begin=(0, 1, 1), end=(2, 3, 4), out=np.zeros(SHAPE, good))
    assert str(e.value) == msg.replace('(2, 3, 4)', '(2, 2, 3)')


@pytest.mark.parametrize('call', sorted(CALLS))
def test_tensor_out_for_numpy_input(call):
    torch = pytest.importorskip('torch')
    fn, name, _, _, _ = CALLS[call]
    with pytest.raises(ValueError) as e:
        fn(out=torch.zeros(SHAPE))
    assert str(e.value) == 'out must be of the same kind as %s (numpy array or CUDA tensor)' % name
