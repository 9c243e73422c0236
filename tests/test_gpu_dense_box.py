"""The box descriptor the dense-volume kernels share (csrc/ctg_plan.h: VolBox,
vol_box): for the thresholded components, the distance transform and the
seeded watershed, a box off the origin on every axis inside an array with odd
strides gives exactly what the same call gives on the contiguous copy of the
box.  The voxels around the box hold values that would change the result if a
kernel read them: foreground, seeds, NaN heights."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from cluster_tools_amd import rag

pytestmark = pytest.mark.gpu

SHAPE, B, E = (5, 9, 13), (1, 2, 3), (4, 9, 12)
BOX = tuple(slice(lo, hi) for lo, hi in zip(B, E))


def _embed(inner, outside):
    """inner in the box of an array of SHAPE that holds `outside` everywhere else"""
    a = np.full(SHAPE, outside, dtype=inner.dtype)
    a[BOX] = inner
    return a


@pytest.fixture(scope='module')
def noise():
    x = np.random.RandomState(5913).rand(*[hi - lo for lo, hi in zip(B, E)]).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('on_dev', [False, True])
def test_components(gpu, noise, on_dev):
    # outside: foreground that would join the components of the box's faces; normalised, it would move the range too
    for normalize, outside in ((False, 1.0), (True, 7.0)):
        big, small = _embed(noise, outside), noise.copy()
        if on_dev:
            import torch
            big, small = torch.from_numpy(big).cuda(), torch.from_numpy(small).cuda()
        want, n = rag.threshold_components(small, 0.7, normalize=normalize, connectivity=1)
        got, m = rag.threshold_components(big, 0.7, normalize=normalize, connectivity=1, begin=B, end=E)
        if on_dev:
            want, got = want.cpu().numpy(), got.cpu().numpy()
        assert n > 1 and m == n
        assert_array_equal(got, want)


def test_distance_transform(gpu, noise):
    # outside: seeds next to every face of the box, which would shorten the distances
    src = (noise > 0.97).astype(np.uint8)
    assert 0 < src.sum() < 8
    want, wi = rag.distance_transform(src, pitch=(2.0, 1.0, 1.5))
    got, gi = rag.distance_transform(_embed(src, 1), pitch=(2.0, 1.0, 1.5), begin=B, end=E)
    assert_array_equal(got, want)
    assert gi == wi
    lab = np.where(noise > 0.97, 5, 0).astype(np.uint64)
    want, wi = rag.distance_transform(lab, label=5, squared=True)
    got, gi = rag.distance_transform(_embed(lab, 5), label=5, squared=True, begin=B, end=E)
    assert_array_equal(got, want)
    assert gi == wi


def test_seeded_watershed(gpu, noise):
    # outside: NaN heights (a NaN read from the array would raise) and seeds of a label the box does not hold
    import torch
    seeds = np.where(noise > 0.9, np.arange(1, noise.size + 1).reshape(noise.shape), 0).astype(np.uint64)
    assert 3 < np.count_nonzero(seeds) < noise.size // 4
    want, wi = rag.seeded_watershed(np.ascontiguousarray(noise), seeds)
    assert wi.n_zero == 0
    # (tensors: the numpy front end looks for NaN in the box itself, and there is none)
    h, s = torch.from_numpy(_embed(noise, np.nan)).cuda(), torch.from_numpy(_embed(seeds, 999).view(np.int64)).cuda()
    got, gi = rag.seeded_watershed(h, s, begin=B, end=E)
    assert_array_equal(got.cpu().numpy().view(np.uint64), want)
    assert (gi.max_id, gi.n_zero, gi.n_dropped) == (wi.max_id, wi.n_zero, wi.n_dropped)
    got, gi = rag.seeded_watershed(_embed(noise, np.nan), _embed(seeds, 999), begin=B, end=E)
    assert_array_equal(got, want)
    # the size filter's second flood reads the box-shaped result as its seeds: the strides change within the call
    want, wi = rag.seeded_watershed(np.ascontiguousarray(noise), seeds, size_filter=6)
    assert wi.n_dropped > 0
    got, gi = rag.seeded_watershed(_embed(noise, np.nan), _embed(seeds, 999), size_filter=6, begin=B, end=E)
    assert_array_equal(got, want)
    assert (gi.max_id, gi.n_zero, gi.n_dropped) == (wi.max_id, wi.n_zero, wi.n_dropped)
