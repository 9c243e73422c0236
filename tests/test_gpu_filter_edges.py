"""The filter branch at its edges (GPU): ctg_filters.hip through
cluster_tools_amd.fastfilters and the C ABI.

* axes shorter than the kernel radius (the multi-fold mirror of reflect_idx,
  axes of length 1 and 2) against the numpy restatement;
* the border rule against a second implementation, scipy.ndimage's 'mirror';
* the 257-tap limit and one step past it;
* ctg_sym_eigenvalues on the matrices where a closed form goes wrong
  (diagonal, repeated eigenvalues, scales from 1e-30 to 1e18) against
  numpy.linalg.eigvalsh, to one float32 epsilon of the largest eigenvalue;
* ndist.accumulateInput on a channel slice of an eigenvalue response, the
  non-contiguous view its caller passes (block_edge_features.py:159-164).

Filter tolerances are those of tests/test_filters.py.
"""
import ctypes

import numpy as np
import pytest

from cluster_tools_amd import _lib
from cluster_tools_amd import fastfilters as F
from oracle import filter_oracle as FO
from oracle import rag_oracle as O

from test_filters import FILTERS

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)


def assert_filter_close(got, ref):
    assert got.shape == ref.shape and got.dtype == np.float32
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6 * scale)


def _volume(shape, seed=3):
    return np.random.default_rng(seed).random(shape).astype(np.float32)


# ---------------------------------------------------------------- short axes
@pytest.mark.parametrize('sigma', [1.0, 3.5])
@pytest.mark.parametrize('shape', [(1, 7, 5), (2, 3, 1), (3, 2, 40), (2, 2)])
@pytest.mark.parametrize('name', FILTERS)
def test_filters_on_axes_shorter_than_the_radius(gpu, name, shape, sigma):
    a = _volume(shape)
    got = getattr(F, name)(a, sigma)
    ref = getattr(FO, name)(a.astype(np.float64), sigma)
    assert_filter_close(got, ref)


# ---------------------------------------------------------------- scipy's mirror
def _conv_axis(a, axis, taps):
    """ctg_filter_conv_axis of the float32 array a along one axis."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    out = torch.empty_like(t)
    w = np.ascontiguousarray(taps, dtype=np.float32)
    shape = np.asarray(t.shape, dtype=np.int64)
    rc = _lib.load().ctg_filter_conv_axis(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                          shape.ctypes.data, t.dim(), axis, w.ctypes.data, int(w.size),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'ctg_filter_conv_axis')
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('sigma', [1.0, 3.5])
@pytest.mark.parametrize('shape', [(9, 33, 17), (3, 2, 40)])
def test_border_rule_matches_scipy_mirror(gpu, shape, sigma):
    from scipy import ndimage as ndi
    a = _volume(shape, seed=8)
    a64 = a.astype(np.float64)
    # order 0: scipy's own Gaussian has this rule (radius int(3 sigma + 0.5), unit-sum taps)
    assert_filter_close(F.gaussianSmoothing(a, sigma), ndi.gaussian_filter(a64, sigma, mode='mirror', truncate=3.0))
    for order in (1, 2):
        taps = F.gaussian_taps(sigma, order)
        for axis in range(len(shape)):
            assert_filter_close(_conv_axis(a, axis, taps), ndi.correlate1d(a64, taps, axis=axis, mode='mirror'))


# ---------------------------------------------------------------- tap limit
def test_tap_limit(gpu):
    a = _volume((3, 5, 40), seed=9)
    assert F.gaussian_taps(42.6, 0).size == 257 and F.gaussian_taps(42.6, 2).size == 259
    assert F.gaussian_taps(43.0, 0).size == 259
    assert_filter_close(F.gaussianSmoothing(a, 42.6), FO.gaussianSmoothing(a.astype(np.float64), 42.6))
    with pytest.raises(_lib.CtgError, match='odd tap count <= 257'):
        F.laplacianOfGaussian(a, 42.6)
    with pytest.raises(_lib.CtgError, match='odd tap count <= 257'):
        F.gaussianSmoothing(a, 43.0)


# ---------------------------------------------------------------- eigenvalues
N_MAT = 3001
SPECTRA = [(1, 1, 2), (2, 2, 1), (1, 1, 1 + 1e-6), (1e4, 1, 1e-4), (-3, -3, -3.0001)]


def _random_symmetric(rng, dim, n):
    m = rng.standard_normal((n, dim, dim))
    return (m + m.transpose(0, 2, 1)) / 2


def _matrices(family, dim):
    """(N_MAT, dim, dim) symmetric float64 matrices of one family (rounded to float32 by the caller)."""
    rng = np.random.default_rng(dim)
    if family == 'random':
        return _random_symmetric(rng, dim, N_MAT)
    if family == 'tiny':
        return _random_symmetric(rng, dim, N_MAT) * 1e-30
    if family == 'huge':
        return _random_symmetric(rng, dim, N_MAT) * 1e18
    if family == 'diagonal':   # in every order, with repeated and zero entries
        d = rng.standard_normal((N_MAT, dim)) * 10.0 ** rng.integers(-3, 4, size=(N_MAT, 1))
        d[::7, 1] = d[::7, 0]
        d[::11, dim - 1] = 0.0
        d[::13] = d[::13, :1]
        return d[:, :, None] * np.eye(dim)
    if family == 'near_multiple_of_identity':   # lambda I and one off-diagonal of 1e-20
        lam = rng.uniform(-2.0, 2.0, size=N_MAT)
        m = lam[:, None, None] * np.eye(dim)
        i, j = np.triu_indices(dim, 1)
        pick = rng.integers(0, i.size, size=N_MAT)
        m[np.arange(N_MAT), i[pick], j[pick]] = m[np.arange(N_MAT), j[pick], i[pick]] = 1e-20
        return m
    assert family == 'rotated_spectra'
    q = np.linalg.qr(rng.standard_normal((N_MAT, dim, dim)))[0]
    spectra = np.array(SPECTRA, dtype=np.float64)[:, [0, 2] if dim == 2 else [0, 1, 2]]
    d = spectra[np.arange(N_MAT) % len(SPECTRA)]
    return np.einsum('nij,nj,nkj->nik', q, d, q)


@pytest.mark.parametrize('dim', [3, 2])
@pytest.mark.parametrize('family', ['random', 'diagonal', 'near_multiple_of_identity', 'rotated_spectra', 'tiny',
                                    'huge'])
def test_sym_eigenvalues_hard_matrices(gpu, family, dim):
    import torch
    m64 = _matrices(family, dim)
    iu = np.triu_indices(dim)                                          # a00 a01 [a02] a11 [a12 a22]
    comps = np.ascontiguousarray(m64[:, iu[0], iu[1]].T.astype(np.float32))     # component planes
    m = np.zeros((N_MAT, dim, dim))
    m[:, iu[0], iu[1]] = comps.T
    m[:, iu[1], iu[0]] = comps.T                                       # the float32 matrices, in float64
    ref = np.linalg.eigvalsh(m)[:, ::-1]
    t = torch.from_numpy(comps).cuda()
    out = torch.full((N_MAT, dim), float('nan'), dtype=torch.float32, device='cuda')
    rc = _lib.load().ctg_sym_eigenvalues(ctypes.c_void_p(t.data_ptr()), dim, N_MAT, ctypes.c_void_p(out.data_ptr()),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, 'ctg_sym_eigenvalues')
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    assert np.all(got[:, :-1] >= got[:, 1:]), 'eigenvalues are not descending'
    bound = F32_EPS * np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    nz = bound[:, 0] > 0
    print('sym_eig %s dim %d: worst |got - ref| / bound = %.3f' % (family, dim, (err[nz] / bound[nz]).max()))
    assert np.all(err <= bound)


# ---------------------------------------------------------------- accumulateInput on a channel slice
def test_accumulate_input_on_channel_slices(gpu):
    from cluster_tools_amd import ndist, synthetic as S
    from test_gpu_parity import check_quantiles
    lab, bnd = S.generate((20, 32, 40), cell=6, seed=5)
    resp = F.hessianOfGaussianEigenvalues(bnd, 1.0)
    assert resp.shape == lab.shape + (3,)
    g = None
    for c in range(3):
        view = resp[..., c]
        assert not view.flags.c_contiguous
        lo, hi = float(view.min()), float(view.max())
        e_ref, f_ref = O.boundary_features(lab, np.ascontiguousarray(view), lo=lo, hi=hi)
        if g is None:
            g = ndist.Graph(e_ref)
        got = ndist.accumulateInput(g, view, lab, False, True, lo, hi)[g.findEdges(e_ref)]
        assert got.shape == f_ref.shape
        np.testing.assert_allclose(got[:, [0, 2, 8]], f_ref[:, [0, 2, 8]], rtol=1e-5, atol=1e-12)
        bound = (f_ref[:, 9] + 2) * np.finfo(np.float64).eps * np.maximum(f_ref[:, 2] ** 2, f_ref[:, 8] ** 2)
        assert np.all(np.abs(got[:, 1] - f_ref[:, 1]) <= np.maximum(1e-5 * np.abs(f_ref[:, 1]), bound))
        check_quantiles(got[:, 3:8], f_ref[:, 3:8], lo, hi)
        np.testing.assert_array_equal(got[:, 9], f_ref[:, 9])
