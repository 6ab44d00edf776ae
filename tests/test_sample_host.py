"""Sampling through a pivoted Cholesky on the host side (no GPU): the NumPy restatement ``utils.pivoted_cholesky`` against
LAPACK ``dpstrf`` and on the covariances that make it necessary, its exact cases, ``GP.sample_conditional(factor=...)`` over a
NumPy stand-in solver, and the four entry points in the header and the signature table.

Two bounds, derived and not tuned:

* reconstruction, ``max|A - L L^T| <= 2 tol`` with ``tol`` the stop threshold actually used: in exact arithmetic the residual
  is positive semidefinite with diagonal ``<= tol``, so every entry is ``<= tol``; forming ``L L^T`` in floating point adds at
  most ``m eps max diag = tol`` to first order;
* the affine law, ``|draws - (mean + z[:, :rank] fac[:, :rank]^T)| <= 8 M eps (|z[:, :rank]| |fac[:, :rank]|^T + |mean|)``
  entrywise: the dot-product rounding bound with a factor 8 for summation order and FMA."""
import ctypes
import os
import re

import numpy as np
import pytest

from george_amd import GP, kernels, utils
from george_amd import _native as N
from george_amd.utils import multivariate_gaussian_samples, pivoted_cholesky
from oracle import solver_np
from sample_ref import EPS, affine_law, check_factor, default_tol, low_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the three posterior covariances a plain Cholesky fails on (1-D ExpSquared, unit amplitude and scale)
def posterior_cases():
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0, 10, 468))
    yield "N468_M250", x, np.linspace(0, 10, 250), 0.1
    x = np.sort(rng.uniform(0, 10, 200))
    t = np.sort(np.concatenate([x[:150], rng.uniform(0, 10, 150)]))
    yield "N200_M300_yerr1e-3", x, t, 1e-3
    yield "N200_M300_yerr1e-6", x, t, 1e-6


def posterior_cov(x, t, yerr):
    kernel = kernels.ExpSquaredKernel(1.0)
    s = solver_np.DenseOracle(kernel)
    s.compute(x[:, None], yerr * np.ones(len(x)))
    _, cov = solver_np.gp_predict(s, kernel, x[:, None], np.sin(x), t[:, None], return_var=False, return_cov=True)
    return cov


@pytest.mark.parametrize("m,k", [(129, 37), (300, 64), (515, 129)])
def test_restatement_against_lapack_dpstrf(m, k):
    a = low_rank(m, k)
    tol = default_tol(a)
    L, piv, rank = pivoted_cholesky(a)
    assert rank == k
    check_factor(a, L, piv, rank, tol)
    L2, piv2, rank2 = pivoted_cholesky(a, tol=-1.0)                   # a negative threshold is the default too
    assert rank2 == rank and np.array_equal(L, L2) and np.array_equal(piv, piv2)
    try:
        from scipy.linalg.lapack import dpstrf
    except ImportError:
        pytest.skip("scipy.linalg.lapack.dpstrf is not available: the restatement's own checks passed")
    c, lpiv, lrank, info = dpstrf(a, lower=1, tol=tol)
    assert lrank == k
    Lp = np.tril(c)
    Lp[:, lrank:] = 0.0
    perm = lpiv - 1                                                    # P^T A P = Lp Lp^T
    back = np.empty_like(a)
    back[np.ix_(perm, perm)] = Lp @ Lp.T
    assert np.max(np.abs(a - back)) <= 2 * tol
    assert np.array_equal(perm[:k], piv[:k]) or np.max(np.abs(L @ L.T - back)) <= 4 * tol


@pytest.mark.parametrize("case", range(3))
def test_posterior_covariances_need_the_pivoted_factor(case):
    name, x, t, yerr = list(posterior_cases())[case]
    cov = posterior_cov(x, t, yerr)
    with pytest.raises(np.linalg.LinAlgError):                         # the reason for the feature
        np.linalg.cholesky(cov)
    # the threshold on the PRIOR's scale, M eps max diag K(t, t) (= 1 here): the rounding error of cov is that of K(t, t) and
    # K* K^-1 K*^T, however small their difference (the device's default; on the covariance's own scale -- 2e-16 for the first
    # case -- the factor would chase that rounding error)
    tol = len(cov) * EPS * 1.0
    L, piv, rank = pivoted_cholesky(cov, tol=tol)
    assert rank < len(cov)
    check_factor(cov, L, piv, rank, tol)


def test_exact_cases():
    rng = np.random.default_rng(7)
    v = rng.permutation(np.arange(1.0, 516.0)) / 7.0                   # distinct
    v[514], v[128], v[127] = 100.0, 99.0, 98.0
    tol = 30.0
    L, piv, rank = pivoted_cholesky(np.diag(v), tol=tol)
    assert rank == np.sum(v > tol)
    assert np.array_equal(piv[:rank], np.argsort(-v)[:rank]) and np.all(piv[rank:] == -1)
    want = np.zeros((515, 515))
    want[piv[:rank], np.arange(rank)] = np.sqrt(v[piv[:rank]])         # diag(sqrt(v)) in pivot order: no swaps are made
    assert np.array_equal(L, want)                                     # bit for bit
    L, piv, rank = pivoted_cholesky(np.diag(v))
    assert rank == 515 and np.array_equal(piv, np.argsort(-v))
    # the tie rule: the lowest index
    L, piv, rank = pivoted_cholesky(np.eye(515))
    assert rank == 515 and np.array_equal(piv, np.arange(515)) and np.array_equal(L, np.eye(515))
    L, piv, rank = pivoted_cholesky(np.zeros((5, 5)))
    assert rank == 0 and np.all(L == 0) and np.all(piv == -1)
    # a negative diagonal entry is never chosen
    a = np.diag([2.0, -3.0, 1.0, -1e-30])
    L, piv, rank = pivoted_cholesky(a, tol=0.0)
    assert rank == 2 and piv[:2].tolist() == [0, 2] and np.all(L[[1, 3]] == 0)
    # a non-finite diagonal
    for bad in (np.nan, np.inf):
        a = np.eye(4)
        a[2, 2] = bad
        L, piv, rank = pivoted_cholesky(a)
        assert rank == -1 and np.all(np.isnan(L))
    with pytest.raises(ValueError):
        pivoted_cholesky(np.zeros((3, 4)))
    assert "pivoted_cholesky" in utils.__all__


class NumpySolver(solver_np.DenseOracle):
    """A duck-typed solver: the reference protocol plus ``predict``, all NumPy (GP.predict would otherwise evaluate the kernel
    on the device)."""

    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        out = solver_np.gp_predict(self, kernel, self._x, r, xs, return_var=return_var, return_cov=return_cov)
        if return_var:
            return out[0], out[1], None
        if return_cov:
            return out[0], None, out[1]
        return out, None, None

    def compute(self, x, yerr):
        self._x = x
        super(NumpySolver, self).compute(x, yerr)


def _gp():
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 10, 60))
    y = np.sin(x) + 0.05 * rng.randn(60)
    gp = GP(1.3 * kernels.ExpSquaredKernel(0.8), mean=0.4, solver=NumpySolver)
    gp.compute(x, 0.05)
    return gp, y, np.linspace(-1, 11, 83)


@pytest.mark.parametrize("size", [1, 5])
def test_gp_sample_conditional_over_a_numpy_solver(size):
    gp, y, t = _gp()
    assert not hasattr(gp.solver, "sample_conditional")
    mu, cov = gp.predict(y, t)
    # "svd" and the default: today's path, draw for draw
    np.random.seed(42)
    want = multivariate_gaussian_samples(cov, size, mean=mu)
    for kw in ({}, {"factor": "svd"}):
        np.random.seed(42)
        got = gp.sample_conditional(y, t, size, **kw)
        assert got.shape == ((83,) if size == 1 else (size, 83)) and np.array_equal(got, want)
    # "cholesky": one call of standard_normal((size, M)), then the affine law
    np.random.seed(42)
    got = gp.sample_conditional(y, t, size, factor="cholesky")
    assert got.shape == ((83,) if size == 1 else (size, 83)) and np.all(np.isfinite(got))
    np.random.seed(42)
    z = np.random.standard_normal((size, 83))
    L, piv, rank = pivoted_cholesky(cov)
    assert 0 < rank < 83
    affine_law(np.atleast_2d(got), mu, z, L, rank, 83)
    with pytest.raises(ValueError, match="factor"):
        gp.sample_conditional(y, t, size, factor="qr")
    with pytest.raises(ValueError, match="factor"):
        gp.sample(t, size, factor="eig")
    with pytest.raises(ValueError, match="factor"):
        gp.sample_conditional_batch(np.zeros((1, len(gp))), y, t, size, factor=None)


def test_gp_sample_conditional_batch_over_a_numpy_solver():
    gp, y, t = _gp()
    v0 = gp.get_parameter_vector()
    vectors = np.array([v0, v0 + 0.2, v0 - 0.1])
    before = gp.solver
    np.random.seed(9)
    got = gp.sample_conditional_batch(vectors, y, t, size=4, factor="cholesky")
    assert got.shape == (3, 4, 83) and np.all(np.isfinite(got))
    assert np.array_equal(gp.get_parameter_vector(), v0) and gp.computed and gp.solver is before
    np.random.seed(9)
    z = np.random.standard_normal((3, 4, 83))
    mu, cov = gp.predict_batch(vectors, y, t, return_cov=True)
    for b in range(3):
        L, piv, rank = pivoted_cholesky(cov[b])
        affine_law(got[b], mu[b], z[b], L, rank, 83)
    np.random.seed(9)
    one = gp.sample_conditional_batch(vectors, y, t, size=1, factor="cholesky")
    assert one.shape == (3, 83)


def test_header_declares_the_entry_points_with_their_comments():
    raw = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"int\s+gh_dev_pstrf\(double\* a, int64_t lda, int64_t stride_a, int64_t m, int32_t nbatch, double tol,\s*"
                     r"double\* l, int64_t ldl, int64_t stride_l, int64_t\* piv, int64_t\* rank, double\* resid_diag, "
                     r"void\* stream\);", text)
    assert re.search(r"int\s+gh_chol_sample_conditional\(gh_chol\* s, gh_kernel\* k, const double\* r\s*, const double\* xs, "
                     r"int64_t m,\s*const double\* z\s*, int64_t nz, double tol, double\* mu\s*,\s*double\* draws\s*, "
                     r"double\* fac\s*, int64_t\* rank\);", text)
    assert re.search(r"int\s+gh_chol_sample_conditional_batch\(gh_chol\* s, gh_kernel\* k, const double\* params, int32_t nbatch,",
                     text)
    assert re.search(r"int\s+gh_kernel_sample\(gh_kernel\* k, const double\* t, int64_t m, double jitter, const double\* z, "
                     r"int64_t nz, double tol,\s*double\* draws\s*, double\* fac\s*, int64_t\* rank\);", text)
    # each has a comment in front of it that names the reference lines it replaces
    for name in ("gh_dev_pstrf", "gh_chol_sample_conditional", "gh_chol_sample_conditional_batch", "gh_kernel_sample"):
        at = re.search(r"\*/\s*int\s+" + name + r"\(", raw)
        assert at, name
        comment = raw[raw.rfind("/*", 0, at.start()):at.start()]
        assert "utils.py:11-33" in comment and "gp.py" in comment, name
        assert hasattr(N.lib, name)
    _vp, _i64, _i32, _d = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_double
    assert N.SIGNATURES["gh_dev_pstrf"] == (ctypes.c_int, [_vp, _i64, _i64, _i64, _i32, _d, _vp, _i64, _i64, _vp, _vp, _vp, _vp])
    assert N.SIGNATURES["gh_chol_sample_conditional"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp])
    assert N.SIGNATURES["gh_kernel_sample"] == (ctypes.c_int, [_vp, _vp, _i64, _d, _vp, _i64, _d, _vp, _vp, _vp])
    assert N.SIGNATURES["gh_chol_sample_conditional_batch"] == (
        ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _d, _vp, _vp, _vp, _vp, _vp])


def test_native_calls_reject_bad_arguments_without_a_gpu():
    buf = np.zeros(16)
    idx = np.zeros(4, dtype=np.int64)
    with pytest.raises(ValueError):                                    # m < 1
        N.check(N.lib.gh_dev_pstrf(N.ptr(buf), 4, 16, 0, 1, -1.0, N.ptr(buf), 4, 16, N.ptr(idx), N.ptr(idx), None, None))
    with pytest.raises(ValueError):                                    # negative batch
        N.check(N.lib.gh_dev_pstrf(N.ptr(buf), 4, 16, 4, -1, -1.0, N.ptr(buf), 4, 16, N.ptr(idx), N.ptr(idx), None, None))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_sample_conditional_batch(None, None, None, 1, None, 1, 1, None, None, None, 1, None, 1, -1.0,
                                                       None, None, None, None, None))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_kernel_sample(None, None, 1, 0.0, None, 1, -1.0, None, None, None))
    from george_amd import BasicSolver
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):
        s.sample_conditional(s.kernel, np.zeros(3), np.zeros((2, 1)), np.zeros((1, 2)))
    assert BasicSolver.sample_batch_bytes(468, 250, 16) > BasicSolver.predict_batch_bytes(468, 250, return_cov=True)
