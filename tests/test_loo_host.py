"""Leave-one-out cross-validation on the host side (no GPU): the ABI table, the argument checks that run before any device
call, and the generic NumPy branch of ``GP.loo_*`` on a stand-in solver that offers nothing but ``compute``,
``apply_inverse``, ``get_inverse`` and ``log_determinant``, against tests/loo_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

import loo_ref as R
from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from george_amd.modeling import Model
from oracle import kernels_np, solver_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


class NoiseRamp(Model):
    parameter_names = ("a", "c")

    def get_value(self, t):
        return self.a + self.c * t


class MinimalSolver(object):
    """the least a duck-typed solver offers (HODLRSolver, MultiGPUSolver and the reference's solvers offer more)"""

    def __init__(self, kernel):
        self.kernel = kernel
        self.computed = False
        self.log_determinant = None

    def compute(self, x, yerr):
        Kmat = np.array(solver_np.kernel_matrix(self.kernel, x), dtype=np.float64)
        Kmat[np.diag_indices_from(Kmat)] += yerr ** 2
        self._factor = cho_factor(Kmat, lower=True)
        self.log_determinant = 2.0 * np.sum(np.log(np.diag(self._factor[0])))
        self.computed = True

    def apply_inverse(self, y, in_place=False):
        return cho_solve(self._factor, y)

    def get_inverse(self):
        return cho_solve(self._factor, np.eye(len(self._factor[0])))


def test_signature_table_and_header_agree():
    text = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int gh_chol_loo(gh_chol* s, gh_kernel* k, const uint32_t* which , const double* r, double* lpd_sum, double* resid , "
            "double* var , double* lpd , double* grad , double* v , double* diagB );") in text
    assert ("int gh_chol_loo_objective(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr, "
            "const double* r, const uint32_t* which, double* logdet, double* lpd_sum, double* resid, double* var, double* grad, "
            "double* v, double* diagB);") in text
    _vp, _i64, _i32, _pd = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)
    assert N.SIGNATURES["gh_chol_loo"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, _pd, _vp, _vp, _vp, _vp, _vp, _vp])
    assert N.SIGNATURES["gh_chol_loo_objective"] == (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _pd, _pd,
                                                                    _vp, _vp, _vp, _vp, _vp])
    for name in ("gh_chol_loo", "gh_chol_loo_objective"):
        assert hasattr(N.lib, name)
    assert ctypes.sizeof(N.gh_chol_opts) == 8 * 4 and ctypes.sizeof(N.gh_chol_profile) == 11 * 8


def test_native_calls_reject_bad_arguments_without_a_gpu():
    out, out2 = ctypes.c_double(0.0), ctypes.c_double(0.0)
    buf = np.zeros(4)
    with pytest.raises(ValueError):                                   # no handle
        N.check(N.lib.gh_chol_loo(None, None, None, N.ptr(buf), ctypes.byref(out), N.ptr(buf), N.ptr(buf), None, None, None, None))
    with pytest.raises(ValueError):                                   # no residual
        N.check(N.lib.gh_chol_loo_objective(None, None, N.ptr(buf), 4, 1, N.ptr(buf), None, None, ctypes.byref(out),
                                            ctypes.byref(out2), N.ptr(buf), N.ptr(buf), None, None, None))
    with pytest.raises(ValueError):                                   # a gradient without a mask
        N.check(N.lib.gh_chol_loo_objective(None, None, N.ptr(buf), 4, 1, N.ptr(buf), N.ptr(buf), None, ctypes.byref(out),
                                            ctypes.byref(out2), N.ptr(buf), N.ptr(buf), N.ptr(buf), None, None))
    with pytest.raises(ValueError):                                   # no handle, everything else in place
        N.check(N.lib.gh_chol_loo_objective(None, None, N.ptr(buf), 4, 1, N.ptr(buf), N.ptr(buf), None, ctypes.byref(out),
                                            ctypes.byref(out2), N.ptr(buf), N.ptr(buf), None, None, None))
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):                # never computed
        s.loo(np.zeros(3))
    with pytest.raises(ValueError):
        s.loo_objective(np.zeros((4, 1)), 0.1, np.zeros(3))           # residual of another length
    with pytest.raises(RuntimeError):
        s.loo_objective(np.zeros((4, 2)), 0.1, np.zeros(4))           # input dimension
    import george_amd
    if george_amd.device_count() == 0:
        # no device: nothing quietly computes on the host instead
        gp = GP(kernels.ExpSquaredKernel(1.0))
        with pytest.raises(RuntimeError):
            gp.loo_nll_and_grad(gp.get_parameter_vector(), np.zeros(4)) if hasattr(gp, "_x") else gp.loo_predict(np.zeros(4))
        gp._x, gp._yerr2 = np.arange(4.0)[:, None], np.full(4, 0.01)
        with pytest.raises(RuntimeError):
            gp.loo_nll_and_grad(gp.get_parameter_vector(), np.zeros(4), quiet=False)


def test_only_the_dense_solver_offers_the_device_form():
    # HODLRSolver derives from BasicSolver: the entry points that take a dense handle must not come along
    from george_amd import HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver
    assert callable(BasicSolver.loo) and callable(BasicSolver.loo_objective)
    for cls in (HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver):
        assert not callable(getattr(cls, "loo", None)) and not callable(getattr(cls, "loo_objective", None))
        assert callable(cls.apply_inverse) and callable(cls.get_inverse)


def _host_gradient(kernel):
    """``kernel.get_gradient`` is a device call: on a machine without one the oracle's evaluator stands in for it"""
    return lambda x: kernels_np.gradient_symmetric(kernel, np.ascontiguousarray(x, dtype=np.float64))[:, :, kernel.unfrozen_mask]


def _gp(solver=MinimalSolver):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6) + 0.4 * kernels.Matern32Kernel(2.5)
    kernel.freeze_parameter("k2:k1:log_constant")
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=np.log(0.02), c=0.05), fit_white_noise=True,
            solver=solver)
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(0.0, 10.0, 60))
    yerr = 0.15 + 0.05 * rng.rand(60)
    y = 0.3 * x - 1.0 + np.sin(2.0 * x) + 0.2 * rng.randn(60)
    return gp, x, yerr, y


def test_generic_branch_matches_the_reference(monkeypatch):
    gp, x, yerr, y = _gp()
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    gp.compute(x, yerr)
    assert not hasattr(gp.solver, "loo") and len(gp) == 2 + 2 + 3 and len(gp.kernel) == 3
    wn = np.exp(np.log(0.02) + 0.05 * x)
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + wn), y - (0.25 * x - 0.8))
    mu, var = gp.loo_predict(y)
    L = gp.loo_log_likelihood(y)
    lpd = gp.loo_log_likelihood(y, pointwise=True)
    ratios = dict(resid=ref.ratio("resid", y - mu), var=ref.ratio("var", var), L=ref.ratio("L", L), lpd=ref.ratio("lpd", lpd))
    print("kappa %.3g, error / tolerance %s" % (ref.kappa, ratios))
    assert max(ratios.values()) <= 1.0
    assert lpd.shape == (60,) and abs(np.sum(lpd) - L) <= 1e-12 * ref.S_L
    assert np.array_equal(gp.loo_predict(y, return_var=False), mu)
    # mean | white noise | kernel (the frozen amplitude left out), assembled from the reference's pieces
    mask = gp.kernel.unfrozen_mask
    assert list(mask) == [True, True, False, True]
    mg, ng = np.stack([x, np.ones_like(x)]), np.stack([np.ones_like(x), x])
    g_ref = np.concatenate([mg @ ref.v, (ng * (wn * ref.diagB)[None, :]).sum(axis=1), ref.g[mask]])
    g_tol = np.concatenate([np.abs(mg) @ np.full(60, ref.tol("v")), (np.abs(ng) * wn[None, :]).sum(axis=1) * ref.tol("diagB"),
                            ref.tol("g")[mask]])
    g = gp.grad_loo_log_likelihood(y)
    ratio = R.Ref._ratio(g - g_ref, g_tol)
    print("gradient error / tolerance %.3g" % ratio)
    assert g.shape == (7,) and ratio <= 1.0
    # the optimiser's form: same numbers, negated; a new vector recomputes
    p = gp.get_parameter_vector()
    val, grad = gp.loo_nll_and_grad(p, y)
    assert val == -L and np.array_equal(grad, -g)
    val2, grad2 = gp.loo_nll_and_grad(p + 0.01, y)
    assert gp.computed and val2 != val and np.all(np.isfinite(grad2))
    with pytest.raises(ValueError):
        gp.loo_log_likelihood(y[:-1])


def test_quiet_mode_and_the_prior(monkeypatch):
    kernel = kernels.CosineKernel(log_period=0.0, bounds=dict(log_period=(-1.0, 1.0)))      # rank 2: singular without noise
    gp = GP(kernel, white_noise=-1000.0, solver=MinimalSolver)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    x = np.linspace(0.0, 3.0, 50)
    y = np.sin(x)
    with pytest.raises(np.linalg.LinAlgError):
        gp.compute(x, 0.0)
    gp._x, gp._yerr2 = x[:, None], np.zeros(50)
    assert gp.loo_log_likelihood(y, quiet=True) == -np.inf
    lp = gp.loo_log_likelihood(y, quiet=True, pointwise=True)
    assert lp.shape == (50,) and np.all(lp == -np.inf)
    assert np.array_equal(gp.grad_loo_log_likelihood(y, quiet=True), np.zeros(1))
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector(), y)
    assert val == np.inf and np.array_equal(grad, np.zeros(1))
    with pytest.raises(np.linalg.LinAlgError):
        gp.loo_log_likelihood(y)
    with pytest.raises(np.linalg.LinAlgError):
        gp.loo_nll_and_grad(gp.get_parameter_vector(), y, quiet=False)
    # outside the prior nothing is computed
    gp.compute(x, 0.3)
    solver = gp.solver
    val, grad = gp.loo_nll_and_grad(np.array([2.0]), y)
    assert val == np.inf and np.array_equal(grad, np.zeros(1)) and gp.solver is solver
