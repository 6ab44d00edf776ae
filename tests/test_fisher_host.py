"""The expected information of the hyper-parameters on the host side (no GPU): the ABI table, the argument checks that run
before any device call, and the generic NumPy branch of ``GP.fisher_information`` / ``GP.parameter_covariance`` on a stand-in
solver that offers nothing but ``compute``, ``apply_inverse``, ``get_inverse`` and ``log_determinant``, against
tests/fisher_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

import fisher_ref as R
from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from george_amd.modeling import Model
from oracle import kernels_np, solver_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b

    def compute_gradient(self, t):
        return np.stack([t, np.ones_like(t)])


class NoiseRamp(Model):
    parameter_names = ("a", "c")

    def get_value(self, t):
        return self.a + self.c * t

    def compute_gradient(self, t):
        return np.stack([np.ones_like(t), t])


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


def _host_gradient(kernel):
    """``kernel.get_gradient`` is a device call: on a machine without one the oracle's evaluator stands in for it"""
    return lambda x: kernels_np.gradient_symmetric(kernel, np.ascontiguousarray(x, dtype=np.float64))[:, :, kernel.unfrozen_mask]


def _data(n=60):
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    return x, 0.15 + 0.05 * rng.rand(n)


def _gp(monkeypatch, mean, noise):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6) + 0.4 * kernels.Matern32Kernel(2.5)
    kernel.freeze_parameter("k2:k1:log_constant")
    kw = dict(solver=MinimalSolver)
    if mean:
        kw["mean"] = LinearMean(m=0.25, b=-0.8)
    if noise:
        kw.update(white_noise=NoiseRamp(a=np.log(0.02), c=0.05), fit_white_noise=True)
    gp = GP(kernel, **kw)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    return gp


def test_signature_table_and_header_agree():
    text = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int gh_chol_fisher(gh_chol* s, gh_kernel* k, const uint32_t* which , const double* diag_rows , int32_t n_diag, "
            "int64_t max_bytes , double* fisher );") in text
    _vp, _i64, _i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    assert N.SIGNATURES["gh_chol_fisher"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _vp])
    assert hasattr(N.lib, "gh_chol_fisher")


def test_argument_checks_without_a_gpu():
    buf = np.zeros(4)
    with pytest.raises(ValueError):                                   # no handle
        N.check(N.lib.gh_chol_fisher(None, None, None, None, 0, 0, N.ptr(buf)))
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):                # never computed, as loo
        s.fisher()
    assert BasicSolver.fisher_bytes(300, 3) == 5 * 8 * 384 * 384 and BasicSolver.fisher_bytes(128, 0) == 2 * 8 * 128 * 128
    assert BasicSolver.FISHER_MAX_BYTES == BasicSolver._POOL_MAX_BYTES
    # only the dense solver offers the device form; the others go through get_inverse
    from george_amd import HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver
    assert callable(BasicSolver.fisher)
    for cls in (HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver):
        assert not callable(getattr(cls, "fisher", None)) and callable(cls.get_inverse)
    # nothing new is exported from the package
    import george_amd
    assert not any("fisher" in name.lower() for name in george_amd.__all__)


@pytest.mark.parametrize("mean,noise", [(True, False), (False, True), (True, True)])
def test_generic_branch_matches_the_reference(monkeypatch, mean, noise):
    gp = _gp(monkeypatch, mean, noise)
    x, yerr = _data()
    gp.compute(x, yerr)
    n_m, n_wn = 2 * mean, 2 * noise
    assert not hasattr(gp.solver, "fisher") and len(gp) == n_m + n_wn + 3 and len(gp.kernel) == 3
    F = gp.fisher_information()
    assert F.shape == (len(gp), len(gp)) and np.array_equal(F, F.T)
    # white noise | kernel against the reference; the frozen amplitude is absent
    wn = np.exp(np.log(0.02) + 0.05 * x) if noise else np.full_like(x, 1.25e-12)      # (the GP's default white noise)
    rows = np.stack([wn, wn * x]) if noise else None
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + wn), rows)
    mask = gp.kernel.unfrozen_mask
    assert list(mask) == [True, True, False, True]
    keep = np.concatenate([np.arange(n_wn), n_wn + np.flatnonzero(mask)])
    ratio = ref.ratio(F[n_m:, n_m:], keep)
    print("kappa %.3g, error / tolerance %.3g" % (ref.kappa, ratio))
    assert ratio <= 1.0
    if mean:
        # the mean block under the same rule, and cross blocks of exactly 0
        K = np.array(solver_np.kernel_matrix(gp.kernel, x[:, None]), dtype=np.float64)
        K[np.diag_indices(len(x))] += yerr ** 2 + wn
        mg = np.stack([x, np.ones_like(x)]).astype(R.LD)
        Fm = np.dot(mg, np.dot(R.refined_inverse(K), mg.T)).astype(np.float64)
        d = np.sqrt(np.diag(Fm))
        m_ratio = R.Ref._ratio(F[:2, :2] - Fm, R.C_TOL * R.U * ref.kappa * np.outer(d, d))
        print("mean block error / tolerance %.3g" % m_ratio)
        assert m_ratio <= 1.0
        assert np.all(F[:2, 2:] == 0.0) and np.all(F[2:, :2] == 0.0)
    # the Cramer-Rao covariance inverts it
    C = gp.parameter_covariance()
    kappa_F = np.linalg.cond(F)
    resid = np.max(np.abs(np.dot(C, F) - np.eye(len(gp))))
    print("kappa(F) %.3g, |C F - I| %.3g" % (kappa_F, resid))
    assert C.shape == F.shape and resid <= kappa_F * 1e-12
    # it needs no y and keeps the factorisation
    assert gp.computed


def test_singular_information_raises(monkeypatch):
    # two interchangeable constant factors: their derivatives are the same matrix
    kernel = kernels.ConstantKernel(log_constant=np.log(1.3)) * kernels.ConstantKernel(log_constant=np.log(0.7)) \
        * kernels.ExpSquaredKernel(0.6)
    gp = GP(kernel, solver=MinimalSolver)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    x, yerr = _data(40)
    gp.compute(x, yerr)
    F = gp.fisher_information()
    assert F.shape == (3, 3) and np.all(np.isfinite(F))
    with pytest.raises(np.linalg.LinAlgError):
        gp.parameter_covariance()


def test_no_unfrozen_parameter_and_uncomputed(monkeypatch):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6)
    kernel.freeze_all_parameters()
    gp = GP(kernel, solver=MinimalSolver)
    with pytest.raises(RuntimeError, match="compute the model first"):      # as recompute
        gp.fisher_information()
    with pytest.raises(RuntimeError, match="compute the model first"):
        gp.parameter_covariance()
    x, yerr = _data(20)
    gp.compute(x, yerr)
    assert len(gp) == 0
    assert gp.fisher_information().shape == (0, 0) and gp.parameter_covariance().shape == (0, 0)
