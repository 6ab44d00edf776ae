"""Leave-group-out cross-validation on the host side (no GPU): the ABI table, the conversion of a ``groups`` argument, the
argument checks that run before any device call, and the generic NumPy branch of ``GP.lgo_*`` on a stand-in solver that
offers nothing but ``compute``, ``apply_inverse``, ``get_inverse`` and ``log_determinant``, against tests/lgo_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import lgo_ref as R
from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from test_loo_host import LinearMean, NoiseRamp, MinimalSolver, _host_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_table_and_header_agree():
    text = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    assert ("int gh_chol_lgo(gh_chol* s, gh_kernel* k, const uint32_t* which , const double* r, const int64_t* order , "
            "const int64_t* start , int64_t ngroups, double* lpd_sum, double* resid , double* var , double* lpd , double* cov , "
            "double* grad , double* v , double* diagB );") in text
    _vp, _i64, _pd = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
    assert N.SIGNATURES["gh_chol_lgo"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _pd, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
    assert hasattr(N.lib, "gh_chol_lgo")
    head = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    comment = head[head.index("Leave-group-out cross-validation on a computed handle"):head.index("int  gh_chol_lgo(")]
    for piece in ("no reference lines correspond", "C_gg^-1 alpha_g", "1/2 log|C_gg|", "1/2 (C_gg^-1 + u_g u_g^T)", "- C W C"):
        assert piece in comment, piece


def test_only_the_dense_solver_offers_the_device_form():
    from george_amd import HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver
    assert callable(BasicSolver.lgo) and BasicSolver.LGO_MAX_GROUP == 128
    for cls in (HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver):
        assert not callable(getattr(cls, "lgo", None))
        assert callable(cls.apply_inverse) and callable(cls.get_inverse)


def _gp(solver=MinimalSolver, n=60):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6) + 0.4 * kernels.Matern32Kernel(2.5)
    kernel.freeze_parameter("k2:k1:log_constant")
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=np.log(0.02), c=0.05), fit_white_noise=True,
            solver=solver)
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.15 + 0.05 * rng.rand(n)
    y = 0.3 * x - 1.0 + np.sin(2.0 * x) + 0.2 * rng.randn(n)
    return gp, x, yerr, y


# ------------------------------------------------------------------ the groups argument
def test_groups_argument_becomes_order_and_start():
    gp, x, yerr, y = _gp()
    gp._x = x[:, None]                                   # (the conversion needs the number of points only)
    order, start = gp._lgo_groups(16)
    assert order.dtype == start.dtype == np.int64
    assert np.array_equal(order, np.arange(60)) and np.array_equal(start, [0, 16, 32, 48, 60])
    order, start = gp._lgo_groups(np.int64(60))
    assert np.array_equal(start, [0, 60])
    order, start = gp._lgo_groups(1000)
    assert np.array_equal(start, [0, 60])
    # any integers, in any order: groups numbered by sorted unique label, the points of a group as they appear in the data
    labels = np.array([7, -3, 7, 100, -3, -3] * 10)
    order, start = gp._lgo_groups(labels)
    assert np.array_equal(start, [0, 30, 50, 60])
    assert np.array_equal(order[:30], np.flatnonzero(labels == -3)) and np.array_equal(order[30:50], np.flatnonzero(labels == 7))
    assert np.array_equal(order[50:], np.flatnonzero(labels == 100))
    for lab in (labels.astype(np.int16), list(labels), (labels + 3).astype(np.uint8)):
        o2, s2 = gp._lgo_groups(lab)
        assert np.array_equal(s2, start) and np.array_equal(o2, order)
    o3, s3 = R.order_start(labels)
    assert np.array_equal(o3, order) and np.array_equal(s3, start)
    for bad in (labels[:-1], labels.astype(float), labels.reshape(6, 10), 0, -4, 2.0, True, "ab", None):
        with pytest.raises(ValueError):
            gp._lgo_groups(bad)


def test_argument_errors_raise_before_any_device_call(monkeypatch):
    calls = []
    monkeypatch.setattr(N.lib, "gh_chol_lgo", lambda *a: calls.append(a) or 0, raising=False)
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):                # never computed
        s.lgo(np.zeros(3), np.arange(3), np.array([0, 3]))
    s._need = lambda: 1                                               # a stand-in for a computed handle
    s._n, s._dk = 6, type("Dk", (), {"size": 1, "handle": None})()
    r, order, start = np.zeros(6), np.arange(6), np.array([0, 2, 6])
    for args in ((np.zeros(5), order, start), (r, order[:-1], start), (r, order, np.array([0])),
                 (r, order, start, np.ones(2)), (r, order, start, np.ones((1, 1)))):
        with pytest.raises(ValueError):
            s.lgo(*args)
    with pytest.raises(ValueError):                                   # the covariance blocks of a group too large cannot be sized
        s.lgo(np.zeros(6), order, np.array([0, 6, 2]), want_cov=True)
    assert not calls
    gp, x, yerr, y = _gp()
    gp._x = x[:, None]
    for method in (gp.lgo_predict, gp.lgo_log_likelihood, gp.grad_lgo_log_likelihood):
        with pytest.raises(ValueError):
            method(y, np.zeros(59, dtype=int))
        with pytest.raises(ValueError):
            method(y, np.zeros(60))
    with pytest.raises(ValueError):
        gp.lgo_nll_and_grad(gp.get_parameter_vector(), y, 0)
    out, buf, idx = ctypes.c_double(0.0), np.zeros(4), np.arange(4, dtype=np.int64)
    monkeypatch.undo()
    with pytest.raises(ValueError):                                   # no handle
        N.check(N.lib.gh_chol_lgo(None, None, None, N.ptr(buf), N.ptr(idx), N.ptr(idx), 1, ctypes.byref(out), N.ptr(buf),
                                  N.ptr(buf), None, None, None, None, None))


# ------------------------------------------------------------------ the generic branch
@pytest.mark.parametrize("form", ["windows", "labels"])
def test_generic_branch_matches_the_reference(monkeypatch, form):
    gp, x, yerr, y = _gp()
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    gp.compute(x, yerr)
    assert not hasattr(gp.solver, "lgo") and len(gp) == 2 + 2 + 3 and len(gp.kernel) == 3
    groups = 7 if form == "windows" else np.random.RandomState(5).randint(-2, 4, 60) * 3
    order, start = R.order_start(np.arange(60) // 7 if form == "windows" else groups)
    G = len(start) - 1
    wn = np.exp(np.log(0.02) + 0.05 * x)
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + wn), y - (0.25 * x - 0.8), order, start)
    mu, var, cov = gp.lgo_predict(y, groups, return_cov=True)
    L = gp.lgo_log_likelihood(y, groups)
    lpd = gp.lgo_log_likelihood(y, groups, pointwise=True)
    ratios = dict(resid=ref.ratio("resid", y - mu), var=ref.ratio("var", var), L=ref.ratio("L", L), lpd=ref.ratio("lpd", lpd),
                  cov=ref.ratio("cov", cov))
    print("kappa %.3g, error / tolerance %s" % (ref.kappa, ratios))
    assert max(ratios.values()) <= 1.0
    assert lpd.shape == (G,) and abs(np.sum(lpd) - L) <= 1e-12 * ref.S_L
    assert [c.shape for c in cov] == [(m, m) for m in np.diff(start)]
    assert np.array_equal(gp.lgo_predict(y, groups, return_var=False), mu)
    mu2, var2 = gp.lgo_predict(y, groups)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    # the same against G refits
    bL, blpd, bresid, bvar, bcov = R.brute_force(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + wn), y - (0.25 * x - 0.8), order, start)
    assert R.Ref._ratio(L - bL, ref.tol("L")) <= 1.0 and R.Ref._ratio((y - mu) - bresid, ref.tol("resid")) <= 1.0
    # mean | white noise | kernel (the frozen amplitude left out), assembled from the reference's pieces
    mask = gp.kernel.unfrozen_mask
    assert list(mask) == [True, True, False, True]
    mg, ng = np.stack([x, np.ones_like(x)]), np.stack([np.ones_like(x), x])
    g_ref = np.concatenate([mg @ ref.v, (ng * (wn * ref.diagB)[None, :]).sum(axis=1), ref.g[mask]])
    g_tol = np.concatenate([np.abs(mg) @ np.full(60, ref.tol("v")), (np.abs(ng) * wn[None, :]).sum(axis=1) * ref.tol("diagB"),
                            ref.tol("g")[mask]])
    g = gp.grad_lgo_log_likelihood(y, groups)
    ratio = R.Ref._ratio(g - g_ref, g_tol)
    print("gradient error / tolerance %.3g" % ratio)
    assert g.shape == (7,) and ratio <= 1.0
    # the optimiser's form: same numbers, negated; a new vector recomputes
    p = gp.get_parameter_vector()
    val, grad = gp.lgo_nll_and_grad(p, y, groups)
    assert val == -L and np.array_equal(grad, -g)
    val2, grad2 = gp.lgo_nll_and_grad(p + 0.01, y, groups)
    assert gp.computed and val2 != val and np.all(np.isfinite(grad2))
    with pytest.raises(ValueError):
        gp.lgo_log_likelihood(y[:-1], groups)


def test_one_point_groups_are_leave_one_out(monkeypatch):
    gp, x, yerr, y = _gp()
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    gp.compute(x, yerr)
    mu, var = gp.lgo_predict(y, 1)
    mu1, var1 = gp.loo_predict(y)
    assert np.allclose(mu, mu1, rtol=0, atol=1e-10) and np.allclose(var, var1, rtol=1e-10)
    assert np.isclose(gp.lgo_log_likelihood(y, np.arange(60)[::-1]), gp.loo_log_likelihood(y), rtol=1e-11)
    assert np.allclose(gp.grad_lgo_log_likelihood(y, 1), gp.grad_loo_log_likelihood(y), rtol=1e-8, atol=1e-8)


def test_quiet_mode_and_the_prior(monkeypatch):
    kernel = kernels.CosineKernel(log_period=0.0, bounds=dict(log_period=(-1.0, 1.0)))      # rank 2: singular without noise
    gp = GP(kernel, white_noise=-1000.0, solver=MinimalSolver)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    x = np.linspace(0.0, 3.0, 50)
    y = np.sin(x)
    with pytest.raises(np.linalg.LinAlgError):
        gp.compute(x, 0.0)
    gp._x, gp._yerr2 = x[:, None], np.zeros(50)
    assert gp.lgo_log_likelihood(y, 8, quiet=True) == -np.inf
    lp = gp.lgo_log_likelihood(y, 8, quiet=True, pointwise=True)
    assert lp.shape == (7,) and np.all(lp == -np.inf)
    assert np.array_equal(gp.grad_lgo_log_likelihood(y, 8, quiet=True), np.zeros(1))
    val, grad = gp.lgo_nll_and_grad(gp.get_parameter_vector(), y, 8)
    assert val == np.inf and np.array_equal(grad, np.zeros(1))
    with pytest.raises(np.linalg.LinAlgError):
        gp.lgo_log_likelihood(y, 8)
    # outside the prior nothing is computed
    gp.compute(x, 0.3)
    solver = gp.solver
    val, grad = gp.lgo_nll_and_grad(np.array([2.0]), y, 8)
    assert val == np.inf and np.array_equal(grad, np.zeros(1)) and gp.solver is solver


# ------------------------------------------------------------------ a group beyond the device form's 128 points
class RecordingSolver(BasicSolver):
    """a BasicSolver whose device calls are the stand-in's host arithmetic, and which records what GP asks of it"""
    calls = []

    def __init__(self, kernel, **kwargs):
        super(RecordingSolver, self).__init__(kernel, **kwargs)
        self._host = MinimalSolver(kernel)

    def compute(self, x, yerr):
        self._host.compute(x, yerr)
        self._computed, self._log_det = True, self._host.log_determinant

    def apply_inverse(self, y, in_place=False):
        RecordingSolver.calls.append("apply_inverse")
        return self._host.apply_inverse(y)

    def get_inverse(self):
        RecordingSolver.calls.append("get_inverse")
        return self._host.get_inverse()

    def lgo(self, r, order, start, which=None, want_cov=False):
        RecordingSolver.calls.append(("lgo", int(np.max(np.diff(start)))))
        raise RuntimeError("stub: the device form was asked")


def test_a_group_of_129_points_takes_the_generic_branch(monkeypatch):
    n = 140
    gp, x, yerr, y = _gp(RecordingSolver, n=n)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    gp.compute(x, yerr)
    assert isinstance(gp.solver, BasicSolver) and callable(gp.solver.lgo)
    RecordingSolver.calls[:] = []
    with pytest.raises(RuntimeError, match="stub"):                   # 128 points: the device form
        gp.lgo_log_likelihood(y, 128)
    assert RecordingSolver.calls == [("lgo", 128)]
    RecordingSolver.calls[:] = []
    labels = (np.arange(n) >= 129).astype(int)                        # 129 points and 11
    order, start = R.order_start(labels)
    L = gp.lgo_log_likelihood(y, labels)
    g = gp.grad_lgo_log_likelihood(y, labels)
    assert RecordingSolver.calls and all(c in ("apply_inverse", "get_inverse") for c in RecordingSolver.calls)
    wn = np.exp(np.log(0.02) + 0.05 * x)
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + wn), y - (0.25 * x - 0.8), order, start)
    assert ref.ratio("L", L) <= 1.0 and g.shape == (7,)
    assert R.Ref._ratio(g[-3:] - ref.g[gp.kernel.unfrozen_mask], ref.tol("g")[gp.kernel.unfrozen_mask]) <= 1.0
