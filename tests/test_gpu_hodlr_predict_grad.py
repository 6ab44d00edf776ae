"""HODLRSolver.predict / HODLRSolver.grad (gh_hodlr_predict, gh_hodlr_grad): the device-resident strip driver against
quantities it does not produce -- the definition through ``apply_inverse`` / ``get_inverse`` / ``kernel.get_value`` /
``kernel.get_gradient`` on the SAME factor, the dense solver's answer (the reference's own HODLR criterion,
tests/test_solvers.py:44-62), and the parent path of ``GP`` (a subclass with ``predict = grad = None``).

Tolerances.  predict: those of tests/test_gpu_solver.py::test_full_size_c5_properties (mu rtol=1e-9, atol=1e-11; var / cov
rtol=1e-7, atol=1e-12).  A case that misses one of them is bounded instead at ten times its recorded deviation on the scale
of the sum that cancels -- sum_i |Kts[j,i]| |W[i,j]| for var / cov, sum_i |Kts[j,i]| |alpha_i| for mu
(profiles/hodlr/predict_grad_parity.json, "predict_scaled"; above 1e-9 on that scale is a defect).  One does: the mean of
C4_density_4096, whose 4096 points lie within 0.16 length scales, so that alpha has entries of +-1e3 and sums of 8e4 in absolute
terms give means of order 0.1 -- the two summation orders differ by 5e-11, 6e-16 of that sum.
grad: capped by the project's gradient tolerance (rtol=1e-6, atol=1e-6, tests/test_gpu_solver.py:71) and bounded at ten times
the largest recorded  max_p |fused_p - generic_p| / S_p,  S_p = 1/2 sum_ij |A_ij| |dK_ij/dtheta_p|  ("grad_scaled" in the same
file: 5.1e-15 over all cases, 7.9e-16 at N = 32 768).  With GEORGE_AMD_PARITY_OUT=<file> every figure is also written there
(how the committed file was made); without a committed file the bound is the defect threshold 1e-9."""
import json
import os
import pickle

import numpy as np
import pytest

import zoo

from george_amd import kernels, GP, BasicSolver, HODLRSolver
from george_amd import _native as N
from george_amd.modeling import Model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCONF = zoo.hodlr_configs(kernels)
PARITY_FILE = os.path.join(ROOT, "profiles", "hodlr", "predict_grad_parity.json")
DEFECT = 1e-9
MU_TOL = dict(rtol=1e-9, atol=1e-11)
VAR_TOL = dict(rtol=1e-7, atol=1e-12)
GRAD_CAP = dict(rtol=1e-6, atol=1e-6)

try:
    with open(PARITY_FILE) as _f:
        PARITY = json.load(_f)
except (IOError, OSError):
    PARITY = {}
_rec = PARITY.get("grad_scaled", {})
GRAD_BOUND = 10.0 * max(_rec.values()) if _rec else DEFECT
MEASURED = {"grad_scaled": {}, "predict_scaled": {}, "predict_scaled_all": {}}


def _record(kind, key, value):
    MEASURED[kind][key] = float(value)
    print("%s %s %.3e" % (kind, key, value))
    out = os.environ.get("GEORGE_AMD_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def test_recorded_parity_is_below_the_defect_threshold():
    for kind in ("grad_scaled", "predict_scaled"):
        for key, v in PARITY.get(kind, {}).items():
            assert v <= DEFECT, (kind, key, v)


def _X(x):
    return np.ascontiguousarray(x.reshape(len(x), -1))


def _test_points(X, m, seed=5):
    """m points inside the data range, per coordinate"""
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(rng.uniform(X.min(axis=0), X.max(axis=0), (m, X.shape[1])))


def _solver(name):
    kernel, x, yerr, y, kw = HCONF[name]
    X = _X(x)
    s = HODLRSolver(kernel, **kw)
    s.compute(X, yerr)
    return kernel, X, yerr, y, s


def _predict_definition(kernel, X, s, r, t):
    """gp.py:532-545 through independent entry points on the same factor"""
    Kts = kernel.get_value(t, X)
    W = s.apply_inverse(np.ascontiguousarray(Kts.T))
    alpha = s.apply_inverse(r)
    mu = Kts @ alpha
    var = kernel.get_value(t, diag=True) - np.sum(Kts.T * W, axis=0)
    cov = kernel.get_value(t) - Kts @ W
    scale = np.sum(np.abs(Kts.T) * np.abs(W), axis=0)
    return mu, var, cov, scale, np.abs(Kts) @ np.abs(alpha)


def _close_or_recorded(key, got, want, scale, tol):
    dev = np.abs(got - want) / scale
    _record("predict_scaled_all", key, dev.max())
    if np.allclose(got, want, **tol):
        return
    _record("predict_scaled", key, dev.max())
    rec = PARITY.get("predict_scaled", {}).get(key)
    assert rec is not None and rec <= DEFECT and dev.max() <= 10 * rec, (key, dev.max(), rec, np.abs(got - want).max())


# ------------------------------------------------------------------ 1. the definition, same factor
@pytest.mark.parametrize("name", list(HCONF))
def test_predict_against_its_definition(name):
    kernel, X, yerr, y, s = _solver(name)
    t = _test_points(X, 300)
    mu0, var0, cov0, scale, scale_mu = _predict_definition(kernel, X, s, y, t)
    mu, var, cov = s.predict(kernel, y, t)
    assert var is None and cov is None
    _close_or_recorded(name + "/mu", mu, mu0, scale_mu, MU_TOL)
    mu_v, var, _ = s.predict(kernel, y, t, return_var=True)
    assert np.array_equal(mu_v, mu)
    _close_or_recorded(name + "/var", var, var0, scale, VAR_TOL)
    mu_c, _, cov = s.predict(kernel, y, t, return_cov=True)
    assert np.array_equal(mu_c, mu) and cov.shape == (300, 300)
    _close_or_recorded(name + "/cov", cov, cov0, np.sqrt(np.outer(scale, scale)), VAR_TOL)
    _close_or_recorded(name + "/diagcov", np.diag(cov), var, scale, VAR_TOL)


# ------------------------------------------------------------------ 2. the reference's criterion: the dense answer
@pytest.mark.parametrize("name", [k for k in HCONF if HCONF[k][4]["tol"] <= 1e-8])
def test_predict_against_the_dense_solver(name):
    kernel, x, yerr, y, kw = HCONF[name]
    X = _X(x)
    t = _test_points(X, 300)
    gh = GP(kernel, solver=HODLRSolver, **kw)
    gd = GP(kernel, solver=BasicSolver)
    gh.compute(X, yerr)
    gd.compute(X, yerr)
    assert callable(gh.solver.predict) and not gh.solver.dense_fallback
    mu_h, var_h = gh.predict(y, t, return_var=True)
    mu_d, var_d = gd.predict(y, t, return_var=True)
    assert np.allclose(mu_h, mu_d) and np.allclose(var_h, var_d)
    mu_h, cov_h = gh.predict(y, t)
    mu_d, cov_d = gd.predict(y, t)
    assert np.allclose(mu_h, mu_d) and np.allclose(cov_h, cov_d)


# ------------------------------------------------------------------ 4 / 5. the gradient against the generic branch, same factor
def _generic_grad(kernel, X, s, r):
    """gp.py:429-466 as GP's generic branch writes it, and the scale S_p of each parameter's sum"""
    alpha = s.apply_inverse(r)
    A = np.outer(alpha, alpha) - s.get_inverse()
    dK = kernel.get_gradient(X)
    g = 0.5 * np.einsum("ijk,ij", dK, A)
    S = 0.5 * np.einsum("ijk,ij", np.abs(dK), np.abs(A))
    return g, S, alpha, np.diag(A).copy()


def _check_grad(key, fused, generic, S):
    rel = np.abs(fused - generic) / S
    _record("grad_scaled", key, rel.max())
    assert np.allclose(fused, generic, **GRAD_CAP), (key, fused, generic)
    assert rel.max() <= GRAD_BOUND, (key, rel, GRAD_BOUND)


def _hyper_kernel():
    """docs/tutorials/hyper.rst:91-95: k1 + k2 * ExpSine2 + k3 + k4, eleven parameters"""
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _hyper_problem(n=1000):
    """n sorted 1-D inputs over 30 "years" (the tutorial's CO2 record is monthly over 40), error bars 0.5"""
    rng = np.random.RandomState(2024)
    x = np.sort(rng.uniform(1960.0, 1990.0, n))
    y = 340.0 + 1.3 * (x - 1975.0) + 3.0 * np.sin(2 * np.pi * x) - 340.0
    return _hyper_kernel(), x, 0.5 * np.ones(n), y, dict(min_size=100, tol=1e-8, seed=42)


def _grad_case(name):
    if name == "hyper1000":
        kernel, x, yerr, y, kw = _hyper_problem()
    else:
        kernel, x, yerr, y, kw = HCONF[name]
    return kernel, _X(x), yerr, y, kw


@pytest.mark.parametrize("name", ["solver1000", "c5like3d", "expsq2d", "m32_exhausted", "hyper1000"])
def test_grad_against_the_generic_branch(name):
    kernel, X, yerr, y, kw = _grad_case(name)
    assert len(X) <= 3001
    if name == "c5like3d":
        kernel.freeze_parameter(kernel.get_parameter_names()[0])
    try:
        s = HODLRSolver(kernel, **kw)
        s.compute(X, yerr)
        assert not s.dense_fallback
        mask = kernel.unfrozen_mask
        g0, S, alpha0, diag0 = _generic_grad(kernel, X, s, y)
        g, alpha, diagA = s.grad(y, mask.astype(np.uint32))
        assert g.shape == (kernel.full_size,)
        if name == "c5like3d":
            assert not mask.all() and np.all(g[~mask] == 0.0)
        _check_grad(name, g[mask], g0, S)
        assert np.allclose(alpha, alpha0, **MU_TOL)
        # diag(A): alpha_j^2 - K^-1[j, j], each term from a solve of another width than get_inverse()'s
        assert np.allclose(diagA, diag0, rtol=1e-9, atol=1e-9 * np.abs(diag0).max())
        g2, alpha2, diagA2 = s.grad(y, mask.astype(np.uint32))
        assert np.array_equal(g, g2) and np.array_equal(alpha, alpha2) and np.array_equal(diagA, diagA2)
    finally:
        if name == "c5like3d":
            kernel.thaw_parameter(kernel.get_parameter_names(include_frozen=True)[0])


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t.flatten() + self.b

    def compute_gradient(self, t):
        t = t.flatten()
        return np.vstack([t, np.ones_like(t)])


class ParentPathHODLR(HODLRSolver):
    """what ``GP`` saw before the fused methods existed: its generic NumPy branch, line for line"""
    predict = None
    grad = None


def test_grad_through_gp_against_the_parent_path():
    x, yerr, y = zoo.bench_data(1500)
    kw = dict(white_noise=np.log(0.02), fit_white_noise=True, mean=LinearMean(m=0.05, b=-0.2), fit_mean=True, tol=1e-10)
    k = lambda: np.var(y) * kernels.ExpSquaredKernel(1.0)          # noqa: E731
    gf = GP(k(), solver=HODLRSolver, **kw)
    gg = GP(k(), solver=ParentPathHODLR, **kw)
    gf.compute(x, yerr)
    gg.compute(x, yerr)
    assert callable(gf.solver.grad) and gg.solver.grad is None
    a, b = gf.grad_log_likelihood(y), gg.grad_log_likelihood(y)
    assert len(a) == 2 + 1 + 2
    assert np.allclose(a, b, **GRAD_CAP), (a, b)
    # the kernel block on its own scale; the mean and white-noise blocks are sums over alpha and diag(A)
    _, S, _, _ = _generic_grad(gf.kernel, gf._x, gf.solver, gf._residual(y))
    _check_grad("gp_mean_whitenoise_1500", a[3:], b[3:], S)
    assert np.allclose(a[:3], b[:3], rtol=1e-9, atol=1e-9 * np.abs(b[:3]).max())
    mu_f, var_f = gf.predict(y, x[::7] + 1e-3, return_var=True)
    mu_g, var_g = gg.predict(y, x[::7] + 1e-3, return_var=True)
    assert np.allclose(mu_f, mu_g, **MU_TOL) and np.allclose(var_f, var_g, **VAR_TOL)


# ------------------------------------------------------------------ 3. strips
def test_strips():
    name = "C4_3000_tol1e-4_seed7"
    kernel, X, yerr, y, s = _solver(name)
    t = _test_points(X, 200)
    which = np.ones(kernel.full_size, dtype=np.uint32)
    auto_mu, auto_var, _ = s.predict(kernel, y, t, return_var=True)
    _, _, auto_cov = s.predict(kernel, y, t, return_cov=True)
    auto_g, auto_alpha, auto_diag = s.grad(y, which)
    g0, S, _, _ = _generic_grad(kernel, X, s, y)
    _, _, _, scale, _ = _predict_definition(kernel, X, s, y, t)
    old = N.lib.gh_debug_set_hodlr_strip_cols(64)
    try:
        assert old == 0
        full_mu, full_var, _ = s.predict(kernel, y, t, return_var=True)
        for m in (1, 63, 64, 65, 200):
            mu, var, _ = s.predict(kernel, y, t[:m], return_var=True)
            assert np.allclose(mu, auto_mu[:m], **MU_TOL)
            _close_or_recorded("%s/strips64_var_m%d" % (name, m), var, auto_var[:m], scale[:m], VAR_TOL)
            # t[:m] alone gives the first m rows of predicting t: the mean bit for bit (its sum does not depend on the
            # strip), the variance through solves of other widths
            assert np.array_equal(mu, full_mu[:m])
            assert np.allclose(var, full_var[:m], **VAR_TOL)
            mu_only, _, _ = s.predict(kernel, y, t[:m])
            assert np.array_equal(mu_only, mu)
        _, _, cov = s.predict(kernel, y, t, return_cov=True)
        assert np.allclose(cov, auto_cov, **VAR_TOL)
        g, alpha, diagA = s.grad(y, which)                     # 47 strips of 64 columns
        _check_grad(name + "/strips64", g, g0, S)
        _check_grad(name + "/auto", auto_g, g0, S)
        assert np.allclose(g, auto_g, **GRAD_CAP)
        assert np.array_equal(alpha, auto_alpha)
        assert np.allclose(diagA, auto_diag, rtol=1e-9, atol=1e-9 * np.abs(auto_diag).max())
    finally:
        N.lib.gh_debug_set_hodlr_strip_cols(old)


# ------------------------------------------------------------------ 6. a size the generic branch cannot hold
def test_grad_n32768_block_by_block():
    n, blk = 32768, 1024
    x, yerr, y = zoo.bench_data(n)
    X = _X(x)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    s = HODLRSolver(kernel, tol=1e-10)
    s.compute(X, yerr)
    ll = s.log_determinant, s.dot_solve(y)
    g, alpha, diagA = s.grad(y, np.ones(kernel.full_size, dtype=np.uint32))
    assert (s.log_determinant, s.dot_solve(y)) == ll
    alpha0 = s.apply_inverse(y)
    assert np.allclose(alpha, alpha0, **MU_TOL)
    g0 = np.zeros(kernel.full_size)
    S = np.zeros(kernel.full_size)
    diag0 = np.empty(n)
    for j0 in range(0, n, blk):                              # no N x N array on the host
        E = np.zeros((n, blk))
        E[j0 + np.arange(blk), np.arange(blk)] = 1.0
        W = s.apply_inverse(E)
        A = np.outer(alpha0, alpha0[j0:j0 + blk]) - W
        dK = kernel.get_gradient(X, X[j0:j0 + blk])
        g0 += 0.5 * np.einsum("ijk,ij", dK, A)
        S += 0.5 * np.einsum("ijk,ij", np.abs(dK), np.abs(A))
        diag0[j0:j0 + blk] = A[j0 + np.arange(blk), np.arange(blk)]
    _check_grad("C4_32768_blocks", g, g0, S)
    assert np.allclose(diagA, diag0, rtol=1e-9, atol=1e-9 * np.abs(diag0).max())


# ------------------------------------------------------------------ 7. C4 at full size; the factor is untouched
def test_c4_full_size_predict_var():
    n, m = 262144, 1024
    x, yerr, y = zoo.bench_data(n)
    X = _X(x)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel, solver=HODLRSolver, tol=1e-10)
    gp.compute(X, yerr)
    ll0 = gp.log_likelihood(y)
    t = _test_points(X, m)
    mu, var = gp.predict(y, t, return_var=True)
    assert mu.shape == (m,) and var.shape == (m,) and np.all(np.isfinite(mu)) and np.all(np.isfinite(var))
    assert gp.log_likelihood(y) == ll0
    cols = np.arange(0, m, m // 16)[:16]
    Kts = kernel.get_value(t[cols], X)
    W = gp.solver.apply_inverse(np.ascontiguousarray(Kts.T))
    assert np.allclose(mu[cols], Kts @ gp.solver.apply_inverse(y), **MU_TOL)
    var0 = kernel.get_value(t[cols], diag=True) - np.sum(Kts.T * W, axis=0)
    _close_or_recorded("C4_262144/var16", var[cols], var0, np.sum(np.abs(Kts.T) * np.abs(W), axis=0), VAR_TOL)


def test_factor_untouched_by_grad_n8192():
    kernel, X, yerr, y, _ = HCONF["C4_8192"][0], _X(HCONF["C4_8192"][1]), HCONF["C4_8192"][2], HCONF["C4_8192"][3], None
    gp = GP(kernel, solver=HODLRSolver, **HCONF["C4_8192"][4])
    gp.compute(X, yerr)
    ll0 = gp.log_likelihood(y)
    a0 = gp.solver.apply_inverse(y)
    g = gp.grad_log_likelihood(y)
    assert np.all(np.isfinite(g)) and gp.log_likelihood(y) == ll0 and np.array_equal(gp.solver.apply_inverse(y), a0)


# ------------------------------------------------------------------ 8. plumbing
def test_predict_with_a_component_kernel_and_sample_conditional():
    x, yerr, y = zoo.bench_data(1200)
    smooth = np.var(y) * kernels.ExpSquaredKernel(1.0)
    kernel = smooth + 0.01 * kernels.Matern32Kernel(0.05)
    gp = GP(kernel, solver=HODLRSolver, tol=1e-10)
    gp.compute(x, yerr)
    t = np.linspace(x.min(), x.max(), 77)
    mu, var = gp.predict(y, t, kernel=smooth, return_var=True)
    X, T = x[:, None], t[:, None]
    Kts = smooth.get_value(T, X)
    W = gp.solver.apply_inverse(np.ascontiguousarray(Kts.T))
    assert np.allclose(mu, Kts @ gp.solver.apply_inverse(y), **MU_TOL)
    assert np.allclose(var, smooth.get_value(T, diag=True) - np.sum(Kts.T * W, axis=0), **VAR_TOL)
    np.random.seed(3)
    draws = gp.sample_conditional(y, t[:20], size=4)
    assert draws.shape == (4, 20) and np.all(np.isfinite(draws))


def test_dense_fallback_delegates_bit_for_bit():
    x, yerr, y = zoo.bench_data(6000, ndim=3)
    kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
    s = HODLRSolver(kernel, tol=1e-12, min_size=100)
    with pytest.warns(RuntimeWarning):
        s.compute(x, yerr)
    assert s.dense_fallback
    d = BasicSolver(kernel)
    d.compute(x, yerr)
    t = _test_points(x, 50)
    for kw in (dict(), dict(return_var=True), dict(return_cov=True)):
        a, b = s.predict(kernel, y, t, **kw), d.predict(kernel, y, t, **kw)
        for u, v in zip(a, b):
            assert (u is None and v is None) or np.array_equal(u, v)
    which = np.ones(kernel.full_size, dtype=np.uint32)
    for u, v in zip(s.grad(y, which), d.grad(y, which)):
        assert np.array_equal(u, v)


def test_pickle_recomputes_and_two_calls_agree_bit_for_bit():
    x, yerr, y = zoo.bench_data(2000)
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0), solver=HODLRSolver, tol=1e-10)
    gp.compute(x, yerr)
    t = np.linspace(0.5, 9.5, 130)
    mu, var = gp.predict(y, t, return_var=True)
    mu2, var2 = gp.predict(y, t, return_var=True)
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
    _, cov = gp.predict(y, t)
    _, cov2 = gp.predict(y, t)
    assert np.array_equal(cov, cov2)
    assert np.array_equal(gp.grad_log_likelihood(y), gp.grad_log_likelihood(y))
    gp3 = pickle.loads(pickle.dumps(gp, -1))
    assert not gp3.solver.computed
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        gp3.solver.predict(gp3.kernel, y, t[:, None])
    mu3, var3 = gp3.predict(y, t, return_var=True)
    assert gp3.solver.computed
    assert np.allclose(mu3, mu, **MU_TOL) and np.allclose(var3, var, **VAR_TOL)
