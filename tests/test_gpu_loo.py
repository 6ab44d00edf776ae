"""Leave-one-out cross-validation on the device (``-m gpu``): gh_chol_loo / gh_chol_loo_objective, BasicSolver.loo and
the GP methods against the CPU reference of tests/loo_ref.py under its one tolerance rule
(``|x - x_ref| <= 32 * 2^-53 * kappa * S``), against N explicit refits, and against themselves (value path / gradient path,
fused / unfused, call / call again).

The sizes are where the 64-wide reduction tile, the 128-wide solver tile and the padding can go wrong."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.optimize

import loo_ref as R
import george_amd
from george_amd import GP, BasicSolver, HODLRSolver, kernels
from george_amd import _native as N
from george_amd.modeling import Model
from george_amd.program import DeviceKernel

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 300, 1000]
QUANTITIES = ("L", "resid", "var", "lpd", "g", "v", "diagB")


@functools.lru_cache(maxsize=None)
def _problem(name, n):
    return R.problem(name, n)


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    return R.reference(*_problem(name, n))


@functools.lru_cache(maxsize=None)
def _brute(name, n):
    return R.brute_force(*_problem(name, n))


def _computed(name, n):
    kernel, x, yerr, r = _problem(name, n)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    return s, r


def _check(ref, label, **values):
    """every given quantity within the rule; prints each error / tolerance ratio first"""
    ratios = {q: ref.ratio(q, v) for q, v in values.items()}
    print("%s: kappa %.3g, error / tolerance %s" % (label, ref.kappa, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    bad = {q: v for q, v in ratios.items() if not v <= 1.0}
    assert not bad, (label, bad)


# ------------------------------------------------------------------ 1. parity with the CPU reference
@pytest.mark.parametrize("name,n", [(k, n) for k in ("expsq", "matern3d", "hyper") for n in SIZES] + [("2d", 129), ("2d", 300)])
def test_every_output_matches_the_reference(name, n):
    s, r = _computed(name, n)
    ref = _reference(name, n)
    P = s._dk.size
    L, resid, var, lpd, g, v, diagB = s.loo(r, np.ones(P, dtype=np.uint32))
    assert g.shape == (P,) and resid.shape == var.shape == lpd.shape == v.shape == diagB.shape == (n,)
    _check(ref, "%s N=%d gradient path" % (name, n), L=L, resid=resid, var=var, lpd=lpd, g=g, v=v, diagB=diagB)
    L0, resid0, var0, lpd0, g0, v0, d0 = s.loo(r)
    assert g0 is None and v0 is None and d0 is None
    _check(ref, "%s N=%d value path" % (name, n), L=L0, resid=resid0, var=var0, lpd=lpd0)
    if n <= 129:
        bL, blpd, bresid, bvar = _brute(name, n)
        for label, (a, b, c, d) in (("gradient path", (L, lpd, resid, var)), ("value path", (L0, lpd0, resid0, var0))):
            ratios = dict(L=R.Ref._ratio(a - bL, ref.tol("L")), lpd=R.Ref._ratio(b - blpd, ref.tol("lpd")),
                          resid=R.Ref._ratio(c - bresid, ref.tol("resid")), var=R.Ref._ratio(d - bvar, ref.tol("var")))
            print("%s N=%d %s against N refits: %s" % (name, n, label, ratios))
            assert max(ratios.values()) <= 1.0, ratios


# ------------------------------------------------------------------ 2. value path and gradient path
def test_value_path_agrees_with_gradient_path_and_forms_one_buffer():
    n = 300
    np_ = -(-n // 128) * 128
    # the O(N) extras, in doubles: the seven leave-one-out vectors; the solve vectors v0 (at least 64 long, it also takes the
    # gradient), v1, v2; the chunk partials of the column reduction (Np / 128 chunks of Np) or, on the gradient path, the
    # reduction's mask (16 bytes) and partial rows (15 tiles of 64 x 64 over 300 points, 11 parameters); 256 scalars
    nt, P, tiles = np_ // 128, 11, 15
    vectors_value = 8 * (7 * np_ + 3 * np_ + nt * np_ + 256)
    vectors_grad = 8 * (7 * np_ + 3 * np_ + max(nt * np_, 2 + tiles * P) + 256)
    BasicSolver.release_pool()       # a handle of its own: nothing grown by an earlier test
    s, r = _computed("hyper", n)
    ref = _reference("hyper", n)
    h = s._handle
    base = int(N.lib.gh_chol_device_bytes(h))
    assert base >= 8 * np_ * np_
    L0, resid0, var0, lpd0, _, _, _ = s.loo(r)
    one = int(N.lib.gh_chol_device_bytes(h)) - base
    print("value path: %d bytes above the factor (one N x N buffer: %d)" % (one, 8 * np_ * np_))
    assert one <= 8 * np_ * np_ + vectors_value
    L1, resid1, var1, lpd1, _, _, _ = s.loo(r, np.ones(s._dk.size, dtype=np.uint32))
    two = int(N.lib.gh_chol_device_bytes(h)) - base
    print("gradient path: %d bytes above the factor" % two)
    assert two <= 2 * 8 * np_ * np_ + vectors_grad
    for q, a, b in (("L", L0, L1), ("resid", resid0, resid1), ("var", var0, var1), ("lpd", lpd0, lpd1)):
        ratio = R.Ref._ratio(np.asarray(a) - np.asarray(b), ref.tol(q))
        print("value path against gradient path, %s: error / tolerance %.3g" % (q, ratio))
        assert ratio <= 1.0


# ------------------------------------------------------------------ 3. fused against unfused
@pytest.mark.parametrize("n", [300, 1024])
def test_fused_objective_is_compute_then_loo_bit_for_bit(n):
    kernel, x, yerr, r = _problem("hyper", n)
    which = np.ones(11, dtype=np.uint32)
    a = BasicSolver(kernel)
    a.compute(x, yerr)
    g_before = a.grad(r, which)
    L, resid, var, lpd, g, v, diagB = a.loo(r, which)
    g_after = a.grad(r, which)
    for p, q in zip(g_before, g_after):                 # the work buffers are shared safely
        assert np.array_equal(p, q)
    b = BasicSolver(kernel)
    logdet, L2, resid2, var2, g2, v2, diagB2 = b.loo_objective(x, yerr, r, which)
    assert logdet == a.log_determinant and L2 == L
    for p, q in ((resid, resid2), (var, var2), (g, g2), (v, v2), (diagB, diagB2)):
        assert np.array_equal(p, q)
    # values only
    logdet3, L3, resid3, var3, g3, v3, d3 = BasicSolver(kernel).loo_objective(x, yerr, r, want_grad=False)
    L0, resid0, var0, _, _, _, _ = a.loo(r)
    assert g3 is None and v3 is None and d3 is None
    assert logdet3 == logdet and L3 == L0 and np.array_equal(resid3, resid0) and np.array_equal(var3, var0)
    # the handle is left computed
    assert b.computed and int(N.lib.gh_chol_size(b._handle)) == n
    xs = np.linspace(x.min(), x.max(), 37)[:, None]
    for p, q in zip(a.predict(kernel, r, xs, return_var=True), b.predict(kernel, r, xs, return_var=True)):
        assert (p is None and q is None) or np.array_equal(p, q)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("name,n", [("matern3d", 129), ("hyper", 300)])
def test_two_calls_give_the_same_bits(name, n):
    s, r = _computed(name, n)
    which = np.ones(s._dk.size, dtype=np.uint32)
    for args in ((r, which), (r,)):
        first, second = s.loo(*args), s.loo(*args)
        for p, q in zip(first, second):
            assert (p is None and q is None) or np.array_equal(p, q)


# ------------------------------------------------------------------ 5. the parameter mask
@pytest.mark.parametrize("name,P", [("2d", 5), ("p13", 13), ("p17", 17)])
def test_masked_entries_are_exactly_zero(name, P):
    n = 129
    s, r = _computed(name, n)
    ref = _reference(name, n)
    assert s._dk.size == P
    which = (np.arange(P) % 2).astype(np.uint32)
    L, resid, var, lpd, g, v, diagB = s.loo(r, which)
    assert np.all(g[which == 0] == 0.0) and not np.any(np.signbit(g[which == 0]))
    ratio = R.Ref._ratio((g - ref.g)[which == 1], ref.tol("g")[which == 1])
    print("%s: unmasked gradient entries, error / tolerance %.3g" % (name, ratio))
    assert ratio <= 1.0
    _check(ref, "%s masked" % name, L=L, v=v, diagB=diagB)
    L, resid, var, lpd, g, v, diagB = s.loo(r, np.zeros(P, dtype=np.uint32))
    assert np.all(g == 0.0)
    _check(ref, "%s nothing selected" % name, L=L, resid=resid, var=var, lpd=lpd, v=v, diagB=diagB)


# ------------------------------------------------------------------ 6. GP level
class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


class NoLooSolver(BasicSolver):
    """the generic NumPy branch of GP.loo_*, on the device solver's apply_inverse / get_inverse"""
    loo = None
    loo_objective = None


def _gp_case(solver, n=300, seed=4):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.12 + 0.05 * rng.rand(n)
    y = 0.3 * x - 1.0 + np.sin(2.0 * x) + 0.2 * rng.randn(n)
    gp = GP(1.3 * kernels.ExpSquaredKernel(0.6), mean=LinearMean(m=0.25, b=-0.8), white_noise=np.log(0.02),
            fit_white_noise=True, solver=solver)
    gp.compute(x, yerr)
    return gp, x, yerr, y


def test_gp_methods_match_the_generic_branch_and_the_reference():
    gp, x, yerr, y = _gp_case(BasicSolver)
    gen, _, _, _ = _gp_case(NoLooSolver)
    assert callable(gp.solver.loo) and gen.solver.loo is None
    sigma = np.sqrt(yerr ** 2 + 0.02)
    r = y - (0.25 * x - 0.8)
    ref = R.reference(gp.kernel, x[:, None], sigma, r)
    # the gradient's reference and tolerance, assembled as GP does: mean | white noise | kernel
    mg = np.stack([x, np.ones_like(x)])
    g_ref = np.concatenate([mg @ ref.v, [0.02 * np.sum(ref.diagB)], ref.g])
    g_tol = np.concatenate([np.abs(mg).sum(axis=1) * ref.tol("v"), [0.02 * len(x) * ref.tol("diagB")], ref.tol("g")])
    for label, m in (("BasicSolver.loo", gp), ("generic branch", gen)):
        mu, var = m.loo_predict(y)
        L = m.loo_log_likelihood(y)
        lpd = m.loo_log_likelihood(y, pointwise=True)
        g = m.grad_loo_log_likelihood(y)
        _check(ref, label, L=L, resid=y - mu, var=var, lpd=lpd)
        ratio = R.Ref._ratio(g - g_ref, g_tol)
        print("%s: gradient (mean | white noise | kernel) error / tolerance %.3g" % (label, ratio))
        assert g.shape == (5,) and ratio <= 1.0
        assert np.array_equal(m.loo_predict(y, return_var=False), mu)


def test_hodlr_through_the_generic_branch_matches_the_dense_solver():
    n = 500
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.12 + 0.05 * rng.rand(n)
    y = np.sin(2.0 * x) + 0.2 * rng.randn(n)
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6)
    dense = GP(kernel)
    dense.compute(x, yerr)
    hod = GP(kernel, solver=HODLRSolver, tol=1e-12)
    hod.compute(x, yerr)
    assert not callable(getattr(hod.solver, "loo", None)) and not callable(getattr(hod.solver, "loo_objective", None)) and not hod.solver.dense_fallback
    pairs = {"mu": (hod.loo_predict(y)[0], dense.loo_predict(y)[0]), "var": (hod.loo_predict(y)[1], dense.loo_predict(y)[1]),
             "L": (hod.loo_log_likelihood(y), dense.loo_log_likelihood(y)),
             "grad": (hod.grad_loo_log_likelihood(y), dense.grad_loo_log_likelihood(y))}
    for what, (a, b) in pairs.items():
        err = np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))
        print("HODLR (tol 1e-12) against dense, %s: relative difference %.3g" % (what, err))
        assert err <= 1e-8, what


def test_append_then_loo_predict_is_compute_on_all_the_data():
    gp, x, yerr, y = _gp_case(BasicSolver, n=300)
    part = GP(1.3 * kernels.ExpSquaredKernel(0.6), mean=LinearMean(m=0.25, b=-0.8), white_noise=np.log(0.02),
              fit_white_noise=True)
    part.compute(x[:200], yerr[:200])
    part.append(x[200:], yerr[200:])
    assert len(part._x) == 300
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + 0.02), y - (0.25 * x - 0.8))
    for label, m in (("append", part), ("compute", gp)):
        mu, var = m.loo_predict(y)
        _check(ref, label, resid=y - mu, var=var)


# ------------------------------------------------------------------ 7. the optimiser
def test_lbfgs_minimises_the_leave_one_out_objective():
    n = 256
    rng = np.random.RandomState(21)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.12 + 0.05 * rng.rand(n)
    true = 1.3 * kernels.ExpSquaredKernel(0.6)
    Kt = true.get_value(x[:, None]) + np.diag(yerr ** 2)
    y = np.linalg.cholesky(Kt) @ rng.randn(n)
    gp = GP(1.3 * kernels.ExpSquaredKernel(0.6))
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector() + np.array([0.7, -0.5])
    f = lambda p: gp.loo_nll_and_grad(p, y)[0]           # noqa: E731
    fg = lambda p: gp.loo_nll_and_grad(p, y)[1]          # noqa: E731
    g0 = fg(p0)
    rel = scipy.optimize.check_grad(f, fg, p0, epsilon=1e-6) / np.linalg.norm(g0)
    print("check_grad at the start point: %.3g relative to |grad| = %.3g" % (rel, np.linalg.norm(g0)))
    assert rel < 1e-5
    f0 = f(p0)
    res = scipy.optimize.minimize(gp.loo_nll_and_grad, p0, jac=True, args=(y,), method="L-BFGS-B",
                                  options=dict(ftol=1e-14, gtol=1e-9, maxiter=200))
    gp.set_parameter_vector(res.x)
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + george_amd.gp.TINY), y)
    print("objective %.12g -> %.12g in %d iterations, |grad| / S_p = %s" % (f0, res.fun, res.nit, np.abs(res.jac) / ref.S))
    assert res.fun < f0
    assert np.all(np.abs(res.jac) <= 1e-4 * ref.S)


# ------------------------------------------------------------------ 8. not computed, not positive definite
def test_errors():
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6)
    singular = kernels.CosineKernel(log_period=0.0)      # a rank-2 kernel: singular without noise
    dk, dks = DeviceKernel(kernel), DeviceKernel(singular)
    o = N.gh_chol_opts()
    o.device, o.lookahead = 0, 1
    h = N._vp()
    N.check(N.lib.gh_chol_create(ctypes.byref(o), ctypes.byref(h)))
    n = 200
    x = np.linspace(0.0, 3.0, n)[:, None]
    r, resid, var = np.sin(x[:, 0]), np.empty(n), np.empty(n)
    g, v, diagB = np.zeros(2), np.empty(n), np.empty(n)
    total, logdet = ctypes.c_double(0.0), ctypes.c_double(0.0)
    # (every array whose address goes to the library has a name that outlives the call: N.ptr returns a plain integer)
    no_noise, some_noise, one_selected = np.zeros(n), np.full(n, 0.2), np.ones(1, dtype=np.uint32)

    def values_only(handle_kernel):
        return N.lib.gh_chol_loo(h, handle_kernel, None, N.ptr(r), ctypes.byref(total), N.ptr(resid), N.ptr(var), None, None, None,
                                 None)
    try:
        assert values_only(dk.handle) == N.GH_ERR_NOT_COMPUTED                       # a fresh handle
        rc = N.lib.gh_chol_loo_objective(h, dks.handle, N.ptr(x), n, 1, N.ptr(no_noise), N.ptr(r), N.ptr(one_selected),
                                         ctypes.byref(logdet), ctypes.byref(total), N.ptr(resid), N.ptr(var), N.ptr(g), N.ptr(v),
                                         N.ptr(diagB))
        assert rc == N.GH_ERR_NOT_PD
        assert 0 < int(N.lib.gh_chol_info(h)) <= n
        assert values_only(dks.handle) == N.GH_ERR_NOT_COMPUTED
        # a gradient without a mask, and a kernel of another dimension
        N.check(N.lib.gh_chol_compute(h, dk.handle, N.ptr(x), n, 1, N.ptr(some_noise), ctypes.byref(logdet)))
        rc = N.lib.gh_chol_loo(h, dk.handle, None, N.ptr(r), ctypes.byref(total), N.ptr(resid), N.ptr(var), None, N.ptr(g), None, None)
        assert rc == N.GH_ERR_BAD_ARG
        dk3 = DeviceKernel(kernels.ExpSquaredKernel([1.0, 2.0, 3.0], ndim=3))
        assert values_only(dk3.handle) == N.GH_ERR_DIM
        assert values_only(dk.handle) == N.GH_OK
    finally:
        N.lib.gh_chol_destroy(h)
    with pytest.raises(np.linalg.LinAlgError):
        BasicSolver(singular).loo_objective(x, np.zeros(n), r)
    gp = GP(singular, white_noise=-1000.0)
    gp.compute(x[:5], 1.0)
    gp._x, gp._yerr2 = np.ascontiguousarray(x), np.zeros(n)
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector() + 0.1, r)
    assert val == np.inf and np.all(grad == 0.0)
