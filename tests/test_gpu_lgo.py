"""Leave-group-out cross-validation on the device (``-m gpu``): gh_chol_lgo, BasicSolver.lgo and the GP methods against the
CPU reference of tests/lgo_ref.py under its one tolerance rule (``|x - x_ref| <= 32 * 2^-53 * kappa * S``), against G
explicit refits, against leave-one-out, and against themselves (value path / gradient path, call / call again).

The sizes are where the 128-wide slot and solver tile and the padding can go wrong; the groupings fill a slot with many
groups, with one, across the tile edge and out of order."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.optimize

import lgo_ref as R
from george_amd import GP, BasicSolver, HODLRSolver, kernels
from george_amd import _native as N
from george_amd.modeling import Model
from george_amd.program import DeviceKernel

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 127, 128, 129, 300, 1000]


@functools.lru_cache(maxsize=None)
def _problem(name, n):
    return R.problem(name, n)


@functools.lru_cache(maxsize=None)
def _groups(grouping, n):
    labels = R.grouping(grouping, n)
    return None if labels is None else R.order_start(labels)


@functools.lru_cache(maxsize=None)
def _reference(name, n, grouping):
    return R.reference(*(_problem(name, n) + _groups(grouping, n)))


@functools.lru_cache(maxsize=None)
def _brute(name, n, grouping):
    return R.brute_force(*(_problem(name, n) + _groups(grouping, n)))


@functools.lru_cache(maxsize=None)
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


def _named(out):
    L, resid, var, lpd, cov, g, v, diagB = out
    return dict(L=L, resid=resid, var=var, lpd=lpd, cov=cov, g=g, v=v, diagB=diagB)


# ------------------------------------------------------------------ 1. parity with the CPU reference
CASES = [(k, n, grouping) for k in ("expsq", "matern3d", "hyper") for n in SIZES for grouping in R.GROUPINGS
         if grouping != "one" or n <= 128]


@pytest.mark.parametrize("name,n,grouping", CASES)
def test_every_output_matches_the_reference(name, n, grouping):
    s, r = _computed(name, n)
    P = s._dk.size
    order, start = _groups(grouping, n)
    G = len(start) - 1
    ref = _reference(name, n, grouping)
    full = _named(s.lgo(r, order, start, np.ones(P, dtype=np.uint32), want_cov=True))
    assert full["g"].shape == (P,) and full["lpd"].shape == (G,) and len(full["cov"]) == G
    assert full["resid"].shape == full["var"].shape == full["v"].shape == full["diagB"].shape == (n,)
    assert [c.shape for c in full["cov"]] == [(m, m) for m in np.diff(start)]
    _check(ref, "%s N=%d %s gradient path" % (name, n, grouping), **full)
    value = _named(s.lgo(r, order, start, want_cov=True))
    assert value["g"] is None and value["v"] is None and value["diagB"] is None
    _check(ref, "%s N=%d %s value path" % (name, n, grouping), **{q: value[q] for q in ("L", "resid", "var", "lpd", "cov")})
    assert s.lgo(r, order, start)[4] is None
    if n <= 300:
        bL, blpd, bresid, bvar, bcov = _brute(name, n, grouping)
        for label, out in (("gradient path", full), ("value path", value)):
            ratios = dict(L=R.Ref._ratio(out["L"] - bL, ref.tol("L")), lpd=R.Ref._ratio(out["lpd"] - blpd, ref.tol("lpd")),
                          resid=R.Ref._ratio(out["resid"] - bresid, ref.tol("resid")),
                          var=R.Ref._ratio(out["var"] - bvar, ref.tol("var")),
                          cov=max(R.Ref._ratio(a - b, ref.tol("cov")) for a, b in zip(out["cov"], bcov)))
            print("%s N=%d %s %s against G refits: %s" % (name, n, grouping, label, ratios))
            assert max(ratios.values()) <= 1.0, (grouping, label, ratios)


def test_the_cases_are_the_issues():
    assert len(CASES) == 3 * (7 * 7 + 4) and {c[2] for c in CASES if c[1] > 128} == set(R.GROUPINGS) - {"one"}


# ------------------------------------------------------------------ 2. one-point groups are leave-one-out
@pytest.mark.parametrize("name,n", [("expsq", 128), ("matern3d", 129), ("hyper", 300)])
def test_singletons_agree_with_leave_one_out_on_the_same_handle(name, n):
    s, r = _computed(name, n)
    order, start = _groups("singletons", n)
    ref = _reference(name, n, "singletons")
    which = np.ones(s._dk.size, dtype=np.uint32)
    for label, wh in (("gradient path", which), ("value path", None)):
        L, resid, var, lpd, g, v, diagB = s.loo(r, wh)
        out = _named(s.lgo(r, order, start, wh))
        pairs = dict(L=(out["L"], L), resid=(out["resid"], resid), var=(out["var"], var), lpd=(out["lpd"], lpd))
        if wh is not None:
            pairs.update(g=(out["g"], g), v=(out["v"], v), diagB=(out["diagB"], diagB))
        ratios = {q: R.Ref._ratio(np.asarray(a) - np.asarray(b), ref.tol(q)) for q, (a, b) in pairs.items()}
        print("%s N=%d singletons against loo, %s: error / tolerance %s" % (name, n, label, ratios))
        assert max(ratios.values()) <= 1.0, (label, ratios)


# ------------------------------------------------------------------ 3. value path and gradient path
def test_value_path_agrees_with_gradient_path_and_forms_one_buffer():
    n, grouping = 300, "blk7"
    np_ = -(-n // 128) * 128
    order, start = _groups(grouping, n)
    G = len(start) - 1
    nslots = len(R.slots(start))
    assert nslots <= 2 * (np_ // 128) + 1
    # the slot buffers, in bytes: the slot matrices and their inverses, the Gram step's partial sums (at most 16 row chunks)
    # or the gradient path's W, and the tables (two ints per slot position and per slot, two offsets per group, the failure
    # word); the O(N) extras of the leave-one-out test: seven N-vectors, the solve vectors, the reduction's scratch, 256 scalars
    tile = 8 * 128 * 128
    slot_value = nslots * tile * (2 + 16) + 8 * nslots * 129 + 16 * (G + 1) + 16
    slot_grad = nslots * tile * 3 + 8 * nslots * 129 + 16 * (G + 1) + 16
    nt, P, tiles = np_ // 128, 11, 15
    vectors = 8 * (7 * np_ + 3 * np_ + max(nt * np_, 2 + tiles * P) + 256)
    BasicSolver.release_pool()       # a handle of its own: nothing grown by an earlier test
    kernel, x, yerr, r = _problem("hyper", n)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    ref = _reference("hyper", n, grouping)
    which = np.ones(P, dtype=np.uint32)
    h = s._handle
    base = int(N.lib.gh_chol_device_bytes(h))
    assert base >= 8 * np_ * np_
    value = _named(s.lgo(r, order, start))
    one = int(N.lib.gh_chol_device_bytes(h)) - base
    print("value path: %d bytes above the factor (one N x N buffer: %d, slot buffers at most %d)" % (one, 8 * np_ * np_, slot_value))
    assert one <= 8 * np_ * np_ + slot_value + vectors
    full = _named(s.lgo(r, order, start, which))
    two = int(N.lib.gh_chol_device_bytes(h)) - base
    print("gradient path: %d bytes above the factor" % two)
    assert two <= 2 * 8 * np_ * np_ + max(slot_value, slot_grad) + vectors
    for q in ("L", "resid", "var", "lpd"):
        ratio = R.Ref._ratio(np.asarray(value[q]) - np.asarray(full[q]), ref.tol(q))
        print("value path against gradient path, %s: error / tolerance %.3g" % (q, ratio))
        assert ratio <= 1.0
    # the work buffers are shared safely: grad and predict give the same bits before and after an lgo call of either path
    xs = np.linspace(x.min(), x.max(), 37)[:, None]
    g_before, p_before = s.grad(r, which), s.predict(kernel, r, xs, return_var=True)
    s.lgo(r, order, start, which, want_cov=True)
    s.lgo(r, order, start)
    for p, q in zip(g_before, s.grad(r, which)):
        assert np.array_equal(p, q)
    for p, q in zip(p_before, s.predict(kernel, r, xs, return_var=True)):
        assert (p is None and q is None) or np.array_equal(p, q)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.parametrize("grouping", ["ragged", "random"])
@pytest.mark.parametrize("name,n", [("matern3d", 129), ("hyper", 300)])
def test_two_calls_give_the_same_bits(name, n, grouping):
    s, r = _computed(name, n)
    order, start = _groups(grouping, n)
    which = np.ones(s._dk.size, dtype=np.uint32)
    for wh in (which, None):
        first, second = s.lgo(r, order, start, wh, want_cov=True), s.lgo(r, order, start, wh, want_cov=True)
        for p, q in zip(first, second):
            if isinstance(p, list):
                assert all(np.array_equal(a, b) for a, b in zip(p, q))
            else:
                assert (p is None and q is None) or np.array_equal(p, q)


# ------------------------------------------------------------------ 5. the parameter mask
@pytest.mark.parametrize("name,P", [("2d", 5), ("p13", 13)])
def test_masked_entries_are_exactly_zero(name, P):
    n, grouping = 129, "ragged"
    s, r = _computed(name, n)
    order, start = _groups(grouping, n)
    ref = _reference(name, n, grouping)
    assert s._dk.size == P
    which = (np.arange(P) % 2).astype(np.uint32)
    out = _named(s.lgo(r, order, start, which))
    g = out["g"]
    assert np.all(g[which == 0] == 0.0) and not np.any(np.signbit(g[which == 0]))
    ratio = R.Ref._ratio((g - ref.g)[which == 1], ref.tol("g")[which == 1])
    print("%s: unmasked gradient entries, error / tolerance %.3g" % (name, ratio))
    assert ratio <= 1.0
    _check(ref, "%s masked" % name, L=out["L"], v=out["v"], diagB=out["diagB"])
    out = _named(s.lgo(r, order, start, np.zeros(P, dtype=np.uint32)))
    assert np.all(out["g"] == 0.0)
    _check(ref, "%s nothing selected" % name, **{q: out[q] for q in ("L", "resid", "var", "lpd", "v", "diagB")})


# ------------------------------------------------------------------ 6. GP level
class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


class NoLgoSolver(BasicSolver):
    """the generic NumPy branch of GP.lgo_*, on the device solver's apply_inverse / get_inverse"""
    lgo = None


def _gp_case(solver, n=300, seed=4):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.12 + 0.05 * rng.rand(n)
    y = 0.3 * x - 1.0 + np.sin(2.0 * x) + 0.2 * rng.randn(n)
    gp = GP(1.3 * kernels.ExpSquaredKernel(0.6), mean=LinearMean(m=0.25, b=-0.8), white_noise=np.log(0.02),
            fit_white_noise=True, solver=solver)
    gp.compute(x, yerr)
    return gp, x, yerr, y


def _gp_labels(n):
    return np.random.RandomState(31).randint(-4, 9, n) * 5


@pytest.mark.parametrize("form", ["windows", "labels"])
def test_gp_methods_match_the_generic_branch_and_the_reference(form):
    gp, x, yerr, y = _gp_case(BasicSolver)
    gen, _, _, _ = _gp_case(NoLgoSolver)
    assert callable(gp.solver.lgo) and gen.solver.lgo is None
    n = len(x)
    groups = 16 if form == "windows" else _gp_labels(n)
    order, start = R.order_start(np.arange(n) // 16 if form == "windows" else groups)
    sigma = np.sqrt(yerr ** 2 + 0.02)
    r = y - (0.25 * x - 0.8)
    ref = R.reference(gp.kernel, x[:, None], sigma, r, order, start)
    # the gradient's reference and tolerance, assembled as GP does: mean | white noise | kernel
    mg = np.stack([x, np.ones_like(x)])
    g_ref = np.concatenate([mg @ ref.v, [0.02 * np.sum(ref.diagB)], ref.g])
    g_tol = np.concatenate([np.abs(mg).sum(axis=1) * ref.tol("v"), [0.02 * n * ref.tol("diagB")], ref.tol("g")])
    for label, m in (("BasicSolver.lgo", gp), ("generic branch", gen)):
        mu, var, cov = m.lgo_predict(y, groups, return_cov=True)
        L = m.lgo_log_likelihood(y, groups)
        lpd = m.lgo_log_likelihood(y, groups, pointwise=True)
        g = m.grad_lgo_log_likelihood(y, groups)
        _check(ref, "%s, %s" % (label, form), L=L, resid=y - mu, var=var, lpd=lpd, cov=cov)
        ratio = R.Ref._ratio(g - g_ref, g_tol)
        print("%s: gradient (mean | white noise | kernel) error / tolerance %.3g" % (label, ratio))
        assert g.shape == (5,) and ratio <= 1.0
        assert np.array_equal(m.lgo_predict(y, groups, return_var=False), mu)
        val, grad = m.lgo_nll_and_grad(m.get_parameter_vector(), y, groups)
        assert ref.ratio("L", -val) <= 1.0 and np.array_equal(grad, -g)       # (the value comes from the gradient path here)


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
    assert not callable(getattr(hod.solver, "lgo", None)) and callable(dense.solver.lgo) and not hod.solver.dense_fallback
    pairs = {"mu": (hod.lgo_predict(y, 16)[0], dense.lgo_predict(y, 16)[0]), "var": (hod.lgo_predict(y, 16)[1], dense.lgo_predict(y, 16)[1]),
             "L": (hod.lgo_log_likelihood(y, 16), dense.lgo_log_likelihood(y, 16)),
             "grad": (hod.grad_lgo_log_likelihood(y, 16), dense.grad_lgo_log_likelihood(y, 16))}
    for what, (a, b) in pairs.items():
        err = np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b))
        print("HODLR (tol 1e-12) against dense, %s: relative difference %.3g" % (what, err))
        assert err <= 1e-8, what


def test_append_then_lgo_predict_is_compute_on_all_the_data():
    gp, x, yerr, y = _gp_case(BasicSolver, n=300)
    part = GP(1.3 * kernels.ExpSquaredKernel(0.6), mean=LinearMean(m=0.25, b=-0.8), white_noise=np.log(0.02),
              fit_white_noise=True)
    part.compute(x[:200], yerr[:200])
    part.append(x[200:], yerr[200:])
    assert len(part._x) == 300
    order, start = R.order_start(np.arange(300) // 16)
    ref = R.reference(gp.kernel, x[:, None], np.sqrt(yerr ** 2 + 0.02), y - (0.25 * x - 0.8), order, start)
    for label, m in (("append", part), ("compute", gp)):
        mu, var = m.lgo_predict(y, 16)
        _check(ref, label, resid=y - mu, var=var)


# ------------------------------------------------------------------ 7. the optimiser
def test_lbfgs_minimises_the_leave_group_out_objective():
    n = 256
    rng = np.random.RandomState(21)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.12 + 0.05 * rng.rand(n)
    true = 1.3 * kernels.ExpSquaredKernel(0.6)
    Kt = true.get_value(x[:, None]) + np.diag(yerr ** 2)
    y = np.linalg.cholesky(Kt) @ rng.randn(n)
    gp = GP(1.3 * kernels.ExpSquaredKernel(0.6))
    gp.compute(x, yerr)
    # The start: amplitude too small, length scale too long.  check_grad's forward difference is off by about h |f''| / 2 plus
    # the round-off of f over h, whatever the size of the gradient, so "relative to |grad|" tests the gradient only where it is
    # not nearly zero: at the leave-one-out test's start (+0.7, -0.5) this objective is almost stationary (|grad| = 0.58 where
    # the other starts have 17 .. 41), and the same 2.7e-5 of truncation that every solver branch shows there reads as 5e-5.
    p0 = gp.get_parameter_vector() + np.array([-0.7, 0.5])
    f = lambda p: gp.lgo_nll_and_grad(p, y, 16)[0]           # noqa: E731
    fg = lambda p: gp.lgo_nll_and_grad(p, y, 16)[1]          # noqa: E731
    g0 = fg(p0)
    rel = scipy.optimize.check_grad(f, fg, p0, epsilon=1e-6) / np.linalg.norm(g0)
    print("check_grad at the start point: %.3g relative to |grad| = %.3g" % (rel, np.linalg.norm(g0)))
    assert rel < 1e-5
    f0 = f(p0)
    res = scipy.optimize.minimize(gp.lgo_nll_and_grad, p0, jac=True, args=(y, 16), method="L-BFGS-B",
                                  options=dict(ftol=1e-14, gtol=1e-9, maxiter=200))
    print("objective %.12g -> %.12g in %d iterations" % (f0, res.fun, res.nit))
    assert res.fun < f0


# ------------------------------------------------------------------ 8. errors through the C ABI
def test_errors():
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6)
    dk = DeviceKernel(kernel)
    o = N.gh_chol_opts()
    o.device, o.lookahead = 0, 1
    h = N._vp()
    N.check(N.lib.gh_chol_create(ctypes.byref(o), ctypes.byref(h)))
    n = 200
    x = np.linspace(0.0, 3.0, n)[:, None]
    r, resid, var = np.sin(x[:, 0]), np.empty(n), np.empty(n)
    g = np.zeros(2)
    total, logdet = ctypes.c_double(0.0), ctypes.c_double(0.0)
    # (every array whose address goes to the library has a name that outlives the call: N.ptr returns a plain integer)
    some_noise, one_selected = np.full(n, 0.2), np.ones(2, dtype=np.uint32)
    order = np.arange(n, dtype=np.int64)
    start = np.arange(0, n + 1, 8, dtype=np.int64)
    twice = order.copy()
    twice[5] = 4
    beyond = order.copy()
    beyond[0] = n
    falls = start.copy()
    falls[3], falls[4] = start[4], start[3]
    short = start.copy()
    short[-1] = n - 1
    empty = start.copy()
    empty[7] = empty[6]
    big = np.array([0, 129, n], dtype=np.int64)

    def call(handle_kernel, order_, start_, which=None, grad=None):
        return N.lib.gh_chol_lgo(h, handle_kernel, N.ptr(which), N.ptr(r), N.ptr(order_), N.ptr(start_), len(start_) - 1,
                                 ctypes.byref(total), N.ptr(resid), N.ptr(var), None, None, N.ptr(grad), None, None)
    try:
        assert call(dk.handle, order, start) == N.GH_ERR_NOT_COMPUTED               # a fresh handle
        N.check(N.lib.gh_chol_compute(h, dk.handle, N.ptr(x), n, 1, N.ptr(some_noise), ctypes.byref(logdet)))
        assert call(dk.handle, order, start, None, g) == N.GH_ERR_BAD_ARG           # a gradient without a mask
        for bad_order in (twice, beyond):
            assert call(dk.handle, bad_order, start) == N.GH_ERR_BAD_ARG
            assert b"permutation" in N.lib.gh_last_error()
        for bad_start in (falls, short, empty, big):
            assert call(dk.handle, order, bad_start) == N.GH_ERR_BAD_ARG
        assert call(dk.handle, order, empty) == N.GH_ERR_BAD_ARG and b"empty" in N.lib.gh_last_error()
        assert call(dk.handle, order, big) == N.GH_ERR_BAD_ARG and b"128" in N.lib.gh_last_error()
        dk3 = DeviceKernel(kernels.ExpSquaredKernel([1.0, 2.0, 3.0], ndim=3))
        assert call(dk3.handle, order, start) == N.GH_ERR_DIM
        assert call(dk.handle, order, start) == N.GH_OK
        assert call(dk.handle, order, start, one_selected, g) == N.GH_OK
    finally:
        N.lib.gh_chol_destroy(h)
    s, rr = _computed("expsq", 300)
    with pytest.raises(ValueError):
        s.lgo(rr, np.arange(300), np.array([0, 129, 300]))
