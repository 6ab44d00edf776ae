"""The host side of tests/test_gpu_inducing_loo.py: the two NumPy routes of the DTC / FITC leave-one-out
(tests/inducing_loo_ref.py) against each other, the low-rank route against central differences of its own ``L`` and, with ``u = x``
and no jitter, against the dense leave-one-out by LAPACK (tests/loo_ref.py); the deliberately wrong gradients against the bound
the device tests use; the problems of the device tests against the cap on the gap; ``GP`` routing to ``loo_lowrank``; and the
inputs that are refused.  No device is touched.

Central differences.  ``L`` is smooth in the log-parameters, the residuals and the diagonal of ``C``; with the step ``h`` the
central difference has a truncation error of ``h^2 / 6 |L'''|`` and a rounding error of about ``eps |L| / h``.  At ``h = 1e-5``
(relative to the variable's scale) and ``|L|`` a few hundred that is 1e-10 and 1e-8 of a derivative of order one: the bound is
``FD_BOUND = 1e-6`` of the largest entry of each of ``kgrad``, ``v`` and ``diagB``, a hundred times that, while every structural
error -- a missing half of ``Z``, the ``S`` term of ``d2``, a weight 1/2 -- is of order one.

``u = x`` without jitter.  ``C`` is then ``K + diag(yerr^2)`` up to the rounding of ``K_uu^-1 K_uf``, which is ``eps cond(K_uu)``
per entry: the bound against the dense reference is ``100 eps cond(K_uu)``, printed with the error.

Observed on the CPU (every test prints its figures): the two routes differ by at most 3.6e-13 (``v``, the composite kernel) on
the problems below; central differences agree to 2e-9 (``kgrad``), 2e-10 (``v``) and 3e-9 (``diagB``).
"""
import copy
import ctypes

import numpy as np
import pytest

from george_amd import GP, InducingSolver, kernels
from george_amd import _native as N
from oracle import solver_np

import inducing_cases as IC
import inducing_loo_ref as IL
import loo_ref
from test_fisher_host import LinearMean, MinimalSolver, NoiseRamp, _host_gradient

FD_BOUND = 1e-6
H = 1e-5

# (problem, N, m, inducing, relative jitter) of every device test that takes a bound
DEVICE_PROBLEMS = ([("m32_3d", 300, 65, "maxmin", 1e-10), ("m32_3d", 300, 65, "random", 1e-10), ("m32_1d", 300, 65, "maxmin", 1e-10),
                    ("comp_3d", 300, 65, "maxmin", 1e-10), ("expsq_1d", 300, 65, "maxmin", 1e-8), ("m32_3d", 300, 300, "all", 0.0),
                    ("m32_3d", 257, 65, "maxmin", 1e-10), ("m32_3d", 256, 65, "maxmin", 1e-10), ("m32_3d", 1, 1, "maxmin", 1e-10),
                    ("m32_3d", 4097, 16, "maxmin", 1e-10), ("m32_3d", 20011, 128, "maxmin", 1e-10)] +
                   [("m32_3d", 300, m, "maxmin", 1e-10) for m in (1, 64, 128, 129)])


def _case(name, n, m, inducing="maxmin"):
    """(kernel, x, yerr, r, u) of a named problem of tests/inducing_cases.py; ``inducing``: max-min points of the data, uniform
    points that are no data points ("random"), or the data themselves ("all")"""
    kernel, x, yerr, r, _ = IC._problem(name, n)
    if inducing == "all":
        return kernel, x, yerr, r, x.copy()
    if inducing == "random":
        return kernel, x, yerr, r, np.random.RandomState(m).uniform(0, 10 if x.shape[1] == 1 else 2, (m, x.shape[1]))
    return kernel, x, yerr, r, np.ascontiguousarray(x[IC.inducing_points(x, m)])


# ------------------------------------------------------------------ the two routes, and the cap
@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("name,n,m,inducing,rel_jitter", DEVICE_PROBLEMS)
def test_the_two_cpu_routes_stay_inside_the_cap(name, n, m, inducing, rel_jitter, method):
    """every problem of tests/test_gpu_inducing_loo.py: ``tolerances`` asserts the cap on the gap"""
    kernel, x, yerr, r, u = _case(name, n, m, inducing)
    _, tol = IL.tolerances(kernel, x, yerr, u, rel_jitter, method, r, label=name)
    assert sorted(tol) == sorted(IL.QUANTITIES + ("c",)) and all(4000 * IL.EPS <= t <= 1000 * IL.GAP_CAP for t in tol.values()), tol


@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("name", IC.PCASE_NAMES)
def test_the_parameter_count_cases_stay_inside_the_cap(name, method):
    kernel, x, yerr, r, _, u = IC.pcase(name)
    IL.tolerances(kernel, x, yerr, u, 1e-10, method, r, label="P=%s" % name)


def test_the_block_route_is_the_stacked_route():
    kernel, x, yerr, r, u = _case("m32_3d", 600, 65)
    a = IL.reference(kernel, x, yerr, u, 1e-10, "fitc", r)
    b = IL.reference(kernel, x, yerr, u, 1e-10, "fitc", r, route="blocks")
    err = IL._over(a.kgrad - b.kgrad, a.S)
    print("stacked against blocks: %.2e of S" % err)
    assert err <= 16 * IL.EPS and np.array_equal(a.diagB, b.diagB) and np.allclose(a.S, b.S, rtol=1e-13, atol=0)


# ------------------------------------------------------------------ central differences of the restatement's own L
def _L(kernel, x, yerr, u, jitter, method, r):
    return IL.reference(kernel, x, yerr, u, jitter, method, r, want_grad=False).L


@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("name,n,m,inducing", [("m32_1d", 200, 30, "maxmin"), ("m32_3d", 257, 65, "maxmin"), ("comp_3d", 120, 40, "random")])
def test_gradient_parts_against_central_differences(name, n, m, inducing, method):
    kernel, x, yerr, r, u = _case(name, n, m, inducing)
    kernel = copy.deepcopy(kernel)
    jitter = 1e-10 * float(np.mean(solver_np.kernel_matrix(kernel, u, diag=True)))        # absolute: a constant of the derivative
    ref = IL.reference(kernel, x, yerr, u, jitter, method, r)
    if method == "fitc":                                                                   # (the clamp is inactive)
        assert np.all(ref.base.lam > yerr ** 2)
    mask = kernel.unfrozen_mask
    p0 = kernel.get_parameter_vector()
    fd = np.empty(len(p0))
    for a in range(len(p0)):
        Ls = []
        for sign in (1.0, -1.0):
            p = p0.copy()
            p[a] += sign * H
            kernel.set_parameter_vector(p)
            Ls.append(_L(kernel, x, yerr, u, jitter, method, r))
        fd[a] = (Ls[0] - Ls[1]) / (2 * H)
    kernel.set_parameter_vector(p0)
    err = np.max(np.abs(fd - ref.kgrad[mask])) / np.max(np.abs(ref.kgrad[mask]))
    print("%s %s kgrad: %s  central differences: %s  error over the largest entry %.2e" % (name, method, ref.kgrad[mask], fd, err))
    assert err <= FD_BOUND
    # v = dL/dmean = -dL/dr and diagB = dL/dC_ii (through the error bar of point i)
    pts = [0, 1, 2, 5, 17, n // 2, n - 2, n - 1]
    fv, fb = np.empty(len(pts)), np.empty(len(pts))
    for q, j in enumerate(pts):
        hr = H * np.max(np.abs(r))
        hk = H * yerr[j] ** 2
        Lr, Lk = [], []
        for sign in (1.0, -1.0):
            rr = r.copy()
            rr[j] += sign * hr
            Lr.append(_L(kernel, x, yerr, u, jitter, method, rr))
            ye = yerr.copy()
            ye[j] = np.sqrt(yerr[j] ** 2 + sign * hk)
            Lk.append(_L(kernel, x, ye, u, jitter, method, r))
        fv[q] = -(Lr[0] - Lr[1]) / (2 * hr)
        fb[q] = (Lk[0] - Lk[1]) / (2 * hk)
    ev = np.max(np.abs(fv - ref.v[pts])) / np.max(np.abs(ref.v))
    eb = np.max(np.abs(fb - ref.diagB[pts])) / np.max(np.abs(ref.diagB))
    print("%s %s v: error %.2e   diagB: error %.2e" % (name, method, ev, eb))
    assert ev <= FD_BOUND and eb <= FD_BOUND


# ------------------------------------------------------------------ u = x without jitter: the dense leave-one-out
@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_all_points_inducing_is_the_dense_leave_one_out(method):
    kernel, x, yerr, r, u = _case("m32_3d", 120, 120, "all")
    ref = IL.reference(kernel, x, yerr, u, 0.0, method, r)
    d = loo_ref.reference(kernel, x, yerr, r)
    bound = 100 * IL.EPS * np.linalg.cond(solver_np.kernel_matrix(kernel, x))
    errs = dict(L=IL.rel(ref.L, d.L), resid=IL.rel(ref.resid, d.resid), var=IL.rel(ref.var, d.var), lpd=IL.rel(ref.lpd, d.lpd),
                v=IL.rel(ref.v, d.v), diagB=IL.rel(ref.diagB, d.diagB), kgrad=IL._over(ref.kgrad - d.g, ref.S))
    print(method, "bound %.2e" % bound, {key: "%.1e" % e for key, e in errs.items()})
    assert max(errs.values()) <= bound <= 1e-9
    # with m < N it is another quantity
    kernel, x, yerr, r, u = _case("m32_3d", 120, 30)
    far = IL.reference(kernel, x, yerr, u, 1e-10, method, r)
    assert IL.rel(far.resid, d.resid) > 1e-3


# ------------------------------------------------------------------ the defects
@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_every_defect_is_rejected_by_the_bound_of_the_device_tests(method):
    kernel, x, yerr, r, u = _case("m32_3d", 300, 65)
    jitter, tol = IL.tolerances(kernel, x, yerr, u, 1e-10, method, r)
    ref = IL.reference(kernel, x, yerr, u, jitter, method, r)
    for defect in IL.DEFECTS:
        bad = IL.reference(kernel, x, yerr, u, jitter, method, r, defect=defect)
        eg, eb = IL._over(bad.kgrad - ref.kgrad, ref.S), IL.rel(bad.diagB, ref.diagB)
        print("%-18s %s  kgrad %.2e of S (bound %.2e)  diagB %.2e (bound %.2e)" % (defect, method, eg, tol["kgrad"], eb, tol["diagB"]))
        if method == "dtc" and defect in ("fitc_weight_half", "z_phi_zero"):
            assert eg == 0.0 and eb == 0.0
        else:
            assert eg > tol["kgrad"] or eb > tol["diagB"]
        assert (eb > tol["diagB"]) == (defect == "d2_without_s")
        if method == "fitc":                                              # under FITC every defect shows in the kernel gradient
            assert eg > tol["kgrad"]


# ------------------------------------------------------------------ GP routing
class LowRankSolver(MinimalSolver):
    """a solver that offers ``loo_lowrank`` and neither ``loo`` nor ``loo_blocks``: what it is asked, and canned answers"""
    asked = None

    def get_inverse(self):
        raise AssertionError("the generic N x N branch was taken")

    def loo_lowrank(self, r, which=None):
        type(self).asked = (np.array(r), None if which is None else np.array(which))
        n = len(r)
        lpd = -np.arange(1.0, n + 1)
        if which is None:
            return float(np.sum(lpd)), 0.5 * np.asarray(r), np.full(n, 2.0), lpd, None, None, None
        return float(np.sum(lpd)), 0.5 * np.asarray(r), np.full(n, 2.0), lpd, 10.0 + np.arange(len(which)), np.ones(n), np.full(n, 3.0)


class BlocksAndLowRankSolver(LowRankSolver):
    def loo_blocks(self, r, which=None):
        out = self.loo_lowrank(r, which)
        return (out[0] - 1000.0,) + out[1:]


class AllThreeSolver(BlocksAndLowRankSolver):
    def loo(self, r, which=None):
        out = self.loo_lowrank(r, which)
        return (out[0] - 2000.0,) + out[1:]


def _routed_gp(solver):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6) + 0.4 * kernels.Matern32Kernel(2.5)
    kernel.freeze_parameter("k2:k1:log_constant")
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=np.log(0.02), c=0.05), fit_white_noise=True, solver=solver)
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(0.0, 10.0, 40))
    gp.compute(x, 0.15 + 0.05 * rng.rand(40))
    return gp, x, np.sin(x)


def test_gp_takes_loo_lowrank_where_the_solver_has_neither_loo_nor_loo_blocks():
    gp, x, y = _routed_gp(LowRankSolver)
    r = y - (0.25 * x - 0.8)
    n = len(x)
    lpd = -np.arange(1.0, n + 1)
    assert gp.loo_log_likelihood(y) == np.sum(lpd)
    assert np.allclose(LowRankSolver.asked[0], r, rtol=0, atol=1e-15) and LowRankSolver.asked[1] is None       # values only: no mask
    assert np.array_equal(gp.loo_log_likelihood(y, pointwise=True), lpd)
    mu, var = gp.loo_predict(y)
    assert np.allclose(mu, y - 0.5 * r, rtol=0, atol=1e-15) and np.array_equal(var, np.full(n, 2.0))
    g = gp.grad_loo_log_likelihood(y)
    mask = gp.kernel.unfrozen_mask
    assert np.array_equal(LowRankSolver.asked[1], mask.astype(np.uint32)) and not np.all(mask)                 # the unfrozen mask
    wn = np.exp(np.log(0.02) + 0.05 * x)
    want = np.concatenate([[np.sum(x), n], [3.0 * np.sum(wn), 3.0 * np.sum(wn * x)], (10.0 + np.arange(len(mask)))[mask]])
    assert np.allclose(g, want, rtol=1e-14, atol=0)
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector(), y)
    assert val == -np.sum(lpd) and np.allclose(grad, -want, rtol=1e-14, atol=0)


def test_loo_wins_over_loo_blocks_which_wins_over_loo_lowrank():
    n = 40
    base = -np.sum(np.arange(1.0, n + 1))
    gp, x, y = _routed_gp(BlocksAndLowRankSolver)
    assert gp.loo_log_likelihood(y) == base - 1000.0
    gp, x, y = _routed_gp(AllThreeSolver)
    assert gp.loo_log_likelihood(y) == base - 2000.0


def test_the_generic_branch_is_still_there(monkeypatch):
    gp, x, y = _routed_gp(MinimalSolver)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    assert np.isfinite(gp.loo_log_likelihood(y)) and gp.grad_loo_log_likelihood(y).shape == (len(gp),)


# ------------------------------------------------------------------ what is offered, and what is refused
def test_only_the_inducing_solver_offers_loo_lowrank():
    from george_amd import BasicSolver, HODLRSolver, VecchiaSolver
    assert callable(InducingSolver.loo_lowrank)
    for cls in (BasicSolver, HODLRSolver, VecchiaSolver):
        assert getattr(cls, "loo_lowrank", None) is None


def test_signature_and_argument_checks_without_a_gpu():
    _vp = ctypes.c_void_p
    assert N.SIGNATURES["gh_inducing_loo"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double)] + [_vp] * 6)
    assert N.SIGNATURES["gh_inducing_loo"] == N.SIGNATURES["gh_vecchia_loo"] and hasattr(N.lib, "gh_inducing_loo")
    buf, total = np.zeros(4), ctypes.c_double(0.0)
    assert N.lib.gh_inducing_loo(None, None, None, N.ptr(buf), ctypes.byref(total), N.ptr(buf), N.ptr(buf), None, None, None, None) == N.GH_ERR_BAD_ARG
    with pytest.raises(ValueError):                                   # no handle
        N.check(N.lib.gh_inducing_loo(None, None, None, N.ptr(buf), ctypes.byref(total), N.ptr(buf), N.ptr(buf), None, None, None, None))
    s = InducingSolver(kernels.ExpSquaredKernel(1.0), inducing=4)
    with pytest.raises(RuntimeError, match="compute"):                # never computed, as BasicSolver.loo
        s.loo_lowrank(np.zeros(4))
    with pytest.raises(RuntimeError, match="compute"):
        s.loo_lowrank(np.zeros(4), np.ones(1))
