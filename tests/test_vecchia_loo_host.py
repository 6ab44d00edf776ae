"""The host side of tests/test_gpu_vecchia_loo.py: the restatement of the Vecchia leave-one-out (tests/vecchia_loo_ref.py) against
the dense leave-one-out by LAPACK (tests/loo_ref.py) with every predecessor in the conditioning set, its gradient parts against
central differences of its own ``L``, the problems of the device tests against the cap on the gap, ``GP`` routing to
``loo_blocks``, and the inputs that are refused.  No device is touched.

Central differences.  ``L`` is smooth in the log-parameters, the residuals and the diagonal of ``K``; with the step ``h`` the
central difference has a truncation error of ``h^2 / 6 |L'''|`` and a rounding error of about ``eps |L| / h``.  At ``h = 1e-5``
(relative to the variable's scale) and ``|L|`` a few hundred that is 1e-10 and 1e-8 of a derivative of order one: the bound is
``FD_BOUND = 1e-6`` of the largest entry of each of ``kgrad``, ``v`` and ``diagB``, a hundred times that, while every structural
error -- a missing factor 2 on the diagonal, ``z[c] = 0`` instead of ``h_last``, a dropped block -- is of order one.

Observed on the CPU (every test prints its figures): the two routes differ by at most 1.7e-12 (``diagB``, the composite kernel)
on 150 points and by 7e-12 with five bare points; central differences agree to 9e-9 (``kgrad``), 3e-11 (``v``) and 8e-10
(``diagB``).
"""
import copy
import ctypes

import numpy as np
import pytest

from george_amd import GP, BasicSolver, VecchiaSolver, kernels
from george_amd import _native as N
from george_amd.solvers.vecchia import vecchia_neighbors

import vecchia_cases as VC
import vecchia_loo_ref as VL
from test_fisher_host import LinearMean, MinimalSolver, NoiseRamp, _host_gradient
from test_gpu_vecchia import _problem

FD_BOUND = 1e-6
H = 1e-5


# ------------------------------------------------------------------ full conditioning: the dense leave-one-out
@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d", "hyper"])
def test_full_conditioning_is_the_dense_leave_one_out(name):
    """m = N - 1 at N = 150: all seven outputs and ``c`` are the dense ones, far inside the cap on the gap; with few neighbours
    they are another quantity"""
    kernel, x, yerr, r, _ = _problem(name, 150)
    g, ref, dense = VL.gaps(kernel, x, yerr, r)
    print(name, {key: "%.1e" % v for key, v in g.items()})
    assert sorted(g) == sorted(("L", "kgrad") + VL.VECTORS) and max(g.values()) <= VL.GAP_CAP
    assert np.all(ref.var > 0.0) and np.all(ref.S > 0.0)
    near = VL.reference(kernel, x, yerr, vecchia_neighbors(x, 2), r)
    assert VL._over(near.kgrad - dense.g, ref.S) > 1e3 * VL.CAP and VL.vecchia_ref.rel(near.resid, dense.resid) > 1e3 * VL.CAP


# ------------------------------------------------------------------ central differences of the restatement's own L
def _fd_problem(which):
    n, m = 60, 12
    kernel, x, yerr, r, _ = _problem("m32_1d" if which == "1d" else "expsq_3d", n)
    nbr = VL.irregular_table(n, m) if which == "irregular" else vecchia_neighbors(x, m)
    return copy.deepcopy(kernel), x, yerr, r, nbr


def _L(kernel, x, yerr, nbr, r):
    return VL.reference(kernel, x, yerr, nbr, r, want_grad=False).L


@pytest.mark.parametrize("which", ["1d", "3d", "irregular"])
def test_gradient_parts_against_central_differences(which):
    kernel, x, yerr, r, nbr = _fd_problem(which)
    ref = VL.reference(kernel, x, yerr, nbr, r)
    p0 = kernel.get_parameter_vector()
    fd = np.empty(len(p0))
    for a in range(len(p0)):
        Ls = []
        for sign in (1.0, -1.0):
            p = p0.copy()
            p[a] += sign * H
            kernel.set_parameter_vector(p)
            Ls.append(_L(kernel, x, yerr, nbr, r))
        fd[a] = (Ls[0] - Ls[1]) / (2 * H)
    kernel.set_parameter_vector(p0)
    err = np.max(np.abs(fd - ref.kgrad)) / np.max(np.abs(ref.kgrad))
    print("%s kgrad: %s  central differences: %s  error over the largest entry %.2e" % (which, ref.kgrad, fd, err))
    assert err <= FD_BOUND
    # v = dL/dmean = -dL/dr and diagB = dL/dK_jj (through the error bar of point j), at the first and last points, point 0's
    # neighbourhood and some in the middle
    pts = [0, 1, 2, 5, 17, 30, 31, 58, 59]
    fv, fb = np.empty(len(pts)), np.empty(len(pts))
    for q, j in enumerate(pts):
        hr = H * np.max(np.abs(r))
        hk = H * yerr[j] ** 2
        Lr, Lk = [], []
        for sign in (1.0, -1.0):
            rr = r.copy()
            rr[j] += sign * hr
            Lr.append(_L(kernel, x, yerr, nbr, rr))
            ye = yerr.copy()
            ye[j] = np.sqrt(yerr[j] ** 2 + sign * hk)
            Lk.append(_L(kernel, x, ye, nbr, r))
        fv[q] = -(Lr[0] - Lr[1]) / (2 * hr)
        fb[q] = (Lk[0] - Lk[1]) / (2 * hk)
    ev = np.max(np.abs(fv - ref.v[pts])) / np.max(np.abs(ref.v))
    eb = np.max(np.abs(fb - ref.diagB[pts])) / np.max(np.abs(ref.diagB))
    print("%s v: error %.2e   diagB: error %.2e" % (which, ev, eb))
    assert ev <= FD_BOUND and eb <= FD_BOUND


def test_the_irregular_table_has_the_longest_and_the_empty_columns():
    n, m = 777, 24
    tab = VL.irregular_table(n, m)
    cols = np.bincount(tab[tab >= 0], minlength=n)
    assert cols[0] == n - 1 and np.all(cols[2::3] == 0) and np.any(cols[1::3] > 0)
    counts = (tab >= 0).sum(axis=1)
    assert counts.min() == 0 and counts.max() == m
    assert np.any(np.diff(tab, axis=1)[(tab[:, 1:] >= 0) & (tab[:, :-1] >= 0)] < 0)
    assert np.any((tab[:, :-1] < 0) & (tab[:, 1:] >= 0))                    # padding in the middle of a row
    for i in range(n):
        c = tab[i][tab[i] >= 0]
        assert np.all(c < i) and len(np.unique(c)) == len(c)


# ------------------------------------------------------------------ the problems of the device tests stay inside the cap
@pytest.mark.parametrize("name,n", [("m32_1d", 777), ("expsq_3d", 777), ("hyper", 300), ("m32_1d", 65), ("expsq_3d", 65), ("expsq_3d", 1),
                                    ("expsq_3d", 2), ("m32_1d", 1), ("m32_1d", 4099), ("m32_1d", 20011), (5, 300), (17, 300), (64, 300)])
def test_the_two_cpu_routes_stay_inside_the_cap(name, n):
    """every problem of tests/test_gpu_vecchia_loo.py: ``tolerances`` asserts the cap on the gap"""
    kernel, x, yerr, r = VC.pcase(name, n)[:4] if isinstance(name, int) else _problem(name, n, 250.0 if n == 20011 else 10.0)[:4]
    tol = VL.tolerances(kernel, x, yerr, r)
    assert all(4000 * VL.EPS <= t <= VL.CAP for t in tol.values()), tol


def test_the_cap_with_fitted_noise_and_with_bare_points():
    """the two remaining problems of the device tests: the composite kernel with a white-noise ramp on its error bars (group i),
    and the Matern problem with no error bar at five points (group h)"""
    kernel, x, yerr, y, _ = _problem("hyper", 300)
    t = x[:, 0]
    ye = np.sqrt(yerr ** 2 + np.exp(np.log(0.5 * np.min(yerr ** 2)) + 0.1 * t))
    VL.tolerances(kernel, x, ye, y - (0.25 * t - 0.8))
    kernel, x, yerr, r, _ = _problem("m32_1d", 300)
    yerr = yerr.copy()
    yerr[[3, 40, 41, 150, 299]] = 0.0
    VL.tolerances(kernel, x, yerr, r)
    # under a narrow LocalGaussianKernel exactly the blocks that hold a bare point fail, and the rest still count
    other = kernels.LocalGaussianKernel(location=float(x[100, 0]), log_width=np.log(1e-3))
    nbr = vecchia_neighbors(x, 7)
    ref = VL.reference(kernel, x, yerr, nbr, r, block_spec=other)
    hit = [i for i in range(300) if np.intersect1d(np.concatenate([nbr[i][nbr[i] >= 0], [i]]), [3, 40, 41, 150, 299]).size]
    assert sorted(ref.failed) == hit and 5 < len(hit) < 60 and np.all(ref.S > 0.0) and np.all(ref.diagB[[3, 40, 41, 150, 299]] == 0.0)
    assert VL.reference(kernel, x, yerr, nbr, r).failed == []


# ------------------------------------------------------------------ GP routing
class BlocksSolver(MinimalSolver):
    """a solver that offers ``loo_blocks`` and no ``loo``: what it is asked, and canned answers"""
    asked = None

    def get_inverse(self):
        raise AssertionError("the generic N x N branch was taken")

    def loo_blocks(self, r, which=None):
        type(self).asked = (np.array(r), None if which is None else np.array(which))
        n = len(r)
        lpd = -np.arange(1.0, n + 1)
        if which is None:
            return float(np.sum(lpd)), 0.5 * np.asarray(r), np.full(n, 2.0), lpd, None, None, None
        return float(np.sum(lpd)), 0.5 * np.asarray(r), np.full(n, 2.0), lpd, 10.0 + np.arange(len(which)), np.ones(n), np.full(n, 3.0)


class BothSolver(BlocksSolver):
    def loo(self, r, which=None):
        out = self.loo_blocks(r, which)
        return (out[0] - 1000.0,) + out[1:]


def _routed_gp(solver):
    kernel = 1.3 * kernels.ExpSquaredKernel(0.6) + 0.4 * kernels.Matern32Kernel(2.5)
    kernel.freeze_parameter("k2:k1:log_constant")
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=np.log(0.02), c=0.05), fit_white_noise=True, solver=solver)
    rng = np.random.RandomState(8)
    x = np.sort(rng.uniform(0.0, 10.0, 40))
    gp.compute(x, 0.15 + 0.05 * rng.rand(40))
    return gp, x, np.sin(x)


def test_gp_takes_loo_blocks_where_the_solver_has_no_loo():
    gp, x, y = _routed_gp(BlocksSolver)
    r = y - (0.25 * x - 0.8)
    n = len(x)
    lpd = -np.arange(1.0, n + 1)
    assert gp.loo_log_likelihood(y) == np.sum(lpd)
    assert np.allclose(BlocksSolver.asked[0], r, rtol=0, atol=1e-15) and BlocksSolver.asked[1] is None      # values only: no mask
    assert np.array_equal(gp.loo_log_likelihood(y, pointwise=True), lpd)
    mu, var = gp.loo_predict(y)
    assert np.allclose(mu, y - 0.5 * r, rtol=0, atol=1e-15) and np.array_equal(var, np.full(n, 2.0))
    g = gp.grad_loo_log_likelihood(y)
    mask = gp.kernel.unfrozen_mask
    assert np.array_equal(BlocksSolver.asked[1], mask.astype(np.uint32)) and not np.all(mask)
    wn = np.exp(np.log(0.02) + 0.05 * x)
    # mean | white noise | kernel from v = 1, diagB = 3 with diag_weight = 1, and the unfrozen slots of grad_full
    want = np.concatenate([[np.sum(x), n], [3.0 * np.sum(wn), 3.0 * np.sum(wn * x)], (10.0 + np.arange(len(mask)))[mask]])
    assert np.allclose(g, want, rtol=1e-14, atol=0)
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector(), y)
    assert val == -np.sum(lpd) and np.allclose(grad, -want, rtol=1e-14, atol=0)


def test_loo_wins_over_loo_blocks():
    gp, x, y = _routed_gp(BothSolver)
    n = len(x)
    assert gp.loo_log_likelihood(y) == -np.sum(np.arange(1.0, n + 1)) - 1000.0


def test_the_generic_branch_is_still_there(monkeypatch):
    gp, x, y = _routed_gp(MinimalSolver)
    monkeypatch.setattr(gp.kernel, "get_gradient", _host_gradient(gp.kernel), raising=False)
    assert np.isfinite(gp.loo_log_likelihood(y)) and gp.grad_loo_log_likelihood(y).shape == (len(gp),)


# ------------------------------------------------------------------ what is offered, and what is refused
def test_only_the_vecchia_solver_offers_loo_blocks():
    from george_amd import HODLRSolver, InducingSolver
    assert callable(VecchiaSolver.loo_blocks) and getattr(VecchiaSolver, "loo", None) is None
    assert callable(BasicSolver.loo) and getattr(BasicSolver, "loo_blocks", None) is None
    for cls in (HODLRSolver, InducingSolver):
        assert getattr(cls, "loo", None) is None and getattr(cls, "loo_blocks", None) is None


def test_signature_and_argument_checks_without_a_gpu():
    _vp = ctypes.c_void_p
    assert N.SIGNATURES["gh_vecchia_loo"] == (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double)] + [_vp] * 6)
    buf, total = np.zeros(4), ctypes.c_double(0.0)
    with pytest.raises(ValueError):                                   # no handle
        N.check(N.lib.gh_vecchia_loo(None, None, None, N.ptr(buf), ctypes.byref(total), N.ptr(buf), N.ptr(buf), None, None, None, None))
    s = VecchiaSolver(kernels.ExpSquaredKernel(1.0), m=4)
    with pytest.raises(RuntimeError, match="compute"):                # never computed, as BasicSolver.loo
        s.loo_blocks(np.zeros(4))
