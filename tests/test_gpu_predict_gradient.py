"""Input derivatives of the prediction on the device (``-m gpu``): gh_chol_predict_grad, BasicSolver.predict_gradient and
GP.predict_gradient against the CPU reference of tests/predgrad_ref.py under its one tolerance rule
(``|x - x_ref| <= 32 * 2^-53 * kappa * S``), against the reduction they are defined as on the device's own solves, against
``predict``, and against themselves (with / without the variance, call / call again, appended-and-removed / fresh factor).

The sizes are where the padding to 128 (points and test points), the 64-point column tile, the 128-row tile and the row
chunks of the reduction can go wrong."""
import functools

import numpy as np
import pytest
import scipy.optimize

import predgrad_ref as R
from predict_ref import U
from george_amd import GP, BasicSolver, HODLRSolver, kernels as K
from george_amd.gp import TINY

pytestmark = pytest.mark.gpu

R_X = 1e-10          # the relative tolerance tests/test_gpu_kernels.py grants the device's x-gradients against the oracle

GENERAL_METRIC = np.array([[1.0, 0.3, 0.1], [0.3, 1.5, 0.2], [0.1, 0.2, 0.8]])
KERNELS = {
    # the fast form a + b F(r2): register-only instantiations in 1 and 3 dimensions
    "expsq_1d": (lambda: 1.3 * K.ExpSquaredKernel(0.6), 1),
    "matern32_axis_3d": (lambda: 0.9 * K.Matern32Kernel([1.0, 2.5, 0.6], ndim=3), 3),
    "ratquad_3d": (lambda: 0.8 * K.RationalQuadraticKernel(log_alpha=0.4, metric=1.2, ndim=3) + K.ConstantKernel(-2.0, ndim=3), 3),
    # off the fast form: the interpreter
    "sum2_1d": (lambda: 1.1 * K.ExpSquaredKernel(0.7) + 0.4 * K.Matern52Kernel(2.5), 1),
    "blocked_1d": (lambda: 0.6 * K.ExpSquaredKernel(1.5) + 0.7 * K.Matern32Kernel(0.8, block=(2.0, 6.0)), 1),
    "poly_3d": (lambda: 0.7 * K.ExpSquaredKernel([0.8, 1.5, 0.6], ndim=3) + 0.02 * K.PolynomialKernel(log_sigma2=0.1, order=2, ndim=3), 3),
    "dot_1d": (lambda: 0.9 * K.Matern32Kernel(1.2) + 0.05 * K.DotProductKernel(), 1),
    # (a well-conditioned matrix.  Under zoo._spd(3, 7) the metric's forward substitution cancels up to 87-fold, and the ORACLE's
    #  own fp64 x-gradient is then 49 U away from a long-double evaluation of the same formula -- more than the 32 U the rule
    #  leaves at kappa = 1; the device missed the rule there by 1.35 at N = 1, M = 129.  Under this matrix the oracle's own
    #  error is 7 U at most.)
    "general_3d": (lambda: 1.2 * K.ExpSquaredKernel(metric=GENERAL_METRIC, ndim=3), 3),
}
# (kernel, N, M): N and M from {1, 5, 127, 128, 129, 300} x {1, 5, 64, 65, 129, 300}, every value with both evaluators
CASES = [
    ("expsq_1d", 1, 1), ("expsq_1d", 5, 5), ("expsq_1d", 127, 64), ("expsq_1d", 128, 65), ("expsq_1d", 129, 129),
    ("expsq_1d", 300, 300),
    ("matern32_axis_3d", 1, 5), ("matern32_axis_3d", 129, 1), ("matern32_axis_3d", 128, 300), ("matern32_axis_3d", 300, 65),
    ("ratquad_3d", 127, 129), ("ratquad_3d", 5, 64),
    ("sum2_1d", 129, 65), ("sum2_1d", 300, 5), ("sum2_1d", 1, 64),
    ("blocked_1d", 128, 64), ("blocked_1d", 300, 129),
    ("poly_3d", 5, 1), ("poly_3d", 127, 65), ("poly_3d", 300, 300),
    ("dot_1d", 129, 5), ("dot_1d", 128, 129),
    ("general_3d", 300, 64), ("general_3d", 1, 129), ("general_3d", 127, 300),
]


@functools.lru_cache(maxsize=None)
def _problem(name, n, m):
    make, nd = KERNELS[name]
    rng = np.random.RandomState(1000 * nd + 7 * n + m)
    if nd == 1:
        x = np.sort(rng.uniform(0.0, 10.0, n))[:, None]
    else:
        x = rng.uniform(0.0, 3.0, (n, nd))
    # every test point lies within 0.4 per coordinate of SOME training point (and so inside and outside the data's hull and
    # the blocked kernel's block).  The rule has no term for the evaluator's own rounding: an exp-type kernel carries a relative
    # error of about (r2 / 2) c U from the c roundings of its argument, which the rule's C_TOL kappa U covers only while r2 is
    # small -- and kappa is 1 at N = 1.  A test point far from every training point (r2 = 28 occurred with uniform test
    # points at N = 1 under the general metric: 2.0 times the tolerance in mu and dmu, 4.0 in dvar, gh_chol_predict's mu
    # included) tests the evaluator against the oracle, which tests/test_gpu_kernels.py does at 1e-10, not this reduction.
    xs = x[rng.randint(0, n, m)] + rng.uniform(-0.4, 0.4, (m, nd))
    yerr = 0.15 + 0.05 * rng.rand(n)
    r = np.sin(x.sum(axis=1)) + 0.1 * rng.randn(n)
    return make(), x, yerr, r, xs


@functools.lru_cache(maxsize=None)
def _reference(name, n, m):
    return R.reference(*_problem(name, n, m))


def _reduction_law(label, solver, kernel, x, r, xs, G, D, dmu, dvar):
    """(b): the results are the reduction of the oracle's G against the device's OWN solves, within what any summation order
    (N U times the sum of the absolute terms) and the evaluator's allowance (R_X) can differ"""
    n = len(x)
    a = np.asarray(solver.apply_inverse(r)).reshape(-1)
    Wd = np.asarray(solver.apply_inverse(np.ascontiguousarray(kernel.get_value(x, xs)))).reshape(n, len(xs))
    f = n * U + R_X
    em = np.abs(dmu - np.einsum("cid,i->cd", G, a))
    bm = f * np.einsum("cid,i->cd", np.abs(G), np.abs(a))
    ev = np.abs(dvar - (D - 2.0 * np.einsum("cid,ic->cd", G, Wd)))
    bv = f * (np.abs(D) + 2.0 * np.einsum("cid,ic->cd", np.abs(G), np.abs(Wd)))
    qm, qv = R.GRef._ratio(em, bm), R.GRef._ratio(ev, bv)
    print("%s: reduction law, error / bound dmu %.3g dvar %.3g" % (label, qm, qv))
    assert qm <= 1.0 and qv <= 1.0, (label, qm, qv)


@pytest.mark.parametrize("name,n,m", CASES)
def test_against_the_reference_the_reduction_law_and_predict(name, n, m):
    kernel, x, yerr, r, xs = _problem(name, n, m)
    ref = _reference(name, n, m)
    nd = x.shape[1]
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    mu, var, dmu, dvar = s.predict_gradient(kernel, r, xs, return_var=True)
    assert mu.shape == var.shape == (m,) and dmu.shape == dvar.shape == (m, nd)
    # (a) the reference, under the rule
    ratios = dict(mu=ref.pred.ratio_mu(mu), var=ref.pred.ratio_var(var), dmu=ref.ratio_dmu(dmu), dvar=ref.ratio_dvar(dvar))
    label = "%s N=%d M=%d" % (name, n, m)
    print("%s: kappa %.3g, error / tolerance %s" % (label, ref.kappa, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    assert max(ratios.values()) <= 1.0, (label, ratios)
    # (b) the reduction law
    _reduction_law(label, s, kernel, x, r, xs, ref.G, ref.D, dmu, dvar)
    # (c) mu and var are predict's, bit for bit
    pmu, pvar, _ = s.predict(kernel, r, xs, return_var=True)
    assert np.array_equal(mu, pmu) and np.array_equal(var, pvar)
    # (d) two calls give the same bits
    again = s.predict_gradient(kernel, r, xs, return_var=True)
    for p, q in zip((mu, var, dmu, dvar), again):
        assert np.array_equal(p, q)
    # (e) the mean part does not depend on whether the variance part is compiled in
    mu0, var0, dmu0, dvar0 = s.predict_gradient(kernel, r, xs)
    assert var0 is None and dvar0 is None and np.array_equal(dmu0, dmu) and np.array_equal(mu0, mu)
    # ... nor on whether the values are formed at all (dmu alone: the two sweeps for alpha, no K(x, xs))
    mu1, var1, dmu1, dvar1 = s.predict_gradient(kernel, r, xs, return_value=False)
    assert mu1 is None and var1 is None and dvar1 is None and np.array_equal(dmu1, dmu)
    mu2, var2, dmu2, dvar2 = s.predict_gradient(kernel, r, xs, return_var=True, return_value=False)
    assert mu2 is None and var2 is None and np.array_equal(dmu2, dmu) and np.array_equal(dvar2, dvar)


def test_row_chunks_of_more_than_one_tile_n8320():
    # 65 row tiles of 128: the reduction's chunks hold two tiles (and the last chunk one)
    n, m = 8320, 3
    for name in ("matern32_axis_3d", "sum2_1d"):
        kernel, x, yerr, r, xs = _problem(name, n, m)
        s = BasicSolver(kernel)
        s.compute(x, yerr)
        mu, var, dmu, dvar = s.predict_gradient(kernel, r, xs, return_var=True)
        G, D = R.gradients(kernel, xs, x)
        _reduction_law("%s N=%d M=%d" % (name, n, m), s, kernel, x, r, xs, G, D, dmu, dvar)
        pmu, pvar, _ = s.predict(kernel, r, xs, return_var=True)
        assert np.array_equal(mu, pmu) and np.array_equal(var, pvar)
        again = s.predict_gradient(kernel, r, xs, return_var=True)
        assert np.array_equal(again[2], dmu) and np.array_equal(again[3], dvar)
        assert np.array_equal(s.predict_gradient(kernel, r, xs)[2], dmu)
        assert np.array_equal(s.predict_gradient(kernel, r, xs, return_value=False)[2], dmu)


@pytest.mark.parametrize("name", ["expsq_1d", "poly_3d"])
def test_a_factor_that_was_appended_to_and_removed_from(name):
    kernel, x, yerr, r, xs = _problem(name, 300, 65)
    drop = np.array([3, 130, 131, 207, 298])
    keep = np.setdiff1d(np.arange(300), drop)
    s = BasicSolver(kernel)
    s.compute(x[:250], yerr[:250])
    s.append(x[250:], yerr[250:])
    s.remove(drop)
    mu, var, dmu, dvar = s.predict_gradient(kernel, r[keep], xs, return_var=True)
    ref = R.reference(kernel, x[keep], yerr[keep], r[keep], xs)
    ratios = dict(mu=ref.pred.ratio_mu(mu), var=ref.pred.ratio_var(var), dmu=ref.ratio_dmu(dmu), dvar=ref.ratio_dvar(dvar))
    print("%s after append and remove (%s): kappa %.3g, error / tolerance %s" % (name, s.last_remove_path, ref.kappa, ratios))
    assert max(ratios.values()) <= 1.0, ratios
    fresh = BasicSolver(kernel)
    fresh.compute(x[keep], yerr[keep])
    fmu, fvar, fdmu, fdvar = fresh.predict_gradient(kernel, r[keep], xs, return_var=True)
    assert max(ref.pred.ratio_mu(fmu), ref.pred.ratio_var(fvar), ref.ratio_dmu(fdmu), ref.ratio_dvar(fdvar)) <= 1.0


def test_gp_on_the_dense_solver_and_on_hodlr():
    # (f) the device call against the generic NumPy branch on another solver.  HODLR approximates; the rule's tolerances are
    # those of exact solvers.  Matern-3/2 on sorted one-dimensional points has off-diagonal blocks of rank exactly 2, which
    # the factorisation at tol = 1e-12 represents exactly: its solves then differ from the dense ones by rounding alone.
    rng = np.random.RandomState(5)
    n, m = 300, 65
    x = np.sort(rng.uniform(0.0, 10.0, n))
    yerr = 0.15 + 0.05 * rng.rand(n)
    y = 0.4 + np.sin(x) + 0.1 * rng.randn(n)
    t = rng.uniform(-0.5, 10.5, m)
    make = lambda: 0.9 * K.Matern32Kernel(1.2)            # noqa: E731
    dense = GP(make(), mean=0.4, solver=BasicSolver)
    hodlr = GP(make(), mean=0.4, solver=HODLRSolver, tol=1e-12)
    dense.compute(x, yerr)
    hodlr.compute(x, yerr)
    assert callable(getattr(dense.solver, "predict_gradient", None)) and not callable(getattr(hodlr.solver, "predict_gradient", None))
    ref = R.reference(dense.kernel, x[:, None], np.sqrt(yerr ** 2 + TINY), y - 0.4, t[:, None], mean_t=0.4)
    a = dense.predict_gradient(y, t, return_var=True, return_value=True)
    b = hodlr.predict_gradient(y, t, return_var=True, return_value=True)
    tols = (ref.pred.tol_mu(), ref.pred.tol_var(), ref.tol_dmu(), ref.tol_dvar())
    ratios = [R.GRef._ratio(p - q, 2.0 * tol) for p, q, tol in zip(a, b, tols)]
    print("dense against HODLR (tol 1e-12): kappa %.3g, error / (two tolerances) mu %.3g var %.3g dmu %.3g dvar %.3g"
          % ((ref.kappa,) + tuple(ratios)))
    assert max(ratios) <= 1.0
    assert max(ref.pred.ratio_mu(a[0]), ref.pred.ratio_var(a[1]), ref.ratio_dmu(a[2]), ref.ratio_dvar(a[3])) <= 1.0
    # the four return shapes of the device branch carry the same bits
    assert np.array_equal(dense.predict_gradient(y, t), a[2])
    p, q = dense.predict_gradient(y, t, return_var=True)
    assert np.array_equal(p, a[2]) and np.array_equal(q, a[3])
    p, q = dense.predict_gradient(y, t, return_value=True)
    assert np.array_equal(p, a[0]) and np.array_equal(q, a[2])
    pm, pv = dense.predict(y, t, return_var=True)
    assert np.array_equal(pm, a[0]) and np.array_equal(pv, a[1])


def test_searching_a_fitted_gp_for_the_maxima_of_its_mean():
    # (g) the use the method is for: scipy.optimize.minimize(..., jac=True) over the test point
    rng = np.random.RandomState(12)
    x = np.sort(rng.uniform(0.0, 10.0, 80))
    y = np.sin(x) + 0.05 * rng.randn(80)
    gp = GP(1.0 * K.ExpSquaredKernel(1.0))
    gp.compute(x, 0.1)

    def neg(t):
        mu, dmu = gp.predict_gradient(y, t, return_value=True)
        return -float(mu[0]), -dmu[0]

    gtol = 1e-6
    for start in (1.2, 2.2, 7.5):
        res = scipy.optimize.minimize(neg, np.array([start]), jac=True, method="BFGS", options=dict(gtol=gtol))
        g = gp.predict_gradient(y, res.x)
        print("start %.1f -> t = %.6f, mu = %.6f, |dmu| = %.3g after %d evaluations (%s)"
              % (start, res.x[0], -res.fun, abs(g[0, 0]), res.nfev, res.message))
        assert res.success and abs(g[0, 0]) <= gtol
        near = gp.predict(y, np.array([res.x[0] - 0.01, res.x[0], res.x[0] + 0.01]), return_cov=False)
        assert near[1] >= near[0] and near[1] >= near[2]
