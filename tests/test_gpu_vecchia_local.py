"""Local (nearest-neighbour) prediction of ``VecchiaSolver`` on the device (``vecchia_local_kernel``, george_amd/csrc/gh_vecchia.hip)
against the dense device solver where every data point is in every conditioning set, and against the NumPy restatement
(tests/vecchia_local_ref.py) everywhere else.

Tolerances follow tests/test_gpu_vecchia.py.  For ``mu`` and ``var`` the bound is ``1000 x`` the gap that two float64 routes on
the CPU -- the restatement with every data point in every set, and dense LAPACK (``vecchia_ref.dense``) -- show on the test's own
inputs (``vecchia_local_ref.gaps``).  A set holds at most 64 points, so the gap is taken on the first 64 data points of the same
sorted inputs (the same point density and error bars, which set the conditioning of a block) with the test's own test points.
The margin of 1000 covers the device ``exp`` / ``sqrt`` differing from libm by a few ulp and the reordered sums; a gap counts as
at least ``4 eps``, and no bound is looser than 1e-9.  ``mu`` is measured over its largest absolute entry, ``var`` over its
largest entry.  Error bars are at least 0.1 of the kernel amplitude, except in the error-return test.  Gaps observed on the CPU
(every test prints them): mu 1.4e-14 .. 6.1e-14, var 1.3e-16 .. 5.4e-14; hyper.rst kernel, whose amplitudes span five orders of
magnitude: mu 2.1e-13, var 7.4e-14.  The device was within 2e-16 .. 2.7e-13 of the restatement on every quantity.

The fast form ``a + b F(r^2)`` exists for ``c * Stationary + Constant``; the hyper.rst kernel (four terms) and a product of two
leaves have none.  The four pairings of (data kernel, cross kernel) are reached by ``test_cross_kernel_differs_from_the_data_kernel``
and ``test_interpreter_path``.
"""
import functools

import numpy as np
import pytest

import george_amd
from george_amd import GP, BasicSolver, VecchiaSolver, kernels
from george_amd import _native as N
from george_amd.solvers.vecchia import vecchia_query_neighbors

import loo_ref
import vecchia_local_ref
import vecchia_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CAP = 1e-9
GAP_N = 64


def _kernel(name):
    if name == "m32_1d":
        return 1.7 * kernels.Matern32Kernel(0.8), 1, np.sqrt(1.7)
    if name == "m32c_1d":                                   # fast form with an offset
        return 1.7 * kernels.Matern32Kernel(0.8) + kernels.ConstantKernel(log_constant=np.log(0.3)), 1, np.sqrt(2.0)
    if name == "expsq_2d":
        return 0.9 * kernels.ExpSquaredKernel([0.3, 0.5], ndim=2), 2, np.sqrt(0.9)
    if name == "expsq_3d":
        return 0.8 * kernels.ExpSquaredKernel([0.4, 0.6, 0.9], ndim=3), 3, np.sqrt(0.8)
    return loo_ref.kernel_hyper(), 1, 66.0


@functools.lru_cache(maxsize=None)
def _problem(name, n, span=10.0, ntest=300):
    """(kernel, x, yerr, r, xs): inputs sorted by their first column, error bars 0.1 .. 0.15 of the amplitude; every seventh test
    point lies on a data point"""
    kernel, ndim, amp = _kernel(name)
    rng = np.random.RandomState(2000 * ndim + n)
    x = np.sort(rng.uniform(0, span, n))[:, None] if ndim == 1 else rng.uniform(0, 2, (n, ndim))
    x = x[np.argsort(x[:, 0], kind="stable")]
    yerr = amp * (0.1 + 0.05 * rng.rand(n))
    r = amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))
    xs = rng.uniform(0, span if ndim == 1 else 2, (ntest, ndim))
    xs[::7] = x[rng.choice(n, len(xs[::7]), replace=False)]
    return kernel, x, yerr, r, xs


@functools.lru_cache(maxsize=None)
def _tol(name, n, span=10.0, ntest=300):
    kernel, x, yerr, r, xs = _problem(name, n, span, ntest)
    k = min(n, GAP_N)
    g = vecchia_local_ref.gaps(kernel, x[:k], yerr[:k], r[:k], xs[:300])[0]
    print("gaps", name, n, g)
    return {key: min(1000.0 * max(v, 4 * EPS), CAP) for key, v in g.items()}


@functools.lru_cache(maxsize=None)
def _ref(name, n, m, span=10.0):
    kernel, x, yerr, r, xs = _problem(name, n, span)
    return vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs, vecchia_local_ref.query_neighbors(x, xs, m))


def _check(what, got, want, tol, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.max(np.abs(want)) if scale is None else scale
    err = np.max(np.abs(got - want) / scale)
    print("%-30s error %.3g  bound %.3g" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _check_pair(tag, got, want, tol):
    _check(tag + " mean", got[0], want[0], tol["mu"])
    _check(tag + " variance", got[1], want[1], tol["var"])


@pytest.mark.parametrize("name", ["m32_1d", "expsq_2d"])
def test_exact_case_against_the_dense_solver(name):
    """N = 64, m = 64: every data point is in every set, so the answers are the dense ones -- BasicSolver's, on the same device"""
    kernel, x, yerr, r, xs = _problem(name, 64, 3.0)
    tol = _tol(name, 64, 3.0)
    dense = BasicSolver(kernel)
    dense.compute(x, yerr)
    mu0, var0, _ = dense.predict(kernel, r, xs, return_var=True)
    solver = VecchiaSolver(kernel, m=64)
    solver.compute(x, yerr)
    mu, var = solver.predict_local(kernel, r, xs, return_var=True)
    _check_pair("dense:", (mu, var), (mu0, var0), tol)
    mu1, none = solver.predict_local(kernel, r, xs)
    assert none is None and np.array_equal(mu1, mu)


@pytest.mark.parametrize("m", [1, 7, 32, 64])
@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_parity_with_the_restatement(name, m):
    """N = 777, M = 300; the solver's own search against the restatement's brute force.  The solver was computed with another m."""
    kernel, x, yerr, r, xs = _problem(name, 777)
    solver = VecchiaSolver(kernel, m=16)
    solver.compute(x, yerr)
    got = solver.predict_local(kernel, r, xs, return_var=True, m=m)
    _check_pair("m=%d:" % m, got, _ref(name, 777, m), _tol(name, 777))
    s2 = VecchiaSolver(kernel, m=m, predict="local")
    s2.compute(x, yerr)
    mu, var, cov = s2.predict(kernel, r, xs, return_var=True)
    assert cov is None and np.array_equal(mu, got[0]) and np.array_equal(var, got[1])
    assert np.array_equal(s2.predict(kernel, r, xs)[0], mu) and s2.predict(kernel, r, xs)[1] is None


def test_interpreter_path():
    """the 17-node composite of docs/tutorials/hyper.rst (tests/loo_ref.py): no fast form for either kernel"""
    kernel, x, yerr, r, xs = _problem("hyper", 300)
    solver = VecchiaSolver(kernel, m=16)
    solver.compute(x, yerr)
    _check_pair("hyper:", solver.predict_local(kernel, r, xs, return_var=True), _ref("hyper", 300, 16), _tol("hyper", 300))


def _cross_cases():
    term = 1.7 * kernels.Matern32Kernel(0.8)
    no_fast = 0.5 * kernels.ExpSquaredKernel(2.0) * kernels.ExpSine2Kernel(gamma=1.0, log_period=0.5)
    return {"fast_fast": ("m32c_1d", term), "interpreter_fast": ("hyper", 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)),
            "fast_interpreter": ("m32c_1d", no_fast)}


@pytest.mark.parametrize("case", ["fast_fast", "interpreter_fast", "fast_interpreter"])
def test_cross_kernel_differs_from_the_data_kernel(case):
    """``kernel=`` one term of a sum (the prediction of a component): K_cc from the solver's kernel, k_c and k** from the term.
    (data kernel, cross kernel) on the (fast form, fast form), (interpreter, fast form) and (fast form, interpreter)."""
    name, cross = _cross_cases()[case]
    kernel, x, yerr, r, xs = _problem(name, 300)
    nbr = vecchia_local_ref.query_neighbors(x, xs, 12)
    want = vecchia_local_ref.predict(kernel, cross, x, yerr, r, xs, nbr)
    solver = VecchiaSolver(kernel, m=12)
    solver.compute(x, yerr)
    got = solver.predict_local(cross, r, xs, return_var=True)
    _check_pair(case + ":", got, want, _tol(name, 300))
    # through GP.predict(..., kernel=component): its default white noise is on the diagonal too
    gp = GP(kernel, solver=VecchiaSolver, m=12, predict="local")
    gp.compute(x, yerr)
    want = vecchia_local_ref.predict(kernel, cross, x, np.sqrt(yerr ** 2 + george_amd.gp.TINY), r, xs, nbr)
    _check_pair(case + " GP:", gp.predict(r, xs, return_var=True, kernel=cross), want, _tol(name, 300))


def _irregular_query(n, ntest, mq):
    """rows with 0 .. mq entries, far-away points among them, entries not in ascending order, padding in the middle of a row"""
    rng = np.random.RandomState(78)
    tab = np.full((ntest, mq), -1, dtype=np.int32)
    for c in range(ntest):
        k = c % (mq + 1)
        near = (rng.randint(0, n) + np.arange(k // 2)) % n
        far = rng.choice(n, size=k, replace=False)
        pts = np.unique(np.concatenate([near, far]))[:k] if c % 3 else far
        pts = rng.permutation(pts)
        slots = np.sort(rng.choice(mq, size=len(pts), replace=False)) if c % 5 == 0 else np.arange(len(pts))
        tab[c, slots] = pts
    return tab


@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_irregular_table(name):
    """a caller's table, mq = 40 on a solver with m = 24"""
    kernel, x, yerr, r, xs = _problem(name, 777)
    tab = _irregular_query(777, 300, 40)
    counts = (tab >= 0).sum(axis=1)
    assert counts.min() == 0 and counts.max() == 40 and np.any(np.diff(tab, axis=1)[(tab[:, 1:] >= 0) & (tab[:, :-1] >= 0)] < 0)
    assert np.any((tab[:, :-1] < 0) & (tab[:, 1:] >= 0))
    want = vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs, tab)
    solver = VecchiaSolver(kernel, m=24)
    solver.compute(x, yerr)
    got = solver.predict_local(kernel, r, xs, return_var=True, neighbors=tab, m=40)
    _check_pair("irregular:", got, want, _tol(name, 777))
    empty = counts == 0
    assert np.all(got[0][empty] == 0.0) and np.array_equal(got[1][empty], want[1][empty])
    for bad, why in ((tab[:, :39], "shape"), (tab.astype(np.float64), "dtype"), (np.where(tab == tab[40, 0], 777, tab), "range")):
        with pytest.raises(ValueError):
            solver.predict_local(kernel, r, xs, neighbors=bad, m=40)
    dup = tab.copy()
    dup[40, :2] = 5
    with pytest.raises(ValueError, match="twice"):
        solver.predict_local(kernel, r, xs, neighbors=dup, m=40)
    with pytest.raises(ValueError):
        solver.predict_local(kernel, r, xs[:, :1] if xs.shape[1] > 1 else np.zeros((3, 2)))


@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_variance_bounds(name):
    """conditioning on fewer observations: var_local >= the dense variance (BasicSolver's, same device), <= k**, > 0"""
    kernel, x, yerr, r, xs = _problem(name, 777)
    tol = _tol(name, 777)
    dense = BasicSolver(kernel)
    dense.compute(x, yerr)
    var0 = dense.predict(kernel, r, xs, return_var=True)[1]
    solver = VecchiaSolver(kernel, m=16)
    solver.compute(x, yerr)
    kss = kernel.get_value(xs, diag=True)
    for m in (4, 16):
        var = solver.predict_local(kernel, r, xs, return_var=True, m=m)[1]
        print("m=%d: var_local - var_dense in %.3g .. %.3g (allowance %.3g)" % (m, (var - var0).min(), (var - var0).max(), tol["var"] * kss.max()))
        assert np.all(var >= var0 - tol["var"] * kss.max())
        assert np.all(var <= kss + tol["var"] * kss.max()) and np.all(var > 0.0)


def test_through_gp_and_order():
    kernel, x, yerr, y, xs = _problem("expsq_3d", 300)
    tol = _tol("expsq_3d", 300)
    mean, wn = 0.3, np.log(0.02)
    sigma = np.sqrt(yerr ** 2 + np.exp(wn))
    tab = vecchia_local_ref.query_neighbors(x, xs, 16)
    mu0, var0 = vecchia_local_ref.predict(kernel, kernel, x, sigma, y - mean, xs, tab)
    # the caller's points in a random order, the solver told how to put them back
    q = np.random.RandomState(9).permutation(len(x))
    kw = dict(mean=mean, fit_mean=True, white_noise=wn, fit_white_noise=True, solver=VecchiaSolver, m=16, order=np.argsort(q))
    gp = GP(kernel, predict="local", **kw)
    gp.compute(x[q], yerr[q])
    assert isinstance(gp.solver, VecchiaSolver) and gp.solver.predict_mode == "local"
    mu, var = gp.predict(y[q], xs, return_var=True)
    _check_pair("GP:", (mu - mean, var), (mu0, var0), tol)
    _check("GP: mean only", gp.predict(y[q], xs, return_cov=False) - mean, mu0, tol["mu"])
    with pytest.raises(ValueError, match="conditionally independent"):
        gp.predict(y[q], xs)
    with pytest.raises(ValueError, match="conditionally independent"):
        gp.sample_conditional(y[q], xs[:5])
    # a caller's table is in the caller's numbering: solver position p is the caller's point argsort(q)[p]
    caller = np.where(tab >= 0, np.argsort(q)[np.maximum(tab, 0)], -1).astype(np.int32)
    mu2, var2 = gp.solver.predict_local(kernel, y[q] - mean, xs, return_var=True, neighbors=caller)
    assert np.array_equal(mu2 + gp._call_mean(xs), mu) and np.array_equal(var2, var)
    # the default option: today's predict, through Q
    gp0 = GP(kernel, **kw)
    gp0.compute(x[q], yerr[q])
    assert gp0.solver.predict_mode == "global"
    g = vecchia_ref.gaps(kernel, x, yerr, y, xs[:7])[0]
    ref = vecchia_ref.reference(kernel, x, sigma, gp0.solver._default_table(x), r=y - mean)
    gmu, gvar, gcov = ref.predict(kernel, xs[:40])
    mu3, var3 = gp0.predict(y[q], xs[:40], return_var=True)
    _check("default: mean", mu3 - mean, gmu, 1000.0 * max(g["mu"], 4 * EPS))
    _check("default: variance", var3, gvar, 1000.0 * max(g["var"], 4 * EPS))
    _check("default: covariance", gp0.predict(y[q], xs[:40])[1], gcov, 1000.0 * max(g["cov"], 4 * EPS))
    s0 = VecchiaSolver(kernel, m=16, order=np.argsort(q), predict="global")
    s0.compute(x[q], sigma[q])
    mu4, var4, _ = s0.predict(kernel, y[q] - mean, xs[:40], return_var=True)
    assert np.array_equal(mu4 + gp0._call_mean(xs[:40]), mu3) and np.array_equal(var4, var3)


def test_more_workgroups_than_the_chip_holds():
    """M = N = 20 011, 1-D, m = 16: every 97th test point against the restatement; the whole call against two slices of it and
    against a second run, bit for bit"""
    n = 20011
    kernel, x, yerr, r, xs = _problem("m32_1d", n, 250.0, n)
    tol = _tol("m32_1d", n, 250.0, n)
    solver = VecchiaSolver(kernel, m=16)
    solver.compute(x, yerr)
    tab = vecchia_query_neighbors(x, xs, 16)
    mu, var = solver.predict_local(kernel, r, xs, return_var=True, neighbors=tab)
    pick = np.arange(0, n, 97)
    assert np.array_equal(tab[pick], vecchia_local_ref.query_neighbors(x, xs[pick], 16))
    want = vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs[pick], tab[pick])
    _check_pair("M=20011:", (mu[pick], var[pick]), want, tol)
    cut = 7001
    for sl in (slice(0, cut), slice(cut, n)):
        mu_s, var_s = solver.predict_local(kernel, r, xs[sl], return_var=True, neighbors=tab[sl])
        assert np.array_equal(mu_s, mu[sl]) and np.array_equal(var_s, var[sl])
    mu2, var2 = solver.predict_local(kernel, r, xs, return_var=True)          # (the solver's own search this time)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)


def test_native_table_check():
    """the C ABI checks the query table itself, on the host, before anything is launched: GH_ERR_BAD_ARG; the good table then
    gives the same bits as before"""
    kernel, x, yerr, r, xs = _problem("m32_1d", 64, 3.0)
    solver = VecchiaSolver(kernel, m=4)
    solver.compute(x, yerr)
    xs = np.ascontiguousarray(xs[:30])
    good = vecchia_query_neighbors(x, xs, 6)
    mu0, var0 = solver.predict_local(kernel, r, xs, return_var=True, neighbors=good, m=6)
    mu, var = np.empty(30), np.empty(30)

    def call(tab, mq=6):
        return N.lib.gh_vecchia_predict_local(solver._handle, solver._dk.handle, solver._dk.handle, N.ptr(r), N.ptr(xs), 30, N.ptr(tab), mq,
                                              N.ptr(mu), N.ptr(var))

    for i, s, v in ((10, 1, 64), (10, 1, 1000000), (29, 5, -2), (0, 0, -2147483648), (10, 1, good[10, 0])):
        bad = good.copy()
        bad[i, s] = v
        assert call(bad) == N.GH_ERR_BAD_ARG, (i, s, v)
    for mq in (0, 65, -1):
        assert call(good, mq) == N.GH_ERR_BAD_ARG
    assert solver.computed and call(good) == N.GH_OK
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0)
    k2 = george_amd.program.DeviceKernel(0.9 * kernels.ExpSquaredKernel([0.3, 0.5], ndim=2))
    rc = N.lib.gh_vecchia_predict_local(solver._handle, solver._dk.handle, k2.handle, N.ptr(r), N.ptr(xs), 30, N.ptr(good), 6, N.ptr(mu), None)
    assert rc == N.GH_ERR_DIM
    rc = N.lib.gh_vecchia_predict_local(solver._handle, k2.handle, solver._dk.handle, N.ptr(r), N.ptr(xs), 30, N.ptr(good), 6, N.ptr(mu), None)
    assert rc == N.GH_ERR_DIM
    assert solver.computed and call(good) == N.GH_OK and np.array_equal(mu, mu0)


def test_not_positive_definite_is_an_error_return():
    """Two identical data points without error bars in one conditioning set: with unit amplitude the second pivot of K_cc is
    1 - 1 * 1, an exact zero in any arithmetic.  compute() never pairs them (an empty table)."""
    kernel = 1.0 * kernels.ExpSquaredKernel(1.0)
    x = np.linspace(0, 4, 40)[:, None]
    x[23] = x[20]
    solver = VecchiaSolver(kernel, m=2, neighbors=np.full((40, 2), -1, dtype=np.int32))
    solver.compute(x, 0.0)
    assert solver.computed
    r = np.sin(x[:, 0])
    xs = np.linspace(0.05, 3.95, 6)[:, None]
    tab = np.array([[0, 1], [7, -1], [-1, 12], [20, 23], [30, 31], [38, 39]], dtype=np.int32)
    with pytest.raises(np.linalg.LinAlgError):
        solver.predict_local(kernel, r, xs, return_var=True, neighbors=tab)
    assert solver.failed_test_point == 3 and solver.computed and solver.failed_point is None
    # an error return, not a fault: the same solver answers a valid call afterwards.  (Pairs at least 4 / 39 apart: the
    # condition number of a K_cc is at most 2 / (1 - exp(-0.0052)) = 4e2, so float64 routes agree to ~ 1e-13; 1000 times that.)
    tab[3] = [20, 24]
    mu, var = solver.predict_local(kernel, r, xs, return_var=True, neighbors=tab)
    assert solver.failed_test_point is None
    want = vecchia_local_ref.predict(kernel, kernel, x, 0.0, r, xs, tab)
    _check_pair("after the error:", (mu, var), want, dict(mu=1e-10, var=1e-10))
    assert np.isfinite(solver.dot_solve(r))
