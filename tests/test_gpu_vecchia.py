"""``VecchiaSolver`` on the device (george_amd/csrc/gh_vecchia.hip) against the dense device solver where every predecessor is
in the conditioning set, and against the NumPy restatement (tests/vecchia_ref.py) everywhere else.

Tolerances.  For each compared quantity the bound is ``1000 x`` the gap that two float64 routes on the CPU -- the restatement
and dense LAPACK -- show with every predecessor in the conditioning set (``vecchia_ref.gaps``), on the test's own inputs.  The
restatement at ``m = N - 1`` costs O(N^4), so beyond 300 points the gap is taken on the first 300 points of the same inputs
(sorted inputs: the same point density and the same error bars, which is what sets the conditioning of a block and with it the
rounding; N only adds terms of random sign).  The margin of 1000 covers the device ``exp`` / ``sqrt`` differing from libm by a
few ulp and the reordered sums.  Two routes can agree to the last bit by chance, and the comparison itself resolves no better
than a few ulp of the scale, so a gap counts as at least ``4 eps``.  No bound is looser than the project's dense-parity bounds:
1e-10 relative on the log-determinant, 1e-9 on the log-likelihood and on ``dot_solve``.  Vectors and matrices are measured over
their largest absolute entry, gradients over the restatement's sum of absolute terms.  Error bars are at least 0.1 of the kernel
amplitude, so every block is well conditioned (gaps observed on the CPU: 1e-16 .. 4e-13, and up to 8e-12 for the
hyper.rst kernel, whose amplitudes span five orders of magnitude; every test prints them).
"""
import functools

import numpy as np
import pytest

import george_amd
from george_amd import GP, BasicSolver, VecchiaSolver, kernels
from george_amd.solvers.vecchia import vecchia_neighbors

import loo_ref
import vecchia_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
CAPS = {"logdet": 1e-10, "quad": 1e-9, "ll": 1e-9}
GAP_MAX_N = 300


def _kernel(name):
    if name == "m32_1d":
        return 1.7 * kernels.Matern32Kernel(0.8), 1, np.sqrt(1.7)
    if name == "expsq_2d":
        return 0.9 * kernels.ExpSquaredKernel([0.3, 0.5], ndim=2), 2, np.sqrt(0.9)
    if name == "expsq_3d":
        return 0.8 * kernels.ExpSquaredKernel([0.4, 0.6, 0.9], ndim=3), 3, np.sqrt(0.8)
    return loo_ref.kernel_hyper(), 1, 66.0


@functools.lru_cache(maxsize=None)
def _problem(name, n, span=10.0):
    """(kernel, x, yerr, r, xs): inputs sorted by their first column, error bars 0.1 .. 0.15 of the amplitude, 300 test points"""
    kernel, ndim, amp = _kernel(name)
    rng = np.random.RandomState(1000 * ndim + n)
    x = np.sort(rng.uniform(0, span, n))[:, None] if ndim == 1 else rng.uniform(0, 2, (n, ndim))
    x = x[np.argsort(x[:, 0], kind="stable")]
    yerr = amp * (0.1 + 0.05 * rng.rand(n))
    r = amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))
    xs = rng.uniform(0, span if ndim == 1 else 2, (300, ndim))
    return kernel, x, yerr, r, xs


@functools.lru_cache(maxsize=None)
def _tol(name, n, span=10.0):
    kernel, x, yerr, r, xs = _problem(name, n, span)
    k = min(n, GAP_MAX_N)
    g = vecchia_ref.gaps(kernel, x[:k], yerr[:k], r[:k], xs[:7])[0]
    g["ll"] = g["quad"]
    tol = {key: min(1000.0 * max(v, 4 * EPS), CAPS.get(key, np.inf)) for key, v in g.items()}
    print("gaps", name, n, g)
    return tol


@functools.lru_cache(maxsize=None)
def _ref(name, n, m, table="default", span=10.0):
    kernel, x, yerr, r, xs = _problem(name, n, span)
    nbr = vecchia_neighbors(x, m) if table == "default" else _irregular_table(n, m)
    return vecchia_ref.reference(kernel, x, yerr, nbr, r=r, want_grad=True), nbr


def _irregular_table(n, m):
    """rows with 0 .. m neighbours, far-away ones among them, entries not in ascending order, padding in the middle of a row"""
    rng = np.random.RandomState(77)
    tab = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        k = min(i, rng.randint(0, m + 1))
        near = np.arange(max(0, i - k // 2), i)
        far = rng.choice(i, size=k, replace=False)
        c = np.unique(np.concatenate([near, far]))[:k] if i % 3 else far
        c = rng.permutation(c)
        slots = np.sort(rng.choice(m, size=len(c), replace=False)) if i % 5 == 0 else np.arange(len(c))
        tab[i, slots] = c
    return tab


def _check(what, got, want, tol, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.max(np.abs(want)) if scale is None else scale
    err = np.max(np.abs(got - want) / scale)
    print("%-22s error %.3g  bound %.3g" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _compare(solver, kernel, r, xs, want, tol, nrhs_list=(1, 3, 130), m_list=(1, 5, 300)):
    """every call of the solver against ``want``: dict(logdet, quad, apply (matrix -> Q matrix), kgrad, S, alpha, diagA,
    predict (xs -> mu, var, cov))"""
    n = len(r)
    _check("log_determinant", solver.log_determinant, want["logdet"], tol["logdet"])
    _check("dot_solve", solver.dot_solve(r), want["quad"], tol["quad"])
    rng = np.random.RandomState(5)
    for nrhs in nrhs_list:
        Y = r.copy() if nrhs == 1 else np.column_stack([r] + [rng.randn(n) for _ in range(nrhs - 1)])
        ref_out = want["apply"](Y)
        _check("apply_inverse nrhs=%d" % nrhs, solver.apply_inverse(Y), ref_out, tol["alpha"])
        Yc = Y.copy()
        out = solver.apply_inverse(Yc, in_place=True)
        _check("  .. in_place", out, ref_out, tol["alpha"])
        assert np.array_equal(out, solver.apply_inverse(Y))
    which = np.ones(len(kernel), dtype=np.uint32)
    g, alpha, diagA = solver.grad(r, which)
    _check("grad: kernel", g, want["kgrad"], tol["kgrad"], scale=want["S"])
    _check("grad: alpha", alpha, want["alpha"], tol["alpha"])
    _check("grad: diagA", diagA, want["diagA"], tol["diagA"])
    if len(which) > 1:
        which[0] = 0
        g0 = solver.grad(r, which)[0]
        assert g0[0] == 0.0 and np.array_equal(g0[1:], g[1:])
    for mm in m_list:
        mu0, var0, cov0 = want["predict"](xs[:mm])
        mu, var, _ = solver.predict(kernel, r, xs[:mm], return_var=True)
        _check("predict M=%d: mean" % mm, mu, mu0, tol["mu"])
        _check("  .. variance", var, var0, tol["var"])
        mu2, _, cov = solver.predict(kernel, r, xs[:mm], return_cov=True)
        _check("  .. covariance", cov, cov0, tol["cov"])
        assert np.array_equal(mu2, mu)


def _want_from_ref(ref, kernel):
    return dict(logdet=ref.logdet, quad=ref.quad, apply=ref.apply_q, kgrad=ref.kgrad, S=ref.S, alpha=ref.alpha, diagA=ref.diagA,
                predict=lambda t: ref.predict(kernel, t))


@pytest.mark.parametrize("name", ["m32_1d", "expsq_2d"])
def test_exact_case_against_the_dense_solver(name):
    """N = 65, m = 64: every predecessor is used, so the answers are the dense ones -- BasicSolver's, on the same device"""
    kernel, x, yerr, r, xs = _problem(name, 65, 3.0)
    tol = _tol(name, 65, 3.0)
    dense = BasicSolver(kernel)
    dense.compute(x, yerr)
    which = np.ones(len(kernel), dtype=np.uint32)
    kg, alpha, diagA = dense.grad(r, which)
    S = vecchia_ref.dense(kernel, x, yerr, r)["S"]

    def predict(t):
        mu, var, _ = dense.predict(kernel, r, t, return_var=True)
        return mu, var, dense.predict(kernel, r, t, return_cov=True)[2]

    want = dict(logdet=dense.log_determinant, quad=dense.dot_solve(r), apply=dense.apply_inverse, kgrad=kg, S=S, alpha=alpha,
                diagA=diagA, predict=predict)
    solver = VecchiaSolver(kernel, m=64)
    solver.compute(x, yerr)
    _compare(solver, kernel, r, xs, want, tol, nrhs_list=(1, 3), m_list=(1, 5, 300))
    _check("get_inverse", solver.get_inverse(), dense.get_inverse(), tol["Kinv"])


@pytest.mark.parametrize("m", [1, 7, 32, 64])
@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_parity_with_the_restatement(name, m):
    """N = 777: no multiple of any launch size, and the first m rows have short neighbour lists"""
    kernel, x, yerr, r, xs = _problem(name, 777)
    ref, nbr = _ref(name, 777, m)
    solver = VecchiaSolver(kernel, m=m)
    solver.compute(x, yerr)
    _compare(solver, kernel, r, xs, _want_from_ref(ref, kernel), _tol(name, 777))


@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_irregular_table(name):
    kernel, x, yerr, r, xs = _problem(name, 777)
    ref, nbr = _ref(name, 777, 24, table="irregular")
    counts = (nbr >= 0).sum(axis=1)
    assert counts.min() == 0 and counts.max() == 24 and np.any(np.diff(nbr, axis=1)[(nbr[:, 1:] >= 0) & (nbr[:, :-1] >= 0)] < 0)
    solver = VecchiaSolver(kernel, m=24, neighbors=nbr)
    solver.compute(x, yerr)
    _compare(solver, kernel, r, xs, _want_from_ref(ref, kernel), _tol(name, 777), nrhs_list=(1, 3), m_list=(5,))


def test_interpreter_path():
    """the 17-node composite of docs/tutorials/hyper.rst (tests/loo_ref.py): no fast form, eleven gradient slots"""
    kernel, x, yerr, r, xs = _problem("hyper", 300)
    assert len(kernel) == 11
    ref, nbr = _ref("hyper", 300, 16)
    solver = VecchiaSolver(kernel, m=16)
    solver.compute(x, yerr)
    _compare(solver, kernel, r, xs, _want_from_ref(ref, kernel), _tol("hyper", 300), nrhs_list=(1, 3), m_list=(5,))


def test_through_gp_and_order():
    kernel, x, yerr, y, xs = _problem("expsq_3d", 500)
    tol = _tol("expsq_3d", 500)
    mean, wn = 0.3, np.log(0.02)
    sigma = np.sqrt(yerr ** 2 + np.exp(wn))
    nbr = vecchia_neighbors(x, 16)
    ref = vecchia_ref.reference(kernel, x, sigma, nbr, r=y - mean, want_grad=True)
    grad0 = np.concatenate([[np.sum(ref.alpha)], [0.5 * np.exp(wn) * np.sum(ref.diagA)], ref.kgrad])
    S = np.concatenate([[np.sum(np.abs(ref.alpha))], [0.5 * np.exp(wn) * np.sum(np.abs(ref.diagA))], ref.S])
    mu0, var0, cov0 = ref.predict(kernel, xs[:40])

    def check(gp, yy, tag):
        assert len(gp) == 2 + len(kernel)
        _check(tag + "log_likelihood", gp.log_likelihood(yy), ref.log_likelihood(), tol["ll"])
        _check(tag + "grad_log_likelihood", gp.grad_log_likelihood(yy), grad0, max(tol["kgrad"], tol["alpha"], tol["diagA"]), scale=S)
        mu, var = gp.predict(yy, xs[:40], return_var=True)
        _check(tag + "predict mean", mu, mu0 + mean, tol["mu"])
        _check(tag + "predict variance", var, var0, tol["var"])
        _check(tag + "predict covariance", gp.predict(yy, xs[:40])[1], cov0, tol["cov"])

    gp = GP(kernel, mean=mean, fit_mean=True, white_noise=wn, fit_white_noise=True, solver=VecchiaSolver, m=16)
    gp.compute(x, yerr)
    assert isinstance(gp.solver, VecchiaSolver)
    check(gp, y, "")
    _check("apply_inverse", gp.apply_inverse(y), ref.alpha, tol["alpha"])
    # the caller's points in a random order, the solver told how to put them back: results in the caller's order
    q = np.random.RandomState(9).permutation(len(x))
    gp2 = GP(kernel, mean=mean, fit_mean=True, white_noise=wn, fit_white_noise=True, solver=VecchiaSolver, m=16, order=np.argsort(q))
    gp2.compute(x[q], yerr[q])
    check(gp2, y[q], "order: ")
    _check("order: apply_inverse", gp2.apply_inverse(y[q]), ref.alpha[q], tol["alpha"])
    g, alpha, diagA = gp2.solver.grad(y[q] - mean, np.ones(len(kernel), dtype=np.uint32))
    _check("order: alpha", alpha, ref.alpha[q], tol["alpha"])
    _check("order: diagA", diagA, ref.diagA[q], tol["diagA"])
    # "coordinate": a stable argsort of the first column -- here the sorted order again
    s3 = VecchiaSolver(kernel, m=16, order="coordinate")
    s3.compute(x[q], sigma[q])
    _check("coordinate: log_determinant", s3.log_determinant, ref.logdet, tol["logdet"])
    _check("coordinate: alpha", s3.apply_inverse(y[q] - mean), ref.alpha[q], tol["alpha"])


def test_more_workgroups_than_the_chip_holds():
    """N = 20 011, 1-D, m = 32: log-likelihood and gradient"""
    n = 20011
    kernel, x, yerr, r, xs = _problem("m32_1d", n, 250.0)
    tol = _tol("m32_1d", n, 250.0)
    ref, nbr = _ref("m32_1d", n, 32, span=250.0)
    solver = VecchiaSolver(kernel, m=32)
    solver.compute(x, yerr)
    _check("log_determinant", solver.log_determinant, ref.logdet, tol["logdet"])
    ll = -0.5 * (solver.dot_solve(r) + solver.log_determinant + n * np.log(2 * np.pi))
    _check("log_likelihood", ll, ref.log_likelihood(), tol["ll"])
    g, alpha, diagA = solver.grad(r, np.ones(len(kernel), dtype=np.uint32))
    _check("grad: kernel", g, ref.kgrad, tol["kgrad"], scale=ref.S)
    _check("grad: alpha", alpha, ref.alpha, tol["alpha"])
    _check("grad: diagA", diagA, ref.diagA, tol["diagA"])


def test_predict_strips():
    """N = 700, 3-D, m = 32, 600 test points: without a covariance predict walks them in strips of 256 + 256 + 88, and the column
    sums over 6 chunks of 117 rows, the last one short.  A column's value depends on no other column -- not in the forward
    operator, not in the sums -- and a strip only changes the row pitch: every prefix of the test points gives the bits of the full
    call, mean and variance alike, with or without the variance.  The covariance goes through the GEMM: to tolerance."""
    kernel, x, yerr, r, _ = _problem("expsq_3d", 700)
    tol = _tol("expsq_3d", 700)
    t = np.random.RandomState(600).uniform(0, 2, (600, 3))
    solver = VecchiaSolver(kernel, m=32)
    solver.compute(x, yerr)
    mu, var, _ = solver.predict(kernel, r, t, return_var=True)
    cov = solver.predict(kernel, r, t, return_cov=True)[2]
    for k in (1, 255, 256, 257, 512, 513, 600):
        mu_k, var_k, _ = solver.predict(kernel, r, t[:k], return_var=True)
        assert np.array_equal(mu_k, mu[:k]) and np.array_equal(var_k, var[:k]), k
        mu_m, var_m, _ = solver.predict(kernel, r, t[:k])
        assert np.array_equal(mu_m, mu[:k]) and var_m is None, k
        if k < 600:
            _check("predict M=%d: covariance" % k, solver.predict(kernel, r, t[:k], return_cov=True)[2], cov[:k, :k], tol["cov"])


def test_two_runs_give_the_same_bits():
    kernel, x, yerr, r, xs = _problem("expsq_3d", 777)
    which = np.ones(len(kernel), dtype=np.uint32)
    runs = []
    for _ in range(2):
        solver = VecchiaSolver(kernel, m=32)
        solver.compute(x, yerr)
        runs.append((np.array([solver.log_determinant, solver.dot_solve(r)]),) + solver.grad(r, which) + (solver.apply_inverse(r),))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_native_table_check():
    """the C ABI checks the table itself, on the host, before anything is launched: GH_ERR_BAD_ARG; the good table then computes
    the same bits as before"""
    import ctypes
    from george_amd import _native as N
    kernel, x, yerr, r, xs = _problem("m32_1d", 65, 3.0)
    solver = VecchiaSolver(kernel, m=4)
    solver.compute(x, yerr)
    quad = solver.dot_solve(r)
    good = vecchia_neighbors(x, 4)
    logdet = ctypes.c_double(0.0)
    for i, s, v in ((10, 1, 10), (10, 1, 64), (10, 1, -2), (10, 1, good[10, 0]), (0, 0, 0)):
        bad = good.copy()
        bad[i, s] = v
        rc = N.lib.gh_vecchia_compute(solver._handle, solver._dk.handle, N.ptr(x), 65, 1, N.ptr(yerr), N.ptr(bad), ctypes.byref(logdet))
        assert rc == N.GH_ERR_BAD_ARG, (i, s, v)
    rc = N.lib.gh_vecchia_compute(solver._handle, solver._dk.handle, N.ptr(x), 65, 1, N.ptr(yerr), N.ptr(good), ctypes.byref(logdet))
    assert rc == N.GH_OK and logdet.value == solver.log_determinant and solver.dot_solve(r) == quad


def test_not_positive_definite_is_an_error_return():
    """Two identical points without error bars: the conditional of the later one has no variance left.  With m = 1 and unit
    amplitude its f is 1 - 1 * 1, an exact zero in any arithmetic (with more neighbours it is a rounding residue of either sign)."""
    kernel = 1.0 * kernels.ExpSquaredKernel(1.0)
    x = np.linspace(0, 4, 40)[:, None]
    x[23] = x[20]
    solver = VecchiaSolver(kernel, m=1)
    with pytest.raises(np.linalg.LinAlgError):
        solver.compute(x, 0.0)
    assert solver.failed_point == 23 and not solver.computed
    # ... in the caller's numbering when the solver reorders: in the reversed order point 20 comes after point 23
    s2 = VecchiaSolver(kernel, m=1, order=np.arange(40)[::-1].copy())
    with pytest.raises(np.linalg.LinAlgError):
        s2.compute(x, 0.0)
    assert s2.failed_point == 20 and not s2.computed
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        s2.dot_solve(np.zeros(40))
    # a pivot that is not finite: the lowest point it reaches is reported
    yerr = 0.1 * np.ones(40)
    yerr[5] = np.nan
    s3 = VecchiaSolver(kernel, m=8)
    with pytest.raises(np.linalg.LinAlgError):
        s3.compute(x, yerr)
    assert s3.failed_point == 5
    # error returns, not faults: the same solvers compute afterwards
    for s in (solver, s3):
        s.compute(x, 0.1)
        assert s.computed and np.isfinite(s.log_determinant)
    assert george_amd.device_count() > 0
