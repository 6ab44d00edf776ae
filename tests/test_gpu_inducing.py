"""``InducingSolver`` on the device (george_amd/csrc/gh_inducing.hip) against the NumPy restatement (tests/inducing_ref.py).

Tolerances.  For each compared quantity the bound is ``1000 x`` the gap that two float64 routes on the CPU -- the restatement
and ``inducing_ref.dense_model``, LAPACK on the explicit N x N matrix ``C`` -- show on the test's own inputs, inducing points
and jitter (``inducing_ref.gaps``); beyond 800 points the gap is taken on the first 800 points with the same inducing points,
which is what sets the conditioning.  The margin of 1000 covers the device ``exp`` / ``sqrt`` differing from libm by a few ulp,
the reordered sums, and the explicit triangular inverses the device multiplies by where the restatement substitutes.  Two routes
can agree to the last bit by chance, and the comparison itself resolves no better than a few ulp of the scale, so a gap counts as
at least ``4 eps``.  No bound is looser than the project's dense-parity bounds: 1e-10 relative on the log-determinant, 1e-9 on the
log-likelihood and on ``dot_solve``.  Vectors and matrices are measured over their largest absolute entry, gradients over the
restatement's sum of absolute terms ``S``.

The cap on conditioning.  The gap grows with the conditioning of ``K_uu + jitter I``, so kernels and jitter are chosen such that no
gap exceeds 1e-9 of its scale (``_setup`` asserts it): Matern-3/2 with the default relative jitter 1e-10, and ExpSquared in 1-D
with relative jitter 1e-8.  Measured on the CPU at N = 777 (every test prints its own): Matern-3/2 in 3-D, m = 129 / 300:
1e-16 .. 3e-13; the Sum / Product kernel at m = 300: 2e-16 .. 3e-13; ExpSquared in 1-D, m = 60, cond(K_uu) 1e8: 1e-16 .. 4e-12
(the covariance).  The device differed from the restatement by 1e-16 .. 7e-12 on these.
"""
import ctypes
import functools

import numpy as np
import pytest

import george_amd
from george_amd import GP, BasicSolver, InducingSolver, kernels
from george_amd import _native as N
from george_amd.solvers.inducing import inducing_points

import inducing_ref
import vecchia_ref
from inducing_cases import GAP_CAP, GAP_MAX_N, JITTER, _check, _check_grad, _check_predict, _problem, tolerances
from oracle import solver_np

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _setup(name, n, m, method, inducing="maxmin"):
    """(u, relative jitter, absolute jitter, the restatement with its gradient, tolerances)"""
    kernel, x, yerr, r, xs = _problem(name, n)
    if inducing == "maxmin":
        u = np.ascontiguousarray(x[inducing_points(x, m)])
    elif inducing == "x":
        u = x
    else:                                                   # inducing inputs that are no data points
        u = np.random.RandomState(m).uniform(0, 10 if x.shape[1] == 1 else 2, (m, x.shape[1]))
    rel_jitter = 0.0 if inducing == "x" else JITTER.get(name, 1e-10)
    jitter = rel_jitter * float(np.mean(solver_np.kernel_matrix(kernel, u, diag=True)))
    ref = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=n <= GAP_MAX_N)
    k = min(n, GAP_MAX_N)
    g = inducing_ref.gaps(kernel, x[:k], yerr[:k], u, jitter, method, r[:k], xs[:7])[0]
    g["ll"] = g["quad"]
    print("gaps", name, n, m, method, {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    tol = tolerances(g)
    return u, rel_jitter, jitter, ref, tol


def _solver(name, n, m, method, strip, inducing="maxmin"):
    kernel, x, yerr, r, xs = _problem(name, n)
    u, rel_jitter = _setup(name, n, m, method, inducing)[:2]
    s = InducingSolver(kernel, inducing=u, method=method, jitter=rel_jitter, strip_points=strip)
    s.compute(x, yerr)
    return s


CASES = [("m32_3d", 1, "fitc"), ("m32_3d", 127, "fitc"), ("m32_3d", 128, "dtc"), ("m32_3d", 129, "fitc"), ("m32_3d", 129, "dtc"),
         ("m32_3d", 300, "fitc"), ("comp_3d", 129, "fitc"), ("comp_3d", 300, "dtc"), ("m32_1d", 129, "fitc"), ("expsq_1d", 60, "dtc"),
         ("expsq_1d", 60, "fitc")]


@pytest.mark.parametrize("name,m,method", CASES)
def test_against_the_restatement(name, m, method):
    """N = 777 in strips of 256 points (four strips, the last one ragged; test points in two strips) and in one automatic
    strip: every protocol call against the restatement, and the two runs against each other."""
    n = 777
    kernel, x, yerr, r, xs = _problem(name, n)
    u, _, _, ref, tol = _setup(name, n, m, method)
    s = _solver(name, n, m, method, 256)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    rng = np.random.RandomState(5)
    for nrhs in (1, 5):
        Y = r.copy() if nrhs == 1 else np.column_stack([r] + [rng.randn(n) for _ in range(nrhs - 1)])
        want = ref.solve(Y)
        _check("apply_inverse nrhs=%d" % nrhs, s.apply_inverse(Y), want, tol["alpha"])
        Yc = Y.copy()
        out = s.apply_inverse(Yc, in_place=True)
        assert out is Yc and np.array_equal(out, s.apply_inverse(Y))
    g, alpha, diagA = _check_grad(s, kernel, r, ref, tol)
    mu, var = _check_predict(s, kernel, r, xs, ref, tol, (1, 300))
    mu0, _, cov0 = ref.predict(kernel, xs[:130])
    mu2, var2, cov = s.predict(kernel, r, xs[:130], return_cov=True)
    assert var2 is None and np.array_equal(mu2, mu[:130])
    _check("predict M=130: covariance", cov, cov0, tol["cov"])
    # one strip
    t = _solver(name, n, m, method, 0)
    _check("one strip: log_determinant", t.log_determinant, ref.logdet, tol["logdet"])
    _check("  .. against four strips", t.log_determinant, s.log_determinant, tol["logdet"])
    _check("one strip: dot_solve", t.dot_solve(r), ref.quad, tol["quad"])
    g1, alpha1, diagA1 = _check_grad(t, kernel, r, ref, tol)
    mask = kernel.unfrozen_mask
    _check("  .. against four strips", g1[mask], g[mask], tol["kgrad"], scale=ref.S[mask])
    _check("  .. alpha", alpha1, alpha, tol["alpha"])
    _check("  .. diagA", diagA1, diagA, tol["diagA"])
    mu1, var1 = _check_predict(t, kernel, r, xs, ref, tol, (300,))
    _check("  .. against two strips", mu1, mu, tol["mu"])
    _check("  .. variance", var1, var, tol["var"])


@pytest.mark.parametrize("n,m,inducing", [(1, 1, "x"), (100, 129, "random")])
@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_fewer_points_than_a_tile(n, m, inducing, method):
    """N = 1 (its own inducing point), and N = 100 data points under m = 129 inducing inputs that are no data points"""
    kernel, x, yerr, r, xs = _problem("m32_3d", n)
    ref, tol = _setup("m32_3d", n, m, method, inducing)[3:]
    s = _solver("m32_3d", n, m, method, 0, inducing)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    _check("apply_inverse", s.apply_inverse(r), ref.alpha, tol["alpha"])
    _check_grad(s, kernel, r, ref, tol)
    _check_predict(s, kernel, r, xs, ref, tol, (1, 130))
    _check("get_inverse", s.get_inverse(), ref.solve(np.eye(n)), tol["Cinv"])


@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_every_point_an_inducing_point_is_the_dense_solver(method):
    """u = x, jitter = 0, N = m = 300 in 3-D: both methods ARE the dense GP, here the dense solver of the same build.  The
    bound: 1000 x the gap between the restatement at u = x and dense LAPACK."""
    n = 300
    kernel, x, yerr, r, xs = _problem("m32_3d", n)
    ref = inducing_ref.reference(kernel, x, yerr, x, 0.0, method, r=r, want_grad=True)
    d = vecchia_ref.dense(kernel, x, yerr, r, xs)
    g = dict(logdet=inducing_ref.rel(ref.logdet, d["logdet"]), quad=inducing_ref.rel(ref.quad, d["quad"]),
             alpha=inducing_ref.rel(ref.alpha, d["alpha"]), diagA=inducing_ref.rel(ref.diagA, d["diagA"]),
             kgrad=float(np.max(np.abs(ref.kgrad - d["kgrad"]) / d["S"])), mu=inducing_ref.rel(ref.predict(kernel, xs)[0], d["mu"]),
             var=inducing_ref.rel(ref.predict(kernel, xs)[1], d["var"]))
    print("gaps", g)
    tol = tolerances(g)
    s = InducingSolver(kernel, inducing=x, method=method, jitter=0.0)
    s.compute(x, yerr)
    b = BasicSolver(kernel)
    b.compute(x, yerr)
    _check("log_determinant", s.log_determinant, b.log_determinant, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), b.dot_solve(r), tol["quad"])
    _check("apply_inverse", s.apply_inverse(r), b.apply_inverse(r), tol["alpha"])
    which = np.ones(len(kernel), dtype=np.uint32)
    gs, gb = s.grad(r, which), b.grad(r, which)
    _check("grad: kernel", gs[0], gb[0], tol["kgrad"], scale=d["S"])
    _check("grad: alpha", gs[1], gb[1], tol["alpha"])
    _check("grad: diagA", gs[2], gb[2], tol["diagA"])
    ps, pb = s.predict(kernel, r, xs, return_var=True), b.predict(kernel, r, xs, return_var=True)
    _check("predict: mean", ps[0], pb[0], tol["mu"])
    _check("predict: variance", ps[1], pb[1], tol["var"])


@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_through_gp(method):
    """``GP(kernel, solver=InducingSolver, ...)`` through the solver protocol alone: the gradient of ``nll_and_grad`` -- constant
    mean, white noise and kernel parameters -- against central differences of ``GP.log_likelihood`` (step 1e-5: a truncation
    error of 1e-10 and a rounding error of eps |ll| / h = 1e-8 of the scale, bound 1e-6), and ``predict`` /
    ``sample_conditional`` through ``return_cov``."""
    kernel, x, yerr, r, xs = _problem("m32_3d", 777)
    y = r + 0.2
    gp = GP(kernel, solver=InducingSolver, inducing=100, method=method, mean=0.2, fit_mean=True, white_noise=np.log(0.01),
            fit_white_noise=True)
    gp.compute(x, yerr)
    assert isinstance(gp.solver, InducingSolver) and len(gp.solver.u) == 100
    p0 = gp.get_parameter_vector()
    assert len(p0) == 2 + len(kernel)
    try:
        nll, grad = gp.nll_and_grad(p0, y)
        assert abs(nll + gp.log_likelihood(y)) <= 1e-12 * abs(nll)
        assert np.array_equal(-grad, gp.grad_log_likelihood(y))
        for a in range(len(p0)):
            h = 1e-5 * max(1.0, abs(p0[a]))
            up, dn = p0.copy(), p0.copy()
            up[a] += h
            dn[a] -= h
            fd = (gp.nll(up, y) - gp.nll(dn, y)) / (2 * h)
            print("parameter %d: gradient %.10g  central difference %.10g" % (a, grad[a], fd))
            assert abs(fd - grad[a]) <= 1e-6 * max(1.0, abs(grad[a])), (a, fd, grad[a])
    finally:
        gp.set_parameter_vector(p0)
    gp.compute(x, yerr)
    mu, cov = gp.predict(y, xs[:40], return_cov=True)
    mu2, var = gp.predict(y, xs[:40], return_var=True)
    assert np.array_equal(mu, mu2) and np.allclose(np.diag(cov), var, rtol=0, atol=1e-10 * np.max(np.abs(cov)))
    draws = gp.sample_conditional(y, xs[:40], size=3)
    assert draws.shape == (3, 40) and np.all(np.isfinite(draws))


@pytest.mark.parametrize("name,method", [("m32_3d", "fitc"), ("comp_3d", "dtc")])
def test_two_calls_give_identical_bits(name, method):
    kernel, x, yerr, r, xs = _problem(name, 777)
    which = kernel.unfrozen_mask.astype(np.uint32)
    runs = []
    for _ in range(2):
        s = _solver(name, 777, 129, method, 256)
        runs.append([np.float64(s.log_determinant), np.float64(s.dot_solve(r)), s.apply_inverse(r)] + list(s.grad(r, which)) +
                    list(s.predict(kernel, r, xs, return_var=True)[:2]) + [s.predict(kernel, r, xs[:130], return_cov=True)[2]])
        runs.append(runs[-1][:3] + list(s.grad(r, which)) + list(s.predict(kernel, r, xs, return_var=True)[:2]) + [runs[-1][-1]])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


def test_a_factor_that_is_not_positive_definite():
    """A duplicated inducing point with jitter = 0: K_uu = [[1, 1], [1, 1]] exactly (the unit-amplitude kernel at distance 0), so
    the second pivot is exactly 0.  The error return of a numerical failure: ``info`` names factor and pivot, the solver stays
    uncomputed, and the handle serves the next compute."""
    kernel = kernels.ExpSquaredKernel(0.5)
    x = np.linspace(0, 3, 40)[:, None]
    s = InducingSolver(kernel, inducing=np.array([[0.3], [0.3]]), jitter=0.0)
    with pytest.raises(np.linalg.LinAlgError, match="K_uu"):
        s.compute(x, 0.1)
    assert not s.computed and (s.failed_factor, s.failed_pivot) == ("K_uu", 1)
    assert N.lib.gh_inducing_info(s._handle) == 2
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        s.dot_solve(np.zeros(40))
    logdet = ctypes.c_double(0.0)
    u = np.array([[0.3], [1.7]])
    yerr = 0.1 * np.ones(40)
    assert N.lib.gh_inducing_compute(s._handle, s._dk.handle, N.ptr(x), 40, 1, N.ptr(yerr), N.ptr(u), 2, 0.0, ctypes.byref(logdet)) == N.GH_OK
    assert N.lib.gh_inducing_info(s._handle) == 0
    ref = inducing_ref.reference(kernel, x, yerr, u, 0.0, "fitc")
    assert abs(logdet.value - ref.logdet) <= 1e-10 * abs(ref.logdet)
    # the same with a jitter: positive definite
    t = InducingSolver(kernel, inducing=np.array([[0.3], [0.3]]), jitter=1e-6)
    t.compute(x, 0.1)
    assert t.computed and np.isfinite(t.log_determinant)


def test_a_moderate_problem():
    """N = 20 011 (strips and tiles ragged everywhere), m = 512 max-min points in 3-D: the log-likelihood and 100 predictions"""
    n, m = 20011, 512
    kernel, x, yerr, r, xs = _problem("m32_3d", n)
    u, rel_jitter, _, ref, tol = _setup("m32_3d", n, m, "fitc")
    s = InducingSolver(kernel, inducing=m, method="fitc", jitter=rel_jitter, strip_points=8192)
    s.compute(x, yerr)
    assert np.array_equal(s.u, u)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    ll = -0.5 * (s.dot_solve(r) + s.log_determinant + n * np.log(2 * np.pi))
    _check("log-likelihood", ll, ref.log_likelihood(), tol["ll"])
    mu0, var0, cov0 = ref.predict(kernel, xs[:100])
    mu, var, _ = s.predict(kernel, r, xs[:100], return_var=True)
    _check("predict: mean", mu, mu0, tol["mu"])
    _check("  .. variance", var, var0, tol["var"])


def test_device_pointers_give_the_host_route_bits():
    """Every array argument of the ABI as host memory, as device memory (also at an odd element offset) and mixed: the same
    status and the same bits, nothing written outside an output (tests/devptr.py)."""
    import devptr
    n, m = 777, 129
    kernel, x, yerr, r, xs = _problem("m32_3d", n)
    u, _, jitter = _setup("m32_3d", n, m, "fitc")[:3]
    s = _solver("m32_3d", n, m, "fitc", 256)
    h, k = s._handle, s._dk.handle
    logdets = []

    def compute(p):
        logdet = ctypes.c_double(0.0)
        rc = N.lib.gh_inducing_compute(h, k, p["x"], n, 3, p["yerr"], p["u"], m, jitter, ctypes.byref(logdet))
        logdets.append(logdet.value)
        return rc

    res = devptr.check_routes("gh_inducing_compute", compute, dict(x=x, yerr=yerr, u=u), {}, odd=("x", "yerr", "u"))
    assert res["host"][0] == N.GH_OK and len(set(logdets)) == 1 and logdets[0] == s.log_determinant
    B = np.column_stack([r, np.random.RandomState(5).randn(n, 2)])
    res = devptr.check_routes("gh_inducing_solve", lambda p: N.lib.gh_inducing_solve(h, p["b"], 3, p["out"]), dict(b=B),
                              dict(out=devptr.Out((n, 3), np.float64)), odd=("b",))
    assert res["host"][0] == N.GH_OK
    which = np.ones(len(kernel), dtype=np.uint32)
    res = devptr.check_routes("gh_inducing_grad", lambda p: N.lib.gh_inducing_grad(h, k, N.ptr(which), p["r"], p["grad"], p["alpha"], p["diagA"]),
                              dict(r=r), dict(grad=devptr.Out((len(which),), np.float64), alpha=devptr.Out((n,), np.float64),
                                              diagA=devptr.Out((n,), np.float64)), odd=("r",))
    assert res["host"][0] == N.GH_OK and np.array_equal(res["host"][1]["alpha"], s.apply_inverse(r))
    res = devptr.check_routes("gh_inducing_predict", lambda p: N.lib.gh_inducing_predict(h, k, p["r"], p["xs"], 300, p["mu"], p["var"], None),
                              dict(r=r, xs=xs), dict(mu=devptr.Out((300,), np.float64), var=devptr.Out((300,), np.float64)), odd=("r", "xs"))
    assert res["host"][0] == N.GH_OK
    res = devptr.check_routes("gh_inducing_predict", lambda p: N.lib.gh_inducing_predict(h, k, p["r"], p["xs"], 130, p["mu"], None, p["cov"]),
                              dict(r=r, xs=xs[:130]), dict(mu=devptr.Out((130,), np.float64), cov=devptr.Out((130, 130), np.float64)),
                              odd=("r", "xs"))
    assert res["host"][0] == N.GH_OK
