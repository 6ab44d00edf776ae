"""Parity of the HIP dense solver path (through the C ABI and the GP facade) with the reference.
Structure follows the reference's own tests (tests/test_solvers.py:29-58, tests/test_gp.py:16-171,
tests/test_pickle.py, tests/test_tutorial.py) plus the committed golden vectors of the reduced
BASELINE configs and size-independent properties at the full C2 size.

Tolerances (fp64): log-likelihood 1e-6 relative is the north-star bound; what we assert is 1e-9.
"""
import pickle
from itertools import product

import numpy as np
import pytest

import zoo
from oracle import solver_np
import george_amd
from george_amd import kernels, GP, BasicSolver

pytestmark = pytest.mark.gpu


def _as2d(x):
    return x[:, None] if x.ndim == 1 else x


# ------------------------------------------------------------------ tests/test_solvers.py:29-58
@pytest.mark.parametrize("N", [300, 128, 1, 513])
def test_basic_solver(N, seed=1234):
    kernel = 1.0 * kernels.ExpSquaredKernel(1.0)
    solver = BasicSolver(kernel)
    np.random.seed(seed)
    x = np.atleast_2d(np.sort(10 * np.random.randn(N))).T
    yerr = np.ones(N)
    solver.compute(x, yerr)
    K = kernel.get_value(x)
    K[np.diag_indices_from(K)] += yerr ** 2
    sgn, lndet = np.linalg.slogdet(K)
    assert sgn == 1.0, "Invalid determinant"
    assert np.allclose(solver.log_determinant, lndet), "Incorrect determinant"
    y = np.sin(x[:, 0])
    b0 = np.linalg.solve(K, y)
    b = solver.apply_inverse(y).flatten()
    assert np.allclose(b, b0)
    assert np.allclose(solver.apply_inverse(K), np.eye(N)), "Incorrect inverse"
    assert np.allclose(solver.get_inverse(), np.linalg.inv(K))
    assert np.allclose(solver.dot_solve(y), y @ b0)
    # U^T U = K with apply_sqrt(r) = r @ U (basic.py:104-114)
    U = solver.apply_sqrt(np.eye(N))
    assert np.allclose(U.T @ U, K)
    assert np.allclose(np.tril(U, -1), 0.0)


# ----------------------------------------------------------------------- golden vectors (reference)
@pytest.mark.parametrize("name", ["scaling100", "C1", "C2small", "C3small", "C5small"])
def test_reduced_baseline_configs_match_reference(name, golden_gp):
    g = golden_gp
    kernel, x, yerr, y = zoo.gp_configs(kernels)[name]
    gp = GP(kernel)
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    ref = float(g[name + "/loglike"])
    assert abs(ll - ref) <= 1e-9 * abs(ref), (ll, ref)
    assert abs(gp.solver.log_determinant - float(g[name + "/logdet"])) <= 1e-9 * abs(float(g[name + "/logdet"]))
    t = g[name + "/t"]
    mu, var = gp.predict(y, t, return_var=True)
    np.testing.assert_allclose(mu, g[name + "/mu"], rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(var, g[name + "/var"], rtol=1e-6, atol=1e-9)
    mu16, cov = gp.predict(y, t[:16])
    np.testing.assert_allclose(cov, g[name + "/cov16"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(mu16, g[name + "/mu"][:16], rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(gp.grad_log_likelihood(y), g[name + "/grad"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(gp.apply_inverse(y), g[name + "/alpha"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(gp.apply_inverse(g[name + "/Y5"]), g[name + "/alpha5"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gp.solver.apply_sqrt(g[name + "/r3"]), g[name + "/sqrt3"], rtol=1e-8, atol=1e-10)


def test_published_scaling_value():
    kernel, x, yerr, y = zoo.gp_configs(kernels)["scaling100"]
    gp = GP(kernel)
    gp.compute(x, yerr)
    assert abs(gp.log_likelihood(y) - 133.946394912) < 5e-9          # docs/tutorials/scaling.rst:76


def test_white_noise_and_mean_gradient_match_reference(golden_gp):
    kernel, x, yerr, y = zoo.gp_configs(kernels)["C5small"]
    gp = GP(kernel, mean=0.3, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True)
    gp.compute(x, yerr)
    assert list(gp.get_parameter_names()) == list(golden_gp["C5wn/names"])
    ref = float(golden_gp["C5wn/loglike"])
    assert abs(gp.log_likelihood(y) - ref) <= 1e-9 * abs(ref)
    np.testing.assert_allclose(gp.grad_log_likelihood(y), golden_gp["C5wn/grad"], rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------- tests/test_gp.py:16-56
@pytest.mark.parametrize("white_noise", [None, 0.1])
def test_gradient(white_noise, seed=123, N=305, ndim=3, eps=1.32e-3):
    np.random.seed(seed)
    kernel = 1.0 * kernels.ExpSquaredKernel(0.5, ndim=ndim)
    kwargs = dict()
    if white_noise is not None:
        kwargs = dict(white_noise=white_noise, fit_white_noise=True)
    gp = GP(kernel, solver=BasicSolver, **kwargs)
    x = np.random.rand(N, ndim)
    x = x[np.argsort(x[:, 0])]
    y = gp.sample(x)
    gp.compute(x, yerr=0.1)
    grad0 = gp.grad_log_likelihood(y)
    vector = gp.get_parameter_vector()
    for i, v in enumerate(vector):
        vector[i] = v + eps
        gp.set_parameter_vector(vector)
        lp = gp.log_likelihood(y)
        vector[i] = v - eps
        gp.set_parameter_vector(vector)
        lm = gp.log_likelihood(y)
        vector[i] = v
        gp.set_parameter_vector(vector)
        grad = 0.5 * (lp - lm) / eps
        assert np.abs(grad - grad0[i]) < 5 * eps, (i, grad, grad0[i])


def test_prediction(seed=42):                                           # tests/test_gp.py:59-83
    np.random.seed(seed)
    kernel = kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel, solver=BasicSolver, white_noise=0.0)
    x0 = np.linspace(-10, 10, 500)
    x = np.sort(np.random.uniform(-10, 10, 300))
    gp.compute(x)
    y = np.sin(x)
    mu, cov = gp.predict(y, x0)
    Kstar = gp.get_matrix(x0, x)
    K = gp.get_matrix(x)
    K[np.diag_indices_from(K)] += 1.0
    mu0 = np.dot(Kstar, np.linalg.solve(K, y))
    assert np.allclose(mu, mu0)
    cov0 = gp.get_matrix(x0) - Kstar @ np.linalg.solve(K, Kstar.T)
    assert np.allclose(cov, cov0)


def test_repeated_prediction_cache():                                   # tests/test_gp.py:86-120
    kernel = kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel)
    x = np.array((-1, 0, 1))
    gp.compute(x)
    t = np.array((-.5, .3, 1.2))
    y = x / x.std()
    mu0, mu1 = (gp.predict(y, t, return_cov=False) for _ in range(2))
    assert np.array_equal(mu0, mu1)
    y2 = 2 * y
    mu2 = gp.predict(y2, t, return_cov=False)
    assert not np.array_equal(mu0, mu2)
    a0 = gp._alpha
    gp.kernel[0] += 0.1
    gp.recompute()
    gp._compute_alpha(y2, True)
    a1 = gp._alpha
    assert not np.allclose(a0, a1)
    mu, cov = gp.predict(y2, t)
    _, var = gp.predict(y2, t, return_var=True)
    assert np.allclose(np.diag(cov), var)


def test_apply_inverse(seed=1234, N=201, yerr=0.1):                     # tests/test_gp.py:123-149
    np.random.seed(seed)
    kernel = 1.0 * kernels.ExpSquaredKernel(0.5)
    gp = GP(kernel, solver=BasicSolver)
    x = np.sort(np.random.rand(N))
    y = gp.sample(x)
    gp.compute(x, yerr=yerr)
    K = gp.get_matrix(x)
    K[np.diag_indices_from(K)] += yerr ** 2
    assert np.allclose(np.linalg.solve(K, y), gp.apply_inverse(y))
    y = gp.sample(x, size=5).T
    assert np.allclose(np.linalg.solve(K, y), gp.apply_inverse(y))


def test_predict_single(seed=1234, N=201, yerr=0.1):                    # tests/test_gp.py:152-171
    np.random.seed(seed)
    kernel = 1.0 * kernels.ExpSquaredKernel(0.5)
    gp = GP(kernel, solver=BasicSolver)
    x = np.sort(np.random.rand(N))
    y = gp.sample(x)
    gp.compute(x, yerr=yerr)
    mu0, var0 = gp.predict(y, [0.0], return_var=True)
    mu, var = gp.predict(y, [0.0, 1.0], return_var=True)
    _, cov = gp.predict(y, [0.0, 1.0])
    assert np.allclose(mu0, mu[0])
    assert np.allclose(var0, var[0])
    assert np.allclose(var0, cov[0, 0])


def test_sampling_from_factor(seed=3):
    np.random.seed(seed)
    gp = GP(2.0 * kernels.Matern32Kernel(1.0))
    x = np.linspace(0, 5, 150)
    gp.compute(x, 0.01)
    s = gp.sample(size=4000)                                            # gp.py:586-593 via apply_sqrt
    K = gp.get_matrix(x) + np.diag(np.full(150, 1e-4 + george_amd.gp.TINY))
    emp = np.cov(s.T)
    assert np.abs(emp - K).max() < 0.35
    assert gp.sample().shape == (150,)


# ------------------------------------------------------------------- failure path (gp.py:356-359)
def test_not_positive_definite_maps_to_linalgerror():
    k = kernels.CosineKernel(log_period=0.0)        # rank-2 kernel: singular without noise
    x = np.linspace(0, 3, 200)
    s = BasicSolver(k)
    with pytest.raises(np.linalg.LinAlgError):
        s.compute(x[:, None], np.zeros(200))
    gp = GP(k, white_noise=-1000.0)
    gp.compute(x[:5], 1.0)
    gp._x, gp._yerr2 = np.ascontiguousarray(x[:, None]), np.zeros(200)
    gp.kernel.dirty = True
    assert gp.log_likelihood(np.sin(x), quiet=True) == -np.inf
    assert np.all(gp.grad_log_likelihood(np.sin(x), quiet=True) == 0.0)
    with pytest.raises(RuntimeError):
        BasicSolver(k).apply_inverse(np.zeros(3))     # "you must call 'compute' first"


def _fake_compute(arg, *args, **kwargs):
    assert 0, "Unpickled GP shouldn't need to be computed"


def test_pickle_keeps_the_factor(N=50, seed=123):                       # tests/test_pickle.py:21-36, BasicSolver/True
    np.random.seed(seed)
    kernel = 0.1 * kernels.ExpSquaredKernel(1.5)
    gp = GP(kernel, solver=BasicSolver)
    x = np.random.rand(100)
    gp.compute(x, 1e-2)
    ll = gp.log_likelihood(np.sin(x))
    mu, var = gp.predict(np.sin(x), np.linspace(0, 1, 7), return_var=True)
    g = gp.grad_log_likelihood(np.sin(x))
    s = pickle.dumps(gp, -1)
    gp = pickle.loads(s)
    gp.compute = _fake_compute
    assert gp.computed
    with pytest.warns(DeprecationWarning):
        assert gp.lnlikelihood(np.sin(x)) == ll                            # the very same factor: same bits
    mu2, var2 = gp.predict(np.sin(x), np.linspace(0, 1, 7), return_var=True)
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
    assert np.allclose(gp.grad_log_likelihood(np.sin(x)), g, rtol=1e-12, atol=0)
    # a pickle of the unpickled-and-untouched object carries the factor on
    gp3 = pickle.loads(pickle.dumps(pickle.loads(s), -1))
    gp3.compute = _fake_compute
    assert gp3.log_likelihood(np.sin(x)) == ll


def test_pickle_roundtrip_mid_size_and_threshold(seed=1234):
    np.random.seed(seed)
    x, yerr, y = zoo.bench_data(1500)                                      # not a multiple of 128: padding path
    gp = GP(np.var(y) * kernels.Matern32Kernel(1.0))
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    a = gp.apply_inverse(y)
    gp2 = pickle.loads(pickle.dumps(gp, -1))
    assert gp2.computed and gp2.log_likelihood(y) == ll and np.array_equal(gp2.apply_inverse(y), a)
    assert np.array_equal(gp2.solver.apply_sqrt(np.ones(1500)), gp.solver.apply_sqrt(np.ones(1500)))
    # above the size threshold the factor is dropped, as the reference's native solver does (hodlr.py:69-76)
    old = BasicSolver.PICKLE_FACTOR_MAX_N
    BasicSolver.PICKLE_FACTOR_MAX_N = 1000
    try:
        gp4 = pickle.loads(pickle.dumps(gp, -1))
    finally:
        BasicSolver.PICKLE_FACTOR_MAX_N = old
    assert not gp4.computed
    assert np.isclose(gp4.log_likelihood(y), ll, rtol=1e-12)                # recomputed transparently


# ------------------------------------------------------------------ fused objective (gp.py:470-480)
@pytest.mark.parametrize("fit_mean,fit_wn", [(False, False), (True, True)])
def test_fused_objective_matches_separate_calls(fit_mean, fit_wn):
    x, yerr, y = zoo.bench_data(700, ndim=3)
    def make():
        kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
        kw = dict(mean=0.3, fit_mean=True) if fit_mean else {}
        if fit_wn:
            kw.update(white_noise=np.log(0.05), fit_white_noise=True)
        gp = GP(kernel, **kw)
        gp.compute(x, yerr)
        return gp
    ref, gp = make(), make()
    p = ref.get_parameter_vector() + 0.05
    ref.set_parameter_vector(p)
    ll0, g0 = ref.log_likelihood(y), ref.grad_log_likelihood(y)            # separate calls (compute / dot_solve / grad)
    v, g = gp.nll_and_grad(p, y)                                           # ONE device call
    assert abs(v + ll0) <= 1e-12 * abs(ll0)
    np.testing.assert_allclose(-g, g0, rtol=1e-10, atol=1e-10)
    assert gp.computed
    # optimiser call pattern: value then gradient at every iterate; after the first gradient request
    # nll computes the gradient eagerly and grad_nll at the same point is served from it
    gp = make()
    calls = []
    real = BasicSolver.objective
    def spy(self, *a, **k):
        calls.append(k.get("want_grad", True))
        return real(self, *a, **k)
    BasicSolver.objective = spy
    try:
        for step in range(3):
            q = p + 0.01 * step
            v = gp.nll(q, y)
            g = gp.grad_nll(q, y)
            ref.set_parameter_vector(q)
            assert abs(v + ref.log_likelihood(y)) <= 1e-12 * abs(v)
            np.testing.assert_allclose(-g, ref.grad_log_likelihood(y), rtol=1e-10, atol=1e-10)
    finally:
        BasicSolver.objective = real
    # step 0: a value-only fused call (no gradient had been asked for yet; its gradient then comes from
    # the factor already on the device); from then on ONE fused call per iterate
    assert calls == [False, True, True], calls


def test_fused_objective_iterates_do_not_reallocate():
    """An optimiser loop drops its solver at every iterate (gp.py:327); the pooled native handle must
    come back WITH its work arrays (round 2 trimmed it on every drop: two or three hipFree + hipMalloc
    of 8 N^2 bytes per iterate made the fused call 2x slower than the separate calls).  Iterates 3-5 of
    nll_and_grad at N = 8192 must cost no more than compute + dot_solve + grad (+10 %), and the
    handle's device footprint must not move between them."""
    import time
    from george_amd import _native as Nat
    x, yerr, y = zoo.bench_data(8192, ndim=3)
    kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
    gp = GP(kernel)
    sep = []
    for rep in range(3):
        gp.kernel.dirty = True
        t0 = time.perf_counter()
        gp.compute(x, yerr); gp.log_likelihood(y); gp.grad_log_likelihood(y)
        sep.append(time.perf_counter() - t0)
    p = gp.get_parameter_vector()
    fused, foot = [], []
    for it in range(5):
        t0 = time.perf_counter()
        v, g = gp.nll_and_grad(p + 1e-3 * (it + 1), y)
        fused.append(time.perf_counter() - t0)
        foot.append(int(Nat.lib.gh_chol_device_bytes(gp.solver._handle)))
    assert len(set(foot[2:])) == 1, foot
    assert sorted(fused[2:])[1] <= 1.10 * min(sep[1:]), (fused, sep)
    # and the values are those of the separate calls at the last point
    ref = GP(kernel)
    ref.compute(x, yerr)
    ref.set_parameter_vector(p + 5e-3)
    assert abs(v + ref.log_likelihood(y)) <= 1e-12 * abs(v)
    np.testing.assert_allclose(-g, ref.grad_log_likelihood(y), rtol=1e-10, atol=1e-10)


def test_gradient_cache_is_dropped_by_compute():
    """the gradient cached by the fused objective is keyed on (vector, y); compute() with
    other inputs at the same vector must not serve the old one."""
    x, yerr, y = zoo.bench_data(600)
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x, yerr)
    p = gp.get_parameter_vector() + 0.01
    gp.grad_nll(p, y)
    v, g_old = gp.nll_and_grad(p + 0.01, y)
    gp.compute(x, 3.0 * yerr)                                              # same vector, other error bars
    g_new = gp.grad_nll(p + 0.01, y)
    ref = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    ref.compute(x, 3.0 * yerr)
    ref.set_parameter_vector(p + 0.01)
    np.testing.assert_allclose(g_new, -ref.grad_log_likelihood(y), rtol=1e-10, atol=1e-10)
    assert not np.allclose(g_new, g_old, rtol=1e-3)
    # value-only evaluations switch the eager gradient off again (gradient-free optimisers, MCMC)
    calls = []
    real = BasicSolver.objective
    def spy(self, *a, **k):
        calls.append(k.get("want_grad", True))
        return real(self, *a, **k)
    BasicSolver.objective = spy
    try:
        for step in range(4):
            gp.nll(p + 0.1 + 0.01 * step, y)
    finally:
        BasicSolver.objective = real
    assert calls == [True, True, False, False], calls


def test_objective_quiet_and_errors():
    k = kernels.CosineKernel(log_period=0.0)                               # singular without noise
    x = np.linspace(0, 3, 200)
    gp = GP(k, white_noise=-1000.0)
    gp.compute(x[:5], 1.0)
    gp._x, gp._yerr2 = np.ascontiguousarray(x[:, None]), np.zeros(200)
    gp.kernel.dirty = True
    p = gp.get_parameter_vector()
    assert gp.nll(p, np.sin(x)) == np.inf
    gp.kernel.dirty = True
    assert np.all(gp.grad_nll(p, np.sin(x)) == 0.0)
    gp.kernel.dirty = True
    with pytest.raises(np.linalg.LinAlgError):
        gp.nll(p, np.sin(x), quiet=False)
    # a wrongly shaped y is an error even in quiet mode (only mean-function failures are silenced)
    gp2 = GP(1.0 * kernels.ExpSquaredKernel(1.0))
    gp2.compute(x, 0.1)
    with pytest.raises(ValueError):
        gp2.log_likelihood(np.zeros(7), quiet=True)
    with pytest.raises(ValueError):
        gp2.nll(gp2.get_parameter_vector() + 0.1, np.zeros(7))
    with pytest.raises(ValueError):
        gp2.grad_log_likelihood(np.zeros((200, 2)), quiet=True)


def test_handle_pool_is_budgeted_and_releasable():
    x, yerr, y = zoo.bench_data(1024)
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x, yerr)
    gp.grad_log_likelihood(y)                                              # grows the N x N work buffers
    ll = gp.log_likelihood(y)
    del gp
    import gc
    gc.collect()
    assert sum(len(v) for v in BasicSolver._POOL.values()) >= 1
    BasicSolver.release_pool()
    assert sum(len(v) for v in BasicSolver._POOL.values()) == 0
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x, yerr)
    assert gp.log_likelihood(y) == ll
    # the byte budget: a handle is parked as it is while it fits, trimmed to its factor when only that
    # fits, destroyed otherwise
    from george_amd import _native as Nat
    parked = lambda: [h for v in BasicSolver._POOL.values() for h in v]
    old = BasicSolver._POOL_MAX_BYTES
    try:
        gp.grad_log_likelihood(y)
        full = int(Nat.lib.gh_chol_device_bytes(gp.solver._handle))
        assert full > 20 << 20                                             # factor 8 MB + two N x N work arrays
        del gp
        gc.collect()
        assert len(parked()) == 1 and int(Nat.lib.gh_chol_device_bytes(parked()[0])) == full       # untrimmed
        gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
        gp.compute(x, yerr)                                                # takes the parked handle
        assert len(parked()) == 0
        BasicSolver._POOL_MAX_BYTES = 12 << 20
        del gp
        gc.collect()
        assert len(parked()) == 1 and int(Nat.lib.gh_chol_device_bytes(parked()[0])) <= 12 << 20   # trimmed
        gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
        gp.compute(x, yerr)
        BasicSolver._POOL_MAX_BYTES = 1 << 20
        del gp
        gc.collect()
        assert len(parked()) == 0                                          # destroyed
    finally:
        BasicSolver._POOL_MAX_BYTES = old


def test_stepwise_trsv_arm_still_works(tmp_path):
    """GEORGE_AMD_TRSV_STEPS selects the one-launch-per-block-row solves (the fallback should the
    chained kernels' in-order dispatch assumption ever fail): keep it exercised.  The switch is read once per process,
    hence the children.  Beside the log-likelihood and the solve at N = 1500, every entry point with a sweep arm of its own
    -- the fused objective, predict_gradient, the leave-one-out value and gradient paths -- runs at N = 300 (three tiles,
    the last one ragged) and EACH arm is held to the NumPy references of tests/grad_ref.py, predgrad_ref.py and loo_ref.py
    under their tolerance rule, as test_gpu_grad_reference.py, test_gpu_predict_gradient.py and test_gpu_loo.py do."""
    import subprocess, sys, os
    import grad_ref, predgrad_ref, loo_ref
    from george_amd.gp import TINY
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests'); import numpy as np, zoo\n"
            "from george_amd import GP, kernels\n"
            "x, yerr, y = zoo.bench_data(1500)\n"
            "gp = GP(np.var(y) * kernels.Matern32Kernel(1.0)); gp.compute(x, yerr)\n"
            "print(repr(float(gp.log_likelihood(y))), repr(float(y @ gp.apply_inverse(y))))\n"
            "x, yerr, y = zoo.bench_data(300)\n"
            "t = x[[3, 70, 150, 222, 298]] + np.array([0.01, -0.02, 0.03, 0.015, -0.01])\n"
            "gp = GP(np.var(y) * kernels.Matern32Kernel(1.0)); gp.compute(x, yerr)\n"
            "gp.kernel.dirty = True                              # refactorise through the fused objective\n"
            "nll, g = gp.nll_and_grad(gp.get_parameter_vector(), y)\n"
            "mu, var, dmu, dvar = gp.predict_gradient(y, t, return_var=True, return_value=True)\n"
            "np.savez(sys.argv[1], nll=nll, g=g, mu=mu, var=var, dmu=dmu, dvar=dvar,\n"
            "         L=gp.loo_log_likelihood(y), gL=gp.grad_loo_log_likelihood(y))\n") % (root, root)
    x, yerr, y = zoo.bench_data(300)
    n = len(x)
    kernel = np.var(y) * kernels.Matern32Kernel(1.0)
    sigma = np.sqrt(yerr ** 2 + TINY)
    t = x[[3, 70, 150, 222, 298]] + np.array([0.01, -0.02, 0.03, 0.015, -0.01])      # (the child's test points)
    gref = grad_ref.reference(kernel, x, sigma, y)
    lref = loo_ref.reference(kernel, x[:, None], sigma, y)
    pref = predgrad_ref.reference(kernel, x[:, None], sigma, y, t[:, None])
    assert gref.kappa <= 1e6
    outs = []
    for arm, env in enumerate(({}, {"GEORGE_AMD_TRSV_STEPS": "1"})):
        e = dict(os.environ); e.update(env)
        npz = str(tmp_path / ("arm%d.npz" % arm))
        r = subprocess.run([sys.executable, "-c", code, npz], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([float(v) for v in r.stdout.split()[-2:]])
        d = np.load(npz)
        ratios = dict(
            nll=abs(-float(d["nll"]) + 0.5 * (gref.quad + gref.logdet + n * np.log(2 * np.pi))) / (0.5 * (gref.tol_quad() + gref.tol_logdet())),
            grad=gref._ratio(-d["g"] - gref.g, gref.tol_grad()),
            mu=pref.pred.ratio_mu(d["mu"]), var=pref.pred.ratio_var(d["var"]),
            dmu=pref.ratio_dmu(d["dmu"].reshape(-1, 1)), dvar=pref.ratio_dvar(d["dvar"].reshape(-1, 1)),
            L=lref.ratio("L", float(d["L"])), gL=loo_ref.Ref._ratio(d["gL"] - lref.g, lref.tol("g")))
        print("%s arm: kappa %.3g, error / tolerance %s" % ("stepwise" if env else "chained", gref.kappa,
                                                             ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
        assert d["g"].shape == d["gL"].shape == (2,) and d["dmu"].size == d["dvar"].size == 5
        assert max(ratios.values()) <= 1.0, (env, ratios)
    assert abs(outs[0][0] - outs[1][0]) <= 1e-11 * abs(outs[0][0])
    assert abs(outs[0][1] - outs[1][1]) <= 1e-9 * abs(outs[0][1])


def test_chained_solves_are_bit_stable_under_load():
    """The chained solves (trsv_fwd_chain_direct / trsv_bwd_chain_direct: one launch, workgroup b waits for the z_j of
    its predecessors by polling the values themselves -- sentinel-filled output, agent-scope atomics, no fences --
    and every log-likelihood goes through them) repeated 150 times, first alone, then while a second thread keeps the chip full with factorisations of
    another matrix on the SAME process-wide streams: every repetition must reproduce the first result bit for bit
    (a stale value or a missed hand-over shows up as a different sum), and a factor recomputed in between must too."""
    import threading
    x, yerr, y = zoo.bench_data(8192)
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x, yerr)
    q0 = gp.solver.dot_solve(y)
    a0 = gp.solver.apply_inverse(y)
    for _ in range(50):
        assert gp.solver.dot_solve(y) == q0
    x2, yerr2, y2 = zoo.bench_data(6144)
    other = GP(np.var(y2) * kernels.Matern32Kernel(1.0))
    other.compute(x2, yerr2)
    ld2 = other.solver.log_determinant
    stop, bad = threading.Event(), []

    def load():
        while not stop.is_set():
            other.kernel.dirty = True
            other.compute(x2, yerr2)
            if other.solver.log_determinant != ld2:
                bad.append(other.solver.log_determinant)

    t = threading.Thread(target=load)
    t.start()
    try:
        for rep in range(100):
            assert gp.solver.dot_solve(y) == q0, rep
            if rep % 10 == 0:
                assert np.array_equal(gp.solver.apply_inverse(y), a0), rep
            if rep % 25 == 24:                                             # a fresh factor of the same matrix
                gp.kernel.dirty = True
                gp.compute(x, yerr)
    finally:
        stop.set()
        t.join()
    assert not bad, bad[:3]


def test_tutorial_kernel_family():                                      # tests/test_tutorial.py
    rng = np.random.RandomState(1)
    x = np.sort(rng.uniform(0, 30, 50))
    y = np.sin(x) + 0.1 * rng.randn(50)
    kernel = 2.0 * kernels.Matern32Kernel(3.0) + 0.001
    gp = GP(kernel)
    gp.compute(x, 0.1)
    ref = solver_np.gp_log_likelihood(solver_np.DenseOracle(kernel), x[:, None], 0.1, y)
    assert np.isclose(gp.log_likelihood(y), ref, rtol=1e-10)


# -------------------------------------------------------------- mid / full size parity + properties
def test_n4096_vs_oracle():
    x, yerr, y = zoo.bench_data(4096)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel)
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    ref = solver_np.gp_log_likelihood(solver_np.DenseOracle(kernel), x[:, None], yerr, y)
    assert abs(ll - ref) <= 1e-9 * abs(ref), (ll, ref)


@pytest.mark.parametrize("nb", [256, 512, 1024])
def test_panel_width_does_not_change_result(nb):
    x, yerr, y = zoo.bench_data(2000)
    kernel = np.var(y) * kernels.Matern32Kernel(1.0)
    base = GP(kernel)
    base.compute(x, yerr)
    gp = GP(kernel, nb=nb)
    gp.compute(x, yerr)
    assert abs(gp.log_likelihood(y) - base.log_likelihood(y)) <= 1e-10 * abs(base.log_likelihood(y))


def test_adaptive_panel_width_gives_the_same_bits():
    """Round 6: with the panel width left to the solver, panels are 2048 columns wide while more than 25 600 columns of trailing
    matrix lie behind them, 1024 after (gh_chol.hip, panel_starts).  A wide update adds the same k-steps in the same order as the
    two narrow ones it replaces: the factor is IDENTICAL -- log-determinant, quadratic form and alpha bit for bit.  N = 30000:
    three wide panels, then 1024s (and a ragged last panel)."""
    from george_amd import _native as N
    n = 30000
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    got = {}
    try:
        for mode in (0, 1, 8192):                       # off / default bound / wide panels far into the matrix
            N.lib.gh_debug_set_adaptive_panels(mode)
            s = BasicSolver(kernel)
            s.compute(x[:, None], yerr)
            got[mode] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y))
            del s
    finally:
        N.lib.gh_debug_set_adaptive_panels(1)
    for mode in (1, 8192):
        assert got[mode][0] == got[0][0] and got[mode][1] == got[0][1]
        assert np.array_equal(got[mode][2], got[0][2])


@pytest.mark.parametrize("n", [1500, 3000, 9000])
def test_build_on_the_chain_stream_gives_the_same_bits(n):
    """Round 6: with look-ahead, a compute()'s inputs and kernel-matrix build are enqueued on the chain stream (the first panel is the
    first thing that needs them) instead of the main stream + a cross-stream hand-over (gh_debug_set_build_on_chain).  Where the
    work is enqueued changes nothing it computes: identical log-determinant, quadratic form and alpha; a second compute() of the
    same handle (the streams are re-used) and NumPy inputs (copies instead of the one-launch input staging) included."""
    from george_amd import _native as N
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.Matern32Kernel(1.0)
    got = {}
    try:
        for mode in (0, 1):
            N.lib.gh_debug_set_build_on_chain(mode)
            s = BasicSolver(kernel)
            s.compute(x[:, None], yerr)
            first = (s.log_determinant, s.dot_solve(y))
            s.compute(x[:, None], yerr)
            assert (s.log_determinant, s.dot_solve(y)) == first
            got[mode] = first + (s.apply_inverse(y),)
            del s
    finally:
        N.lib.gh_debug_set_build_on_chain(1)
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1]
    assert np.array_equal(got[1][2], got[0][2])


def test_full_size_c2_properties():
    """BASELINE config C2 (N=16384, 1-D ExpSquared): too slow for the CPU oracle inside a test
    (~30 s), so check size-independent properties: residual of the solve against an independent
    device mat-vec, log-det scaling law, and run-to-run bitwise determinism."""
    n = 16384
    x, yerr, y = zoo.bench_data(n)
    amp = np.var(y)
    kernel = amp * kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel)
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    alpha = gp.apply_inverse(y)
    # K alpha == y, with K rows rebuilt independently through value_general in chunks
    X = x[:, None]
    res = 0.0
    for s in range(0, n, 2048):
        Kc = kernel.get_value(X[s:s + 2048], X)
        Kc[np.arange(Kc.shape[0]), np.arange(s, s + Kc.shape[0])] += yerr[s:s + 2048] ** 2
        res = max(res, np.abs(Kc @ alpha - y[s:s + 2048]).max())
    assert res < 1e-8, res
    assert np.isclose(gp.solver.dot_solve(y), y @ alpha, rtol=1e-9)
    # log|c K| = log|K| + n log c
    c = 3.0
    gp2 = GP((c * amp) * kernels.ExpSquaredKernel(1.0))
    gp2.compute(x, np.sqrt(c) * yerr)
    assert abs(gp2.solver.log_determinant - (gp.solver.log_determinant + n * np.log(c))) < 1e-6 * n
    gp3 = GP(kernel)
    gp3.compute(x, yerr)
    assert gp3.log_likelihood(y) == ll                                   # deterministic


def test_full_size_c3_properties():
    """BASELINE config C3's single-GPU part (N=65536, 1-D Matern32, the 34-GB matrix): the same
    size-independent properties, the residual on a sample of row blocks (the full K would be 34 GB
    through PCIe)."""
    n = 65536
    x, yerr, y = zoo.bench_data(n)
    amp = np.var(y)
    kernel = amp * kernels.Matern32Kernel(1.0)
    gp = GP(kernel)
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    assert np.isfinite(ll)
    alpha = gp.apply_inverse(y)
    X = x[:, None]
    res = 0.0
    for s in (0, 20480, 43008, n - 1024):
        Kc = kernel.get_value(X[s:s + 1024], X)
        Kc[np.arange(1024), np.arange(s, s + 1024)] += yerr[s:s + 1024] ** 2
        res = max(res, np.abs(Kc @ alpha - y[s:s + 1024]).max())
    assert res < 1e-7, res
    assert np.isclose(gp.solver.dot_solve(y), y @ alpha, rtol=1e-9)
    c = 3.0
    gp2 = GP((c * amp) * kernels.Matern32Kernel(1.0))
    gp2.compute(x, np.sqrt(c) * yerr)
    assert abs(gp2.solver.log_determinant - (gp.solver.log_determinant + n * np.log(c))) < 1e-6 * n
    gp3 = GP(kernel)
    gp3.compute(x, yerr)
    assert gp3.log_likelihood(y) == ll                                   # deterministic


@pytest.mark.parametrize("n", [130, 1000, 5000, 20000])
def test_chained_forward_solve_repeatable(n):
    """The forward sweep is ONE launch whose workgroups hand z blocks to each other through HBM
    (gh_chol_solve.hip, trsv_fwd_chain_direct): hammer it -- 25 sweeps per size must give the same bits, and
    r^T K^-1 r must agree with the full solve r . apply_inverse(r) (forward + backward sweeps)."""
    x, yerr, y = zoo.bench_data(n)
    s = BasicSolver(np.var(y) * kernels.Matern32Kernel(1.0))
    s.compute(x[:, None] if x.ndim == 1 else x, yerr)
    rng = np.random.default_rng(3)
    r = rng.standard_normal(n)
    first = s.dot_solve(r)
    for _ in range(24):
        assert s.dot_solve(r) == first
    full = float(r @ s.apply_inverse(r))
    assert abs(first - full) <= 1e-10 * abs(full)


def test_full_size_c5_properties():
    """BASELINE config C5 at full size (N=32768, 3-D, Matern52 + Constant): the fused predict()
    against its definition through independent entry points, grad_log_likelihood() against central
    differences of log_likelihood()."""
    n, m = 32768, 64
    rng = np.random.RandomState(1234)
    x = rng.uniform(0, 1, (n, 3))
    x = x[np.argsort(x[:, 0])]
    y = np.sin(x.sum(axis=1))
    t = rng.uniform(0, 1, (m, 3))
    kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
    gp = GP(kernel)
    gp.compute(x, 0.1)
    mu, var = gp.predict(y, t, return_var=True)
    alpha = gp.apply_inverse(y)
    Kts = kernel.get_value(t, x)                                     # (m, n) through value_general
    assert np.allclose(mu, Kts @ alpha, rtol=1e-9, atol=1e-11)
    KinvKst = gp.apply_inverse(np.ascontiguousarray(Kts.T))          # (n, m): multi-RHS solve
    var_def = kernel.get_value(t, diag=True) - np.sum(Kts.T * KinvKst, axis=0)     # gp.py:539
    assert np.allclose(var, var_def, rtol=1e-7, atol=1e-12)
    g = gp.grad_log_likelihood(y)
    p0 = gp.get_parameter_vector()
    eps = 1e-5
    for i in range(len(p0)):
        p = p0.copy(); p[i] += eps; gp.set_parameter_vector(p); fp = gp.log_likelihood(y)
        p = p0.copy(); p[i] -= eps; gp.set_parameter_vector(p); fm = gp.log_likelihood(y)
        assert abs((fp - fm) / (2 * eps) - g[i]) <= 1e-5 * max(1.0, abs(g[i])), (i, (fp - fm) / (2 * eps), g[i])
    gp.set_parameter_vector(p0)


def test_scalar_potf2_validation_arm_agrees():
    """GEORGE_AMD_POTF2=simple selects the scalar 128x128 Cholesky + inverse kernel (the validation arm
    of the MFMA form, as GEORGE_AMD_NO_MFMA=1 is for the GEMMs): same factorisation to rounding, on
    repeated computes with one handle too."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import bench\n"
            "for n in (1000, 4096):\n"
            "    job = bench.DenseJob(n, 0, 0, profile=False)\n"
            "    print(' '.join(repr(float(job.step())) for _ in range(2)))\n"
            "    job.close()\n") % root
    outs = []
    for env in ({}, {"GEORGE_AMD_POTF2": "simple"}):
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()[-2:]])
    for a, b in zip(outs[0], outs[1]):
        assert a[0] == a[1] and b[0] == b[1]                              # each arm repeatable
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])


def test_process_without_torch_runs_at_the_benchmarked_speed():
    """A george user's process never imports torch.  The library's streams are then the first thing created on the
    device, and before gh_prime_device (gh_common.h) the panel chain of every mid-size factorisation ran at half speed
    in such a process (N = 8192: 13.0 instead of 7.0 ms).  Runs scripts/dev/no_torch_step.py in a child process with
    and without the priming launch: same log-likelihood as here, torch really absent, and the primed run not slower
    than the unprimed one (a generous bound: the effect is 1.8x where it exists)."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "scripts", "dev", "no_torch_step.py")

    def run(extra):
        env = dict(os.environ)
        env.update(extra)
        r = subprocess.run([sys.executable, script, "8192"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-400:]
        m = re.search(r"N=\s*8192 GP.compute\+log_likelihood ([0-9.]+) ms \(torch imported: (\w+)\)\s+ll ([-0-9.e+]+)", r.stdout)
        assert m, r.stdout
        return float(m.group(1)), m.group(2), float(m.group(3))

    ms, torch_in, ll = run({})
    assert torch_in == "False"
    x, yerr, y = zoo.bench_data(8192)
    gp = GP(float(np.var(y)) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x, yerr)
    assert abs(ll - gp.log_likelihood(y)) <= 1e-9 * abs(ll)
    ms_unprimed, _, ll2 = run({"GEORGE_AMD_NO_NULL_PRIME": "1"})
    assert ll2 == ll
    assert ms <= 1.15 * ms_unprimed, (ms, ms_unprimed)
    assert ms <= 11.0, ms                                  # (7.0-7.4 ms on an MI355X; 13 ms is the failure this guards against)


@pytest.mark.parametrize("env", [{"GEORGE_AMD_RESERVE_CUS": "0"}, {"GEORGE_AMD_RESERVE_CUS": "16"}, {"GEORGE_AMD_NO_MFMA": "1"}])
def test_every_switch_the_library_still_reads(env):
    """Rounds 4 and 6 pruned the A/B switches whose losing arm has a committed measurement (DESIGN.md section 4 lists the nine the
    library still reads).  Each one that stayed is exercised: the scheduling knob (CUs kept free of the trailing update) must not
    change a bit of the answer; the plain-VALU GEMM arm agrees to rounding.  (GEORGE_AMD_POTF2, _TRSV_STEPS, _NO_NULL_PRIME, _NO_KMAT_INTERIOR, _NO_FAST_KERNEL have tests of their own.)"""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import bench\n"
            "for n in (1500, 5000, 9000, 14000):\n"
            "    job = bench.DenseJob(n, 0, 0, profile=(n == 9000))\n"
            "    print(' '.join(repr(float(job.step())) for _ in range(2)))\n"
            "    job.close()\n") % root
    outs = []
    for e_ in ({}, env):
        e = dict(os.environ); e.update(e_)
        r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([[float(v) for v in line.split()] for line in r.stdout.strip().splitlines()[-4:]])
    for a, b in zip(outs[0], outs[1]):
        assert a[0] == a[1] and b[0] == b[1]                              # repeatable on one handle
        if "GEORGE_AMD_NO_MFMA" in env:
            assert abs(a[0] - b[0]) <= 1e-11 * abs(a[0])
        else:
            assert a[0] == b[0], (env, a, b)
