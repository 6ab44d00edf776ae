"""GP.log_likelihood_batch / gh_chol_objective_batch on the MI355X: B log-likelihoods of one kernel structure in one device
call, against the one-problem path (bit for bit where the issue of the feature says so), against NumPy, and for batch
invariance, failures, GP state, the C ABI and steady-state behaviour."""
import ctypes as C
import time

import numpy as np
import pytest

from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from george_amd.program import DeviceKernel


def _hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _problem(kind, n, seed=0):
    """(gp computed at its initial vector, y, vectors (36, len(gp)): 32 walkers around the point and 4 far apart)"""
    rng = np.random.RandomState(seed + n)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        gp = GP(1.3 * kernels.ExpSquaredKernel(0.8), mean=0.2, fit_mean=True, white_noise=np.log(0.02), fit_white_noise=True)
        y = np.sin(x) + 0.2 * rng.randn(n)
    elif kind == "hyper":
        x = np.sort(rng.uniform(0, 40, n))
        gp = GP(_hyper_kernel(), mean=0.1, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True)
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
    else:
        x = rng.uniform(0, 4, (n, 3))
        k = 1.5 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3)
        gp = GP(k, mean=-0.3, fit_mean=True, white_noise=np.log(0.03), fit_white_noise=True)
        y = np.sin(x[:, 0]) * np.cos(x[:, 1]) + 0.2 * rng.randn(n)
    yerr = 0.1 + 0.05 * rng.rand(n)
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector()
    vec = np.vstack([p0 + 1e-3 * rng.randn(32, len(p0)), p0 + 0.3 * rng.randn(4, len(p0))])
    return gp, y, vec


def _one(gp, v, y):
    """the one-problem path at v: (log-likelihood, gh_chol_compute's logdet, gh_chol_objective's quad, sigma, r)"""
    gp.set_parameter_vector(v)
    ll = gp.log_likelihood(y, quiet=True)
    logdet = gp.solver.log_determinant
    sigma = np.sqrt(gp._yerr2 + np.exp(gp._call_white_noise(gp._x)))
    r = y - gp._call_mean(gp._x)
    s = BasicSolver(gp.kernel)
    _, quad, _, _, _ = s.objective(gp._x, sigma, r, want_grad=False)
    return ll, logdet, quad


def _raw(gp, vec, y):
    kp, sigma, r, ok = gp._batch_inputs(vec, y, quiet=True)
    return BasicSolver(gp.kernel).objective_batch(kp, gp._x, sigma, r)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["expsq", "hyper", "matern3d"])
@pytest.mark.parametrize("n", [50, 468, 1024, 2048])
def test_batch_matches_the_one_problem_path(kind, n):
    gp, y, vec = _problem(kind, n)
    p0 = gp.get_parameter_vector()
    ll = gp.log_likelihood_batch(vec, y)
    logdet, quad, info = _raw(gp, vec, y)
    assert (info == 0).all()
    for b in range(len(vec)):
        ll1, ld1, q1 = _one(gp, vec[b], y)
        assert logdet[b] == ld1, (b, logdet[b], ld1)                     # bit for bit
        assert abs(quad[b] - q1) <= 1e-10 * abs(q1), (b, quad[b], q1)
        assert abs(ll[b] - ll1) <= 1e-12 * abs(ll1), (b, ll[b], ll1)
    gp.set_parameter_vector(p0)


@pytest.mark.gpu
def test_batch_against_numpy():
    for kind in ("expsq", "hyper", "matern3d"):
        gp, y, vec = _problem(kind, 300, seed=7)
        kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
        logdet, quad, info = BasicSolver(gp.kernel).objective_batch(kp, gp._x, sigma, r)
        for b in (0, 5, 33):
            gp.set_parameter_vector(vec[b])
            K = gp.kernel.get_value(gp._x) + np.diag(sigma[b] ** 2)
            s, ld = np.linalg.slogdet(K)
            q = r[b] @ np.linalg.solve(K, r[b])
            assert s > 0 and abs(logdet[b] - ld) <= 1e-11 * abs(ld), (kind, b, logdet[b], ld)
            assert abs(quad[b] - q) <= 1e-11 * abs(q), (kind, b, quad[b], q)


def _singular_member(gp):
    """a parameter vector (1-D ExpSquared GP with fitted white noise, yerr = 0) whose matrix is numerically singular"""
    v = gp.get_parameter_vector().copy()
    names = gp.get_parameter_names()
    v[names.index("white_noise:value")] = -300.0
    v[names.index("kernel:k2:metric:log_M_0_0")] = np.log(1e8)
    return v


@pytest.mark.gpu
def test_batch_invariance():
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0, 10, 300))
    y = np.sin(x) + 0.1 * rng.randn(300)
    gp = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8), white_noise=np.log(0.02), fit_white_noise=True)
    gp.compute(x, 0.0)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(36, len(p0))
    ref = _raw(gp, vec, y)
    for b in (0, 17, 35):
        one = _raw(gp, vec[b:b + 1], y)
        assert one[0][0] == ref[0][b] and one[1][0] == ref[1][b]
    rev = _raw(gp, vec[::-1], y)
    assert np.array_equal(rev[0][::-1], ref[0]) and np.array_equal(rev[1][::-1], ref[1])
    saved = BasicSolver.BATCH_MAX_BYTES
    try:
        BasicSolver.BATCH_MAX_BYTES = 5 * (512 ** 2 + 384 * 128) * 8        # chunks of five members
        ch = _raw(gp, vec, y)
    finally:
        BasicSolver.BATCH_MAX_BYTES = saved
    assert np.array_equal(ch[0], ref[0]) and np.array_equal(ch[1], ref[1])
    bad = vec.copy()
    bad[3] = _singular_member(gp)
    bad[4, -1] = np.nan
    out = _raw(gp, bad, y)
    assert out[2][3] > 0 and out[2][4] > 0
    keep = np.ones(36, bool)
    keep[[3, 4]] = False
    assert np.array_equal(out[0][keep], ref[0][keep]) and np.array_equal(out[1][keep], ref[1][keep])
    assert (out[2][keep] == 0).all()


@pytest.mark.gpu
def test_batch_failures():
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 10, 300))
    y = np.sin(x) + 0.1 * rng.randn(300)
    gp = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8), white_noise=np.log(0.02), fit_white_noise=True)
    gp.compute(x, 0.0)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(8, len(p0))
    good = gp.log_likelihood_batch(vec, y)
    bad = vec.copy()
    bad[2] = _singular_member(gp)
    bad[5, 0] = np.nan
    ll = gp.log_likelihood_batch(bad, y)
    assert ll[2] == -np.inf and ll[5] == -np.inf
    keep = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(ll[keep], good[keep])
    # info is gh_chol_info of the one-problem call
    _, _, info = _raw(gp, bad, y)
    gp.set_parameter_vector(bad[2])
    with pytest.raises(np.linalg.LinAlgError):
        gp.compute(x, 0.0)
    assert info[2] == N.lib.gh_chol_info(gp.solver._handle) and info[2] > 0
    gp.set_parameter_vector(p0)
    gp.compute(x, 0.0)
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.log_likelihood_batch(bad, y, quiet=False)


@pytest.mark.gpu
def test_gp_state_is_unchanged():
    gp, y, vec = _problem("hyper", 468, seed=3)
    p = gp.get_parameter_vector().copy()
    a0 = gp.apply_inverse(y)
    assert gp.computed
    gp.log_likelihood_batch(vec, y)
    assert np.array_equal(gp.get_parameter_vector(), p) and gp.computed
    assert np.array_equal(gp.apply_inverse(y), a0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
def test_c_abi_host_and_device_pointers():
    import torch
    gp, y, vec = _problem("expsq", 500, seed=9)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    x = gp._x
    dk = DeviceKernel(gp.kernel)
    B, n = kp.shape[0], len(x)
    h = N._vp()
    N.check(N.lib.gh_chol_create(C.byref(N.gh_chol_opts(0, 0, 0, 1)), C.byref(h)))
    try:
        ld, q, info = np.empty(B), np.empty(B), np.empty(B, dtype=np.int64)
        assert N.lib.gh_chol_objective_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r),
                                             N.ptr(ld), N.ptr(q), N.ptr(info)) == N.GH_OK
        dld, dq = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
        dinfo = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        assert N.lib.gh_chol_objective_batch(h, dk.handle, N.ptr(_dev(kp)), B, N.ptr(_dev(x)), n, 1, N.ptr(_dev(sigma)),
                                             N.ptr(_dev(r)), N.ptr(dld), N.ptr(dq), N.ptr(dinfo)) == N.GH_OK
        torch.cuda.synchronize()
        assert np.array_equal(dld.cpu().numpy(), ld) and np.array_equal(dq.cpu().numpy(), q)
        assert np.array_equal(dinfo.cpu().numpy(), info) and (info == 0).all()
        # B = 0 is a no-op; a wrong ndim is GH_ERR_DIM
        z = np.full(1, 7.0)
        assert N.lib.gh_chol_objective_batch(h, dk.handle, N.ptr(kp), 0, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r),
                                             N.ptr(z), N.ptr(z), N.ptr(info)) == N.GH_OK and z[0] == 7.0
        assert N.lib.gh_chol_objective_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 2, N.ptr(sigma), N.ptr(r),
                                             N.ptr(ld), N.ptr(q), N.ptr(info)) == N.GH_ERR_DIM
        assert N.lib.gh_chol_objective_batch(h, dk.handle, N.ptr(kp), -1, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r),
                                             N.ptr(ld), N.ptr(q), N.ptr(info)) == N.GH_ERR_BAD_ARG
    finally:
        N.lib.gh_chol_destroy(h)


@pytest.mark.gpu
def test_steady_state_and_speed():
    gp, y, vec = _problem("expsq", 1024, seed=1)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    s = BasicSolver(gp.kernel)
    sizes = []
    for _ in range(5):
        s.objective_batch(kp, gp._x, sigma, r)
        sizes.append(int(N.lib.gh_chol_device_bytes(s._bhandle)))
    assert len(set(sizes[1:])) == 1 and sizes[1] > 0, sizes
    p0 = gp.get_parameter_vector()

    def loop():
        for v in vec:
            gp.set_parameter_vector(v)
            gp.log_likelihood(y)
        gp.set_parameter_vector(p0)

    tb, tl = [], []
    gp.log_likelihood_batch(vec, y)
    loop()
    for _ in range(5):
        t0 = time.perf_counter()
        gp.log_likelihood_batch(vec, y)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tl.append(t2 - t1)
    assert np.median(tl) >= 4.0 * np.median(tb), (np.median(tl), np.median(tb))
