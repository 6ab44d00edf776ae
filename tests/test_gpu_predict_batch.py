"""GP.predict_batch / gh_chol_predict_batch on the MI355X: B posterior predictions of one kernel structure in one device
call, against the CPU reference of tests/predict_ref.py and the one-problem predict under its tolerance rule, bit for bit
against gh_chol_objective_batch and against itself (batch position, batch-mates, chunks), and for failures, GP state, the
C ABI and steady-state behaviour."""
import ctypes as C
import time

import numpy as np
import pytest

import predict_ref as R
from george_amd import GP, BasicSolver, HODLRSolver, kernels
from george_amd import _native as N
from george_amd.program import DeviceKernel


def _hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _problem(kind, n, m, B, seed=0, **gp_kw):
    """(gp computed at its initial vector, y, test points (m, ndim) or (m,), vectors (B, len(gp)): walkers around the
    point, and for B >= 8 four of them far apart)"""
    rng = np.random.RandomState(seed + n + 7 * m)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        t = np.linspace(-0.5, 10.5, m)
        gp = GP(1.3 * kernels.ExpSquaredKernel(0.8), mean=0.2, fit_mean=True, white_noise=np.log(0.02),
                fit_white_noise=True, **gp_kw)
        y = np.sin(x) + 0.2 * rng.randn(n)
    elif kind == "hyper":
        x = np.sort(rng.uniform(0, 40, n))
        t = np.linspace(-1.0, 41.0, m)
        gp = GP(_hyper_kernel(), mean=0.1, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True, **gp_kw)
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
    else:
        x = rng.uniform(0, 4, (n, 3))
        t = rng.uniform(-0.2, 4.2, (m, 3))
        k = 1.5 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3)
        gp = GP(k, mean=-0.3, fit_mean=True, white_noise=np.log(0.03), fit_white_noise=True, **gp_kw)
        y = np.sin(x[:, 0]) * np.cos(x[:, 1]) + 0.2 * rng.randn(n)
    yerr = 0.1 + 0.05 * rng.rand(n)
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-3 * rng.randn(B, len(p0))
    if B >= 8:
        vec[-4:] = p0 + 0.3 * rng.randn(4, len(p0))
    return gp, y, t, vec


def _xs(gp, t):
    return np.ascontiguousarray(gp.parse_samples(t), dtype=np.float64)


# A covering set over (kernel, return mode, N, M, B): every value of each axis appears, and every kernel in every mode.
CASES = [
    ("expsq", "mean", 1, 1, 3),
    ("expsq", "var", 4097, 129, 1),
    ("expsq", "cov", 128, 250, 3),
    ("hyper", "mean", 468, 250, 3),
    ("hyper", "var", 129, 500, 3),
    ("hyper", "cov", 50, 127, 36),
    ("matern3d", "mean", 1024, 128, 3),
    ("matern3d", "var", 127, 1, 36),
    ("matern3d", "cov", 1024, 129, 1),
]


def _call(gp, vec, y, t, mode, **kw):
    if mode == "mean":
        return gp.predict_batch(vec, y, t, return_cov=False, **kw), None
    if mode == "var":
        return gp.predict_batch(vec, y, t, return_var=True, **kw)
    return gp.predict_batch(vec, y, t, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,mode,n,m,B", CASES)
def test_against_the_cpu_reference(kind, mode, n, m, B):
    gp, y, t, vec = _problem(kind, n, m, B)
    mu, second = _call(gp, vec, y, t, mode)
    assert mu.shape == (B, m)
    assert second is None or second.shape == ((B, m) if mode == "var" else (B, m, m))
    members = sorted({0, B // 2, B - 1})
    ref = R.batch_reference(gp, vec, y, _xs(gp, t), members=members)
    for b in members:
        assert ref[b].ratio_mu(mu[b]) <= 1.0, (b, ref[b].ratio_mu(mu[b]))
        if mode == "var":
            assert ref[b].ratio_var(second[b]) <= 1.0, (b, ref[b].ratio_var(second[b]))
        if mode == "cov":
            assert ref[b].ratio_cov(second[b]) <= 1.0, (b, ref[b].ratio_cov(second[b]))
            assert np.array_equal(second[b], second[b].T)                        # exactly symmetric


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["expsq", "hyper", "matern3d"])
def test_agrees_with_the_one_problem_predict(kind):
    gp, y, t, vec = _problem(kind, 300, 150, 5, seed=2)
    xs = _xs(gp, t)
    mu, cov = gp.predict_batch(vec, y, t)
    mu_v, var = gp.predict_batch(vec, y, t, return_var=True)
    ref = R.batch_reference(gp, vec, y, xs)
    p0 = gp.get_parameter_vector()
    for b, v in enumerate(vec):
        gp.set_parameter_vector(v)
        mu1, cov1 = gp.predict(y, t)
        # both against the reference under its rule, and against each other under twice the rule
        assert ref[b].ratio_mu(mu1) <= 1.0 and ref[b].ratio_cov(cov1) <= 1.0
        assert ref[b]._ratio(mu[b] - mu1, 2 * ref[b].tol_mu()) <= 1.0
        assert ref[b]._ratio(cov[b] - cov1, 2 * ref[b].tol_cov()) <= 1.0
        assert np.array_equal(mu_v[b], mu[b]) and np.array_equal(var[b], np.diag(cov[b]))
    gp.set_parameter_vector(p0)


def _raw(gp, vec, y, t, var=False, cov=False, handle=None):
    """gh_chol_predict_batch through the C ABI: (mu, var, cov, logdet, quad, info)"""
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    xs = _xs(gp, t)
    B, n, m = len(vec), len(gp._x), len(xs)
    dk = DeviceKernel(gp.kernel)
    mu, logdet, quad, info = np.empty((B, m)), np.empty(B), np.empty(B), np.empty(B, dtype=np.int64)
    v = np.empty((B, m)) if var else None
    c = np.empty((B, m, m)) if cov else None
    h = handle or N._vp()
    if handle is None:
        N.check(N.lib.gh_chol_create(C.byref(N.gh_chol_opts(0, 0, 0, 1)), C.byref(h)))
    try:
        N.check(N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), B, N.ptr(gp._x), n, gp._x.shape[1], N.ptr(sigma),
                                            N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(v), N.ptr(c), N.ptr(logdet),
                                            N.ptr(quad), N.ptr(info)))
    finally:
        if handle is None:
            N.lib.gh_chol_destroy(h)
    return mu, v, c, logdet, quad, info


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("expsq", 468), ("hyper", 1024), ("matern3d", 129)])
def test_logdet_and_quad_are_those_of_the_objective_bit_for_bit(kind, n):
    gp, y, t, vec = _problem(kind, n, 130, 6, seed=4)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    ld0, q0, info0 = BasicSolver(gp.kernel).objective_batch(kp, gp._x, sigma, r)
    for var, cov in ((False, False), (True, False), (False, True)):
        _, _, _, ld, q, info = _raw(gp, vec, y, t, var=var, cov=cov)
        assert np.array_equal(ld, ld0) and np.array_equal(q, q0) and np.array_equal(info, info0)


def _singular_member(gp):
    """a parameter vector (1-D ExpSquared GP with fitted white noise, yerr = 0) whose matrix is numerically singular"""
    v = gp.get_parameter_vector().copy()
    names = gp.get_parameter_names()
    v[names.index("white_noise:value")] = -300.0
    v[names.index("kernel:k2:metric:log_M_0_0")] = np.log(1e8)
    return v


def _const_expsq(n=300, seed=11):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0, 10, n))
    y = np.sin(x) + 0.1 * rng.randn(n)
    gp = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8), white_noise=np.log(0.02), fit_white_noise=True)
    gp.compute(x, 0.0)
    return gp, x, y, rng


@pytest.mark.gpu
def test_batch_invariance(monkeypatch):
    gp, x, y, rng = _const_expsq()
    t = np.linspace(0, 10, 200)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(36, len(p0))
    ref = gp.predict_batch(vec, y, t)
    for b in (0, 17, 35):
        one = gp.predict_batch(vec[b:b + 1], y, t)
        assert np.array_equal(one[0][0], ref[0][b]) and np.array_equal(one[1][0], ref[1][b])
    rev = gp.predict_batch(vec[::-1], y, t)
    assert np.array_equal(rev[0][::-1], ref[0]) and np.array_equal(rev[1][::-1], ref[1])
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_BYTES", 5 * BasicSolver.predict_batch_bytes(300, 200, False, True))
    ch = gp.predict_batch(vec, y, t)                                           # chunks of five members
    assert np.array_equal(ch[0], ref[0]) and np.array_equal(ch[1], ref[1])


@pytest.mark.gpu
def test_failed_members(monkeypatch):
    gp, x, y, rng = _const_expsq(seed=5)
    t = np.linspace(0, 10, 130)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(8, len(p0))
    good = gp.predict_batch(vec, y, t, return_var=True)
    bad = vec.copy()
    bad[2] = _singular_member(gp)
    bad[5, 0] = np.nan
    mu, var = gp.predict_batch(bad, y, t, return_var=True, quiet=True)
    assert np.isnan(mu[[2, 5]]).all() and np.isnan(var[[2, 5]]).all()
    keep = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(mu[keep], good[0][keep]) and np.array_equal(var[keep], good[1][keep])
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.predict_batch(bad, y, t, return_var=True)
    # the loop path reports the same member
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 0)
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.predict_batch(bad, y, t, return_var=True)
    mu_l, var_l = gp.predict_batch(bad, y, t, return_var=True, quiet=True)
    assert np.isnan(mu_l[[2, 5]]).all() and np.isfinite(mu_l[keep]).all()


@pytest.mark.gpu
def test_gp_state_is_unchanged():
    gp, y, t, vec = _problem("hyper", 468, 250, 12, seed=3)
    p = gp.get_parameter_vector().copy()
    mu0, cov0 = gp.predict(y, t)
    alpha, yc, obj = gp._alpha, gp._y, gp._obj_cache
    solver, h = gp.solver, gp.solver._handle.value
    for mode in ("mean", "var", "cov"):
        _call(gp, vec, y, t, mode)
        assert np.array_equal(gp.get_parameter_vector(), p) and gp.computed
        assert gp.solver is solver and gp.solver._handle.value == h
        assert gp._alpha is alpha and gp._y is yc and gp._obj_cache is obj
    mu1, cov1 = gp.predict(y, t)
    assert np.array_equal(mu1, mu0) and np.array_equal(cov1, cov0)


@pytest.mark.gpu
def test_hodlr_goes_through_the_loop_exactly():
    gp, y, t, vec = _problem("expsq", 400, 90, 4, seed=8, solver=HODLRSolver)
    p0 = gp.get_parameter_vector()
    mu, var = gp.predict_batch(vec, y, t, return_var=True)
    for b, v in enumerate(vec):
        gp.set_parameter_vector(v)
        mu1, var1 = gp.predict(y, t, return_var=True)
        assert np.array_equal(mu[b], mu1) and np.array_equal(var[b], var1)
    gp.set_parameter_vector(p0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
def test_c_abi_host_and_device_pointers():
    import torch
    gp, y, t, vec = _problem("expsq", 500, 140, 6, seed=9)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    x, xs = gp._x, _xs(gp, t)
    dk = DeviceKernel(gp.kernel)
    B, n, m = kp.shape[0], len(x), len(xs)
    h = N._vp()
    N.check(N.lib.gh_chol_create(C.byref(N.gh_chol_opts(0, 0, 0, 1)), C.byref(h)))
    try:
        mu, cov, info = np.empty((B, m)), np.empty((B, m, m)), np.empty(B, dtype=np.int64)
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(xs), m,
                                           N.ptr(mu), None, N.ptr(cov), None, None, N.ptr(info)) == N.GH_OK
        dmu = torch.empty((B, m), dtype=torch.float64, device="cuda")
        dcov = torch.empty((B, m, m), dtype=torch.float64, device="cuda")
        dinfo = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(_dev(kp)), B, N.ptr(_dev(x)), n, 1, N.ptr(_dev(sigma)),
                                           N.ptr(_dev(r)), N.ptr(_dev(xs)), m, N.ptr(dmu), None, N.ptr(dcov), None, None,
                                           N.ptr(dinfo)) == N.GH_OK
        torch.cuda.synchronize()
        assert np.array_equal(dmu.cpu().numpy(), mu) and np.array_equal(dcov.cpu().numpy(), cov)
        assert np.array_equal(dinfo.cpu().numpy(), info) and (info == 0).all()
        # xs of the wrong dimension, var and cov together, B < 0
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 2, N.ptr(sigma), N.ptr(r), N.ptr(xs),
                                           m, N.ptr(mu), None, None, None, None, N.ptr(info)) == N.GH_ERR_DIM
        v = np.empty((B, m))
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(xs),
                                           m, N.ptr(mu), N.ptr(v), N.ptr(cov), None, None, N.ptr(info)) == N.GH_ERR_BAD_ARG
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), -1, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(xs),
                                           m, N.ptr(mu), None, None, None, None, N.ptr(info)) == N.GH_ERR_BAD_ARG
        # B = 0 writes nothing; m = 0 still gives logdet and quad
        z = np.full(1, 7.0)
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), 0, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(xs),
                                           m, N.ptr(z), None, None, N.ptr(z), N.ptr(z), N.ptr(info)) == N.GH_OK and z[0] == 7.0
        ld, q = np.empty(B), np.empty(B)
        assert N.lib.gh_chol_predict_batch(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), None, 0,
                                           None, None, None, N.ptr(ld), N.ptr(q), N.ptr(info)) == N.GH_OK
        ld0, q0, _ = BasicSolver(gp.kernel).objective_batch(kp, x, sigma, r)
        assert np.array_equal(ld, ld0) and np.array_equal(q, q0)
    finally:
        N.lib.gh_chol_destroy(h)
    # the public entry points give empty outputs
    mu, cov = gp.predict_batch(np.zeros((0, len(gp))), y, t)
    assert mu.shape == (0, m) and cov.shape == (0, m, m)
    mu, var = gp.predict_batch(vec, y, np.zeros(0), return_var=True)
    assert mu.shape == (B, 0) and var.shape == (B, 0)


@pytest.mark.gpu
def test_steady_state_and_trim():
    gp, y, t, vec = _problem("expsq", 1024, 256, 36, seed=1)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    xs = _xs(gp, t)
    s = BasicSolver(gp.kernel)
    sizes = []
    for _ in range(5):
        s.predict_batch(kp, gp._x, sigma, r, xs, return_cov=True)
        sizes.append(int(N.lib.gh_chol_device_bytes(s._bhandle)))
    assert len(set(sizes[1:])) == 1 and sizes[1] >= 36 * BasicSolver.predict_batch_bytes(1024, 256, False, True) * 0.9, sizes
    N.lib.gh_chol_trim(s._bhandle)
    assert int(N.lib.gh_chol_device_bytes(s._bhandle)) <= sizes[-1] - 36 * BasicSolver.predict_batch_bytes(1024, 256) * 0.9


@pytest.mark.gpu
def test_speed_floor_at_the_hyper_rst_shape():
    gp, y, t, vec = _problem("expsq", 468, 250, 50, seed=6)
    p0 = gp.get_parameter_vector()

    def loop():
        for v in vec:
            gp.set_parameter_vector(v)
            gp.predict(y, t, return_var=True)
        gp.set_parameter_vector(p0)

    gp.predict_batch(vec, y, t, return_var=True)
    loop()
    tb, tl = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        gp.predict_batch(vec, y, t, return_var=True)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tl.append(t2 - t1)
    assert np.median(tl) >= 10.0 * np.median(tb), (np.median(tl), np.median(tb))       # measured: 44x
