"""GP.nll_and_grad_batch / grad_log_likelihood_batch / gh_chol_objective_grad_batch on the MI355X: B likelihoods and their
gradients in one device call, against the CPU reference of tests/grad_ref.py and the one-problem nll_and_grad under its
tolerance rule, bit for bit against gh_chol_objective_batch (logdet, info) and against itself (masks, batch position,
batch-mates, chunks), and for failures, priors, GP state, the loop routes, the C ABI, steady-state memory and speed."""
import ctypes as C
import copy
import time

import numpy as np
import pytest

import grad_ref as R
from george_amd import GP, BasicSolver, HODLRSolver, kernels
from george_amd import _native as N
from george_amd.modeling import ConstantModel
from george_amd.program import DeviceKernel

pytestmark = pytest.mark.gpu


def _hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _gp_kernel():
    # the GP-layer kernel of test_gpu_grad_reference.py: 1-D, six parameters, a product of sums
    return ((kernels.ConstantKernel(log_constant=np.log(0.5)) + kernels.ExpSquaredKernel(0.8))
            * kernels.RationalQuadraticKernel(log_alpha=np.log(1.5), metric=0.9)
            + kernels.ConstantKernel(log_constant=np.log(0.3)) * kernels.CosineKernel(log_period=0.5))


def _problem(kind, n, B, seed=0, **gp_kw):
    """(gp computed at its initial vector, y, vectors (B, len(gp)): walkers around the point, and for B >= 8 four of them
    farther out).  Mean and white noise are fitted constants."""
    rng = np.random.RandomState(seed + n + 3 * B)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        gp = GP(1.3 * kernels.ExpSquaredKernel(0.8), mean=0.2, fit_mean=True, white_noise=np.log(0.02),
                fit_white_noise=True, **gp_kw)
        y = np.sin(x) + 0.2 * rng.randn(n)
    elif kind == "hyper":
        x = np.sort(rng.uniform(0, 40, n))
        gp = GP(_hyper_kernel(), mean=0.1, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True, **gp_kw)
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
    elif kind == "matern3d":
        x = rng.uniform(0, 4, (n, 3))
        k = 1.5 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3)
        gp = GP(k, mean=-0.3, fit_mean=True, white_noise=np.log(0.03), fit_white_noise=True, **gp_kw)
        y = np.sin(x[:, 0]) * np.cos(x[:, 1]) + 0.2 * rng.randn(n)
    else:
        x = np.sort(rng.uniform(0.0, 4.0, n))
        k = _gp_kernel()
        k.freeze_parameter(k.get_parameter_names(include_frozen=True)[2])
        gp = GP(k, mean=0.3, fit_mean=True, white_noise=np.log(0.02), fit_white_noise=True, **gp_kw)
        y = np.sin(3.0 * x) + 0.3 * rng.randn(n)
    yerr = (0.1 + 0.05 * rng.rand(n)) * max(1.0, np.sqrt(n / 300.0))
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-3 * rng.randn(B, len(p0))
    if B >= 8:
        vec[-4:] = p0 + 0.1 * rng.randn(4, len(p0))
    return gp, y, vec


def _member_kernel(gp, row):
    k = copy.deepcopy(gp.kernel)
    k.set_parameter_vector(row, include_frozen=True)
    return k


def _expected(gp, vec_b, ref, wn):
    """the GP-level gradient from the reference's alpha / diag(A) / kernel block (gp.py:443-466), and its tolerance"""
    n = len(gp._x)
    m = gp.kernel.unfrozen_mask
    expect = np.concatenate([[np.sum(ref.alpha)], [0.5 * np.sum(np.exp(wn) * ref.diagA)], ref.g[m]])
    tol = np.concatenate([[n * ref.tol_alpha()], [0.5 * n * np.exp(wn) * ref.tol_diagA()], ref.tol_grad()[m]])
    return expect, tol


# A covering set over (kernel, N, B): every value of each axis appears, and every kernel at two sizes at least.
CASES = [
    ("expsq", 1, 3), ("expsq", 468, 36), ("expsq", 4097, 1),
    ("hyper", 2, 36), ("hyper", 129, 1), ("hyper", 468, 3),
    ("matern3d", 127, 36), ("matern3d", 1024, 3),
    ("gpk", 128, 3), ("gpk", 1024, 1),
]


@pytest.mark.parametrize("kind,n,B", CASES)
def test_against_the_cpu_reference(kind, n, B):
    gp, y, vec = _problem(kind, n, B)
    kp, sigma, r, ok = gp._batch_inputs(vec, y, quiet=True)
    assert ok.all()
    P = kp.shape[1]
    logdet, quad, g, alpha, diagA, info = BasicSolver(gp.kernel).objective_grad_batch(kp, gp._x, sigma, r)
    assert g.shape == (B, P) and alpha.shape == diagA.shape == (B, n) and (info == 0).all()
    G = gp.grad_log_likelihood_batch(vec, y)
    nll, G2 = gp.nll_and_grad_batch(vec, y)
    assert G.shape == (B, len(gp)) and np.array_equal(G2, -G)
    names = gp.get_parameter_names()
    for b in sorted({0, B // 2, B - 1}):
        ref = R.reference(_member_kernel(gp, kp[b]), gp._x, sigma[b], r[b])
        ratios = (ref.ratio_grad(g[b]), ref.ratio_alpha(alpha[b]), ref.ratio_diagA(diagA[b]), ref.ratio_logdet(logdet[b]),
                  ref.ratio_quad(quad[b]))
        assert max(ratios) <= 1.0, (b, ratios)
        expect, tol = _expected(gp, vec[b], ref, vec[b][names.index("white_noise:value")])
        assert ref._ratio(G[b] - expect, tol) <= 1.0, b
        ll_ref = -0.5 * (ref.quad + ref.logdet + n * np.log(2 * np.pi))
        assert abs(-nll[b] - ll_ref) <= 0.5 * (ref.tol_quad() + ref.tol_logdet())


@pytest.mark.parametrize("kind", ["expsq", "hyper", "matern3d", "gpk"])
def test_agrees_with_the_one_problem_path(kind):
    gp, y, vec = _problem(kind, 300, 5, seed=2)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    nll, G = gp.nll_and_grad_batch(vec, y)
    s = BasicSolver(gp.kernel)
    logdet, quad, _, _, _, info = s.objective_grad_batch(kp, gp._x, sigma, r)
    logdet0, quad0, info0 = s.objective_batch(kp, gp._x, sigma, r)
    assert np.array_equal(logdet, logdet0) and np.array_equal(info, info0)
    names = gp.get_parameter_names()
    p0 = gp.get_parameter_vector()
    for b, v in enumerate(vec):
        ref = R.reference(_member_kernel(gp, kp[b]), gp._x, sigma[b], r[b])
        assert abs(quad[b] - quad0[b]) <= ref.tol_quad()
        expect, tol = _expected(gp, v, ref, v[names.index("white_noise:value")])
        gp.kernel.dirty = True
        nll1, g1 = gp.nll_and_grad(v, y)
        # both against the reference under its rule, and against each other under twice the rule
        assert ref._ratio(-g1 - expect, tol) <= 1.0 and ref._ratio(-G[b] - expect, tol) <= 1.0
        assert ref._ratio(G[b] - g1, 2 * tol) <= 1.0
        assert abs(nll[b] - nll1) <= ref.tol_quad() + ref.tol_logdet()
    gp.set_parameter_vector(p0)


def test_masks_give_exact_zeros():
    gp, y, vec = _problem("hyper", 500, 6, seed=4)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    s = BasicSolver(gp.kernel)
    full = s.objective_grad_batch(kp, gp._x, sigma, r)
    P = kp.shape[1]
    which = np.ones(P, dtype=np.uint32)
    which[[0, 3, P - 1]] = 0
    part = s.objective_grad_batch(kp, gp._x, sigma, r, which)
    assert (part[2][:, which == 0] == 0).all()
    assert np.array_equal(part[2][:, which == 1], full[2][:, which == 1])
    for a, b in zip(part[:2] + part[3:], full[:2] + full[3:]):
        assert np.array_equal(a, b)


def _const_expsq(n=300, seed=11):
    rng = np.random.RandomState(seed)
    x = np.sort(rng.uniform(0, 10, n))
    y = np.sin(x) + 0.1 * rng.randn(n)
    gp = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8), mean=0.1, fit_mean=True, white_noise=np.log(0.02),
            fit_white_noise=True)
    gp.compute(x, 0.0)
    return gp, x, y, rng


def _singular_member(gp):
    """a parameter vector (1-D ExpSquared GP with fitted white noise, yerr = 0) whose matrix is numerically singular"""
    v = gp.get_parameter_vector().copy()
    names = gp.get_parameter_names()
    v[names.index("white_noise:value")] = -300.0
    v[names.index("kernel:k2:metric:log_M_0_0")] = np.log(1e8)
    return v


def test_batch_invariance(monkeypatch):
    gp, x, y, rng = _const_expsq()
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(36, len(p0))
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    s = BasicSolver(gp.kernel)
    out = s.objective_grad_batch(kp, gp._x, sigma, r)
    rev = s.objective_grad_batch(kp[::-1], gp._x, sigma[::-1], r[::-1])
    alone = s.objective_grad_batch(kp[7:8], gp._x, sigma[7:8], r[7:8])
    for a, b, c in zip(out, rev, alone):
        assert np.array_equal(a, b[::-1]) and np.array_equal(a[7:8], c)
    nll, G = gp.nll_and_grad_batch(vec, y)
    # chunks of two members
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_BYTES", 2 * BasicSolver.grad_batch_bytes(len(x)) + 1)
    for a, b in zip(out, s.objective_grad_batch(kp, gp._x, sigma, r)):
        assert np.array_equal(a, b)
    nll_c, G_c = gp.nll_and_grad_batch(vec, y)
    assert np.array_equal(nll, nll_c) and np.array_equal(G, G_c)


def test_failed_members_and_priors():
    gp, x, y, rng = _const_expsq(seed=5)
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(8, len(p0))
    nll0, G0 = gp.nll_and_grad_batch(vec, y)
    bad = vec.copy()
    bad[2] = _singular_member(gp)
    nll, G = gp.nll_and_grad_batch(bad, y)
    assert nll[2] == np.inf and (G[2] == 0).all()
    keep = [0, 1, 3, 4, 5, 6, 7]
    assert np.array_equal(nll[keep], nll0[keep]) and np.array_equal(G[keep], G0[keep])
    Gl = gp.grad_log_likelihood_batch(bad, y)
    assert (Gl[2] == 0).all() and np.array_equal(Gl[keep], -G0[keep])
    # the per-vector path agrees
    gp.set_parameter_vector(bad[2])
    assert gp.nll_and_grad(bad[2], y)[0] == np.inf
    gp.set_parameter_vector(p0)
    gp.compute(x, 0.0)
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.nll_and_grad_batch(bad, y, quiet=False)
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.grad_log_likelihood_batch(bad, y, quiet=False)
    # a row outside the prior: (inf, 0) and not evaluated; errors keep naming the caller's rows
    gp2 = GP(copy.deepcopy(gp.kernel), mean=ConstantModel(0.1, bounds=dict(value=(-1.0, 1.0))), white_noise=np.log(0.02),
             fit_white_noise=True)
    gp2.compute(x, 0.0)
    out = bad.copy()
    out[1, 0] = 5.0
    nll_o, G_o = gp2.nll_and_grad_batch(out, y)
    assert nll_o[1] == np.inf and (G_o[1] == 0).all()
    rest = [0, 3, 4, 5, 6, 7]
    assert np.array_equal(nll_o[rest], nll[rest]) and np.array_equal(G_o[rest], G[rest])
    assert gp2.nll_and_grad(out[1], y)[0] == np.inf
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp2.nll_and_grad_batch(out, y, quiet=False)


def test_gp_state_is_unchanged():
    gp, y, vec = _problem("hyper", 468, 12, seed=3)
    p = gp.get_parameter_vector().copy()
    ll0 = gp.log_likelihood(y)
    mu0, var0 = gp.predict(y, gp._x[::7, 0], return_var=True)
    alpha, yc, obj = gp._alpha, gp._y, gp._obj_cache
    solver, h = gp.solver, gp.solver._handle.value
    gp.nll_and_grad_batch(vec, y)
    gp.grad_log_likelihood_batch(vec, y)
    assert np.array_equal(gp.get_parameter_vector(), p) and gp.computed
    assert gp.solver is solver and gp.solver._handle.value == h
    assert gp._alpha is alpha and gp._y is yc and gp._obj_cache is obj
    mu1, var1 = gp.predict(y, gp._x[::7, 0], return_var=True)
    assert gp.log_likelihood(y) == ll0 and np.array_equal(mu1, mu0) and np.array_equal(var1, var0)


def _loop(gp, vec, y):
    p0 = gp.get_parameter_vector()
    out = [gp.nll_and_grad(v, y) for v in vec]
    gp.set_parameter_vector(p0)
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def test_hodlr_goes_through_the_loop_exactly():
    gp, y, vec = _problem("expsq", 400, 4, seed=8, solver=HODLRSolver)
    nll, G = gp.nll_and_grad_batch(vec, y)
    G2 = gp.grad_log_likelihood_batch(vec, y)
    nll_l, G_l = _loop(gp, vec, y)
    assert np.array_equal(nll, nll_l) and np.array_equal(G, G_l)
    p0 = gp.get_parameter_vector()
    for b, v in enumerate(vec):
        gp.set_parameter_vector(v)
        assert np.array_equal(G2[b], gp.grad_log_likelihood(y, quiet=True))
    gp.set_parameter_vector(p0)


def test_large_n_goes_through_the_loop_exactly(monkeypatch):
    gp, y, vec = _problem("expsq", 700, 3, seed=9)
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 512)
    assert not gp._grad_batch_on_device()
    nll, G = gp.nll_and_grad_batch(vec, y)
    nll_l, G_l = _loop(gp, vec, y)
    assert np.array_equal(nll, nll_l) and np.array_equal(G, G_l)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_c_abi_host_and_device_pointers():
    import torch
    gp, y, vec = _problem("gpk", 500, 6, seed=9)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    x = gp._x
    dk = DeviceKernel(gp.kernel)
    B, n, P = kp.shape[0], len(x), kp.shape[1]
    which = np.ones(P, dtype=np.uint32)
    h = N._vp()
    N.check(N.lib.gh_chol_create(C.byref(N.gh_chol_opts(0, 0, 0, 1)), C.byref(h)))
    f = N.lib.gh_chol_objective_grad_batch
    try:
        ld, q, g, a, d = np.empty(B), np.empty(B), np.empty((B, P)), np.empty((B, n)), np.empty((B, n))
        info = np.empty(B, dtype=np.int64)
        assert f(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(which), N.ptr(ld), N.ptr(q),
                 N.ptr(g), N.ptr(a), N.ptr(d), N.ptr(info)) == N.GH_OK
        dev = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((B,), (B,), (B, P), (B, n), (B, n))]
        dinfo = torch.full((B,), -1, dtype=torch.int64, device="cuda")
        assert f(h, dk.handle, N.ptr(_dev(kp)), B, N.ptr(_dev(x)), n, 1, N.ptr(_dev(sigma)), N.ptr(_dev(r)),
                 N.ptr(_dev(which)), *[N.ptr(t) for t in dev], N.ptr(dinfo)) == N.GH_OK
        torch.cuda.synchronize()
        for t, ref in zip(dev + [dinfo], (ld, q, g, a, d, info)):
            assert np.array_equal(t.cpu().numpy(), ref)
        assert (info == 0).all()
        # NULL alpha / diagA
        ld2, q2, g2 = np.empty(B), np.empty(B), np.empty((B, P))
        assert f(h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(which), N.ptr(ld2), N.ptr(q2),
                 N.ptr(g2), None, None, N.ptr(info)) == N.GH_OK
        assert np.array_equal(ld2, ld) and np.array_equal(q2, q) and np.array_equal(g2, g)
        # bad arguments: B < 0, no mask, no grad, no residual; the wrong dimension
        args = [h, dk.handle, N.ptr(kp), B, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(which), N.ptr(ld), N.ptr(q),
                N.ptr(g), None, None, N.ptr(info)]
        for pos, val in ((3, -1), (9, None), (12, None), (8, None), (5, 0)):
            bad = list(args)
            bad[pos] = val
            assert f(*bad) == N.GH_ERR_BAD_ARG, pos
        bad = list(args)
        bad[6] = 2
        assert f(*bad) == N.GH_ERR_DIM
        # B = 0 writes nothing
        z = np.full(1, 7.0)
        assert f(h, dk.handle, N.ptr(kp), 0, N.ptr(x), n, 1, N.ptr(sigma), N.ptr(r), N.ptr(which), N.ptr(z), N.ptr(z),
                 N.ptr(z), None, None, N.ptr(info)) == N.GH_OK and z[0] == 7.0
    finally:
        N.lib.gh_chol_destroy(h)


def test_steady_state_and_trim():
    gp, y, vec = _problem("expsq", 1024, 36, seed=1)
    kp, sigma, r, _ = gp._batch_inputs(vec, y, quiet=True)
    s = BasicSolver(gp.kernel)
    sizes = []
    for _ in range(5):
        s.objective_grad_batch(kp, gp._x, sigma, r)
        sizes.append(int(N.lib.gh_chol_device_bytes(s._bhandle)))
    per = BasicSolver.grad_batch_bytes(1024)
    assert len(set(sizes[1:])) == 1 and sizes[1] >= 36 * per * 0.9, sizes
    N.lib.gh_chol_trim(s._bhandle)
    assert int(N.lib.gh_chol_device_bytes(s._bhandle)) <= sizes[-1] - 36 * per * 0.9


def test_speed_floor_at_the_hyper_rst_shape():
    gp, y, vec = _problem("expsq", 468, 36, seed=6)
    p0 = gp.get_parameter_vector()

    def loop():
        for v in vec:
            gp.nll_and_grad(v, y)
        gp.set_parameter_vector(p0)

    gp.nll_and_grad_batch(vec, y)
    loop()
    tb, tl = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        gp.nll_and_grad_batch(vec, y)
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tl.append(t2 - t1)
    assert np.median(tl) >= 4.0 * np.median(tb), (np.median(tl), np.median(tb))
