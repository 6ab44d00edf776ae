"""The likelihood gradient on the device against the CPU reference of tests/grad_ref.py, at every parameter count.

The kernel part of the gradient, 1/2 sum_ij A_ij dK_ij/dtheta_p, comes from kgrad_reduce_kernel<PMAX>
(gh_kmat.hip), reached through gh_chol_grad (``BasicSolver.grad``) and gh_chol_objective
(``BasicSolver.objective``).  The host picks the instance from the parameter count P:

=====================================================  ==============================================
case                                                   instance
=====================================================  ==============================================
matrix P = 1, 4  (N = 1 ... 1000; P = 4 also 2049, 4097)  ``<4>``
matrix P = 5, 16 (N = 1 ... 1000; P = 16 also 2049, 4097) ``<16>``
matrix P = 17, 37, 64 (N = 1 ... 1000; P = 17 also 2049, 4097)  ``<64>``
masks P = 5 / 17, 64                                   ``<16>`` / ``<64>``
objective with grad = NULL, diagA != NULL              the instance of P (all-zero mask)
kernel zoo at N = 129                                  ``<4>`` (P <= 4) or ``<16>`` (P = 6, 7);
                                                       P = 0 runs the ``<4>`` instance for diag(A)
stack depth 8 (P = 20, ndim = 16)                      ``<64>``
GP layer (P = 6, one frozen)                           ``<16>``
=====================================================  ==============================================

Every comparison uses the one tolerance rule of grad_ref: ``|x - x_ref| <= C_TOL * u * kappa(K) * S``.  The tensor-API
tests at the end check gh_kernel_gradient_* and the coordinate gradients at P = 37 / 64 and ndim = 16 against
oracle.kernels_np."""
import ctypes as C

import numpy as np
import pytest

import grad_ref as R
import zoo
from george_amd import GP, BasicSolver
from george_amd.gp import TINY
from george_amd import _native as N
from george_amd import kernels as K
from george_amd.kernel_interface import KernelInterface
from george_amd.modeling import Model
from george_amd.program import DeviceKernel
from oracle import kernels_np, solver_np

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 129, 1000)
MATRIX = [(P, n) for P in sorted(R.PCASES) for n in SIZES] + [(P, n) for P in (4, 16, 17) for n in (2049, 4097)]
MARGINS = {}          # instance -> largest |error| / tolerance seen (printed at the end of the module with -s)


def _note(P, *ratios):
    inst = R.instance(P)
    MARGINS[inst] = max([MARGINS.get(inst, 0.0)] + list(ratios))


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    for inst in sorted(MARGINS):
        print("kgrad_reduce_kernel<%d>: largest |error| / tolerance %.3g" % (inst, MARGINS[inst]))


# ------------------------------------------------------------------ a. parameter count x size
@pytest.mark.parametrize("P,n", MATRIX, ids=["P%d-N%d" % c for c in MATRIX])
def test_gradient_matrix_against_reference(P, n):
    kernel, x, yerr, r = R.problem(P, n)
    ref = R.reference(kernel, x, yerr, r)
    assert ref.kappa <= 1e6
    which = np.ones(P, dtype=np.uint32)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    g, alpha, diagA = s.grad(r, which)
    ratios = (ref.ratio_grad(g), ref.ratio_alpha(alpha), ref.ratio_diagA(diagA))
    assert max(ratios) <= 1.0, ratios
    s2 = BasicSolver(kernel)
    logdet, quad, g2, alpha2, diagA2 = s2.objective(x, yerr, r, which, want_grad=True)
    ratios2 = (ref.ratio_grad(g2), ref.ratio_alpha(alpha2), ref.ratio_diagA(diagA2), ref.ratio_logdet(logdet),
               ref.ratio_quad(quad))
    assert max(ratios2) <= 1.0, ratios2
    _note(P, *(ratios + ratios2))


# ------------------------------------------------------------------ b. parameter masks
def _masks(P):
    alt = np.arange(P) % 2 == 0
    first, last = np.ones(P, bool), np.ones(P, bool)
    first[0] = False
    last[-1] = False
    return {"all": np.ones(P, bool), "none": np.zeros(P, bool), "first_frozen": first, "last_frozen": last,
            "alternating": alt}


@pytest.mark.parametrize("P", [5, 17, 64])
def test_masks_zero_frozen_entries_and_leave_the_rest_bitwise(P):
    kernel, x, yerr, r = R.problem(P, 129)
    ones = np.ones(P, dtype=np.uint32)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    g_all, a_all, d_all = s.grad(r, ones)
    _, _, go_all, ao_all, do_all = BasicSolver(kernel).objective(x, yerr, r, ones)
    for name, m in _masks(P).items():
        which = m.astype(np.uint32)
        g, a, d = s.grad(r, which)
        _, _, go, ao, do = BasicSolver(kernel).objective(x, yerr, r, which)
        for gg, gref, aa, aref, dd, dref in ((g, g_all, a, a_all, d, d_all), (go, go_all, ao, ao_all, do, do_all)):
            assert np.all(gg[~m] == 0.0), name
            assert np.array_equal(gg[m], gref[m]), name
            assert np.array_equal(dd, dref), name
            assert np.array_equal(aa, aref), name
    # the objective with grad = NULL and diagA != NULL: the reduction with an all-zero mask
    dk = DeviceKernel(kernel)
    n = len(x)
    h = N._vp()
    N.check(N.lib.gh_chol_create(C.byref(N.gh_chol_opts(0, 0, 0, 1)), C.byref(h)))
    try:
        logdet, quad = C.c_double(0.0), C.c_double(0.0)
        alpha, diagA = np.empty(n), np.empty(n)
        assert N.lib.gh_chol_objective(h, dk.handle, N.ptr(x), n, x.shape[1], N.ptr(yerr), N.ptr(r), None,
                                       C.byref(logdet), C.byref(quad), None, N.ptr(alpha), N.ptr(diagA)) == N.GH_OK
        assert np.array_equal(diagA, do_all)
        assert np.array_equal(alpha, ao_all)
    finally:
        N.lib.gh_chol_destroy(h)


@pytest.mark.parametrize("P", [5, 17, 64])
def test_frozen_parameters_through_the_gp(P):
    _, x, yerr, r = R.problem(P, 129)
    sigma = np.sqrt(yerr ** 2 + TINY)                 # the GP's default white noise is log(TINY)
    ref = R.reference(R.PCASES[P][0](K), x, sigma, r)
    for name, m in _masks(P).items():
        kernel = R.PCASES[P][0](K)
        names = kernel.get_parameter_names(include_frozen=True)
        for i in np.flatnonzero(~m):
            kernel.freeze_parameter(names[i])
        assert np.array_equal(kernel.unfrozen_mask, m)
        gp = GP(kernel)
        gp.compute(x, yerr)
        g = gp.grad_log_likelihood(r)                 # gh_chol_grad
        assert len(g) == int(m.sum()), name
        assert ref._ratio(g - ref.g[m], ref.tol_grad()[m]) <= 1.0, name
        gp2 = GP(kernel)
        gp2.compute(x, yerr)
        gp2.kernel.dirty = True                       # the next call refactorises through gh_chol_objective
        _, g2 = gp2.nll_and_grad(gp2.get_parameter_vector(), r)
        assert ref._ratio(-g2 - ref.g[m], ref.tol_grad()[m]) <= 1.0, name


# ------------------------------------------------------------------ c. every zoo kernel through the reduction
ZOO = zoo.kernel_zoo(K)


def _zoo_problem(kernel, n=129):
    rng = np.random.RandomState(129)
    x = rng.uniform(-2.0, 2.0, (n, kernel.ndim))
    x = x[np.argsort(x[:, 0])]
    K0 = solver_np.kernel_matrix(kernel, x)
    # noise against the largest eigenvalue (the non-stationary leaves get more of it), and against the most negative one
    # of the kernels that are not positive semi-definite (an ExpSine2 with gamma < 0)
    lmin = np.linalg.eigvalsh(K0)[0]
    yerr = np.full(n, np.sqrt(max(0.01, 1e-4 * np.linalg.norm(K0, 1)) + 2.0 * max(0.0, -lmin)))
    r = np.sin(2.0 * x.sum(axis=1)) + 0.2 * rng.randn(n)
    return x, yerr, r


@pytest.mark.parametrize("name,kernel", ZOO, ids=[z[0] for z in ZOO])
def test_zoo_kernel_through_the_reduction(name, kernel):
    x, yerr, r = _zoo_problem(kernel)
    ref = R.reference(kernel, x, yerr, r)
    assert ref.kappa <= 1e6
    P = kernels_np.full_size(kernel)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    g, alpha, diagA = s.grad(r, np.ones(max(P, 1), dtype=np.uint32))
    assert len(g) == P
    ratios = (ref.ratio_grad(g), ref.ratio_alpha(alpha), ref.ratio_diagA(diagA))
    assert max(ratios) <= 1.0, ratios
    _note(P, *ratios)


def test_stack_depth_8_through_the_reduction():
    kernel = R.deep_kernel(K, 8)
    rng = np.random.RandomState(8)
    for n in (65, 129):
        x = rng.uniform(0.0, 2.0, (n, 16))
        yerr, r = 0.1 + 0.05 * rng.rand(n), rng.randn(n)
        ref = R.reference(kernel, x, yerr, r)
        assert ref.kappa <= 1e6
        which = np.ones(len(ref.g), dtype=np.uint32)
        s = BasicSolver(kernel)
        s.compute(x, yerr)
        for g, alpha, diagA in (s.grad(r, which), BasicSolver(kernel).objective(x, yerr, r, which)[2:]):
            ratios = (ref.ratio_grad(g), ref.ratio_alpha(alpha), ref.ratio_diagA(diagA))
            assert max(ratios) <= 1.0, ratios
            _note(len(ref.g), *ratios)


def test_depth_9_and_65_parameters_are_refused_before_device_work():
    x = np.random.RandomState(0).uniform(0.0, 1.0, (10, 16))
    for kernel, msg in ((R.deep_kernel(K, 9), "too deep"),
                        (R.kernel_p64(K) + K.ConstantKernel(log_constant=0.0, ndim=16, axes=1), "too many kernel parameters")):
        s = BasicSolver(kernel)
        with pytest.raises(ValueError, match=msg):
            s.compute(x, 0.1)
        assert not s.computed
        with pytest.raises(ValueError, match=msg):
            s.objective(x, 0.1, np.ones(10))
        with pytest.raises(ValueError, match=msg):
            GP(kernel).compute(x, 0.1)


# ------------------------------------------------------------------ d. the GP layer
class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b

    def compute_gradient(self, t):
        return np.vstack([t, np.ones_like(t)])


def _gp_kernel():
    # 1-D, six parameters (kgrad_reduce_kernel<16>), a product of sums
    return ((K.ConstantKernel(log_constant=np.log(0.5)) + K.ExpSquaredKernel(0.8))
            * K.RationalQuadraticKernel(log_alpha=np.log(1.5), metric=0.9)
            + K.ConstantKernel(log_constant=np.log(0.3)) * K.CosineKernel(log_period=0.5))


@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("mean", ["constant", "model"])
def test_gp_gradient_against_reference(n, mean):
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0.0, 4.0, n))
    y = np.sin(3.0 * x) + 0.3 * rng.randn(n)
    yerr = (0.1 + 0.05 * rng.rand(n)) * max(1.0, np.sqrt(n / 300.0))
    kernel = _gp_kernel()
    kernel.freeze_parameter(kernel.get_parameter_names(include_frozen=True)[2])
    wn = np.log(0.02)
    if mean == "constant":
        make_mean = lambda: 0.3                       # noqa: E731
        mu, mg = np.full(n, 0.3), np.ones((1, n))
    else:
        make_mean = lambda: LinearMean(m=0.2, b=-1.0)  # noqa: E731
        mu, mg = 0.2 * x - 1.0, np.vstack([x, np.ones(n)])
    # restated from the reference's gp.py:443-466 on the reference's alpha and diag(A)
    sigma = np.sqrt(yerr ** 2 + np.exp(wn))
    ref = R.reference(kernel, x, sigma, y - mu)
    assert ref.kappa <= 1e6
    m = kernel.unfrozen_mask
    assert m.sum() == 5
    expect = np.concatenate([mg @ ref.alpha, [0.5 * np.sum(np.exp(wn) * ref.diagA)], ref.g[m]])
    tol = np.concatenate([np.abs(mg).sum(axis=1) * ref.tol_alpha(), [0.5 * n * np.exp(wn) * ref.tol_diagA()],
                          ref.tol_grad()[m]])
    for api in ("grad_log_likelihood", "nll_and_grad"):
        gp = GP(kernel, mean=make_mean(), fit_mean=True, white_noise=wn, fit_white_noise=True)
        gp.compute(x, yerr)
        assert len(gp) == len(expect) == len(mg) + 1 + 5
        if api == "grad_log_likelihood":
            g = gp.grad_log_likelihood(y)             # gh_chol_grad
            ll = gp.log_likelihood(y)
        else:
            gp.kernel.dirty = True                    # refactorise through gh_chol_objective
            nll, g = gp.nll_and_grad(gp.get_parameter_vector(), y)
            g, ll = -g, -nll
        assert ref._ratio(g - expect, tol) <= 1.0, api
        assert abs(ll + 0.5 * (ref.quad + ref.logdet + n * np.log(2 * np.pi))) <= 0.5 * (ref.tol_quad() + ref.tol_logdet())


# ------------------------------------------------------------------ e. tensor API at the new limits
def _close(a, b):
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b))


@pytest.mark.parametrize("P", [37, 64])
def test_tensor_gradient_at_16_dimensions(P):
    kernel = R.PCASES[P][0](K)
    rng = np.random.RandomState(P)
    x1, x2, xs = rng.uniform(0, 2, (65, 16)), rng.uniform(0, 2, (33, 16)), rng.uniform(0, 2, (70, 16))
    ki = KernelInterface(kernel)
    which = np.ones(P, dtype=np.uint32)
    _close(ki.gradient_general(which, x1, x2), kernels_np.gradient_general(kernel, x1, x2))
    _close(ki.gradient_symmetric(which, xs), kernels_np.gradient_symmetric(kernel, xs))
    masked = ki.gradient_general(_masks(P)["alternating"].astype(np.uint32), x1, x2)
    assert np.all(masked[:, :, 1::2] == 0.0)
    _close(masked[:, :, 0::2], kernels_np.gradient_general(kernel, x1, x2)[:, :, 0::2])


def test_coordinate_gradients_of_the_depth_8_expression():
    kernel = R.deep_kernel(K, 8)
    rng = np.random.RandomState(88)
    x1, x2 = rng.uniform(0, 2, (65, 16)), rng.uniform(0, 2, (33, 16))
    ki = KernelInterface(kernel)
    _close(ki.x1_gradient_general(x1, x2), kernels_np.x1_gradient_general(kernel, x1, x2))
    _close(ki.x2_gradient_general(x1, x2), kernels_np.x2_gradient_general(kernel, x1, x2))
    _close(ki.value_general(x1, x2), kernels_np.value_general(kernel, x1, x2))
    P = kernels_np.full_size(kernel)
    _close(ki.gradient_general(np.ones(P, dtype=np.uint32), x1, x2), kernels_np.gradient_general(kernel, x1, x2))
