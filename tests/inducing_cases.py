"""What the tests of ``InducingSolver`` share: the problems, the tolerance rule and the comparison helpers of
tests/test_gpu_inducing.py, tests/test_gpu_inducing_grad.py and tests/test_inducing_host.py.  Nothing here touches a device.

The tolerance rule (derived in the docstring of tests/test_gpu_inducing.py): per compared quantity ``1000 x`` the gap between
``inducing_ref.reference`` and ``inducing_ref.dense_model`` on the test's own inputs, a gap counting as at least ``4 eps``, no
bound looser than the dense-parity bounds ``CAPS``, gradients over ``S``; beyond ``GAP_MAX_N`` points the gap is taken on the
first ``GAP_MAX_N`` with the same inducing points; and no gap may exceed ``GAP_CAP`` (``bounds`` asserts it).
Test helper only: not a conftest.
"""
import functools

import numpy as np

from george_amd import kernels
from george_amd.solvers.inducing import inducing_points

import grad_ref
import inducing_ref
from oracle import solver_np

EPS = np.finfo(np.float64).eps
CAPS = {"logdet": 1e-10, "quad": 1e-9, "ll": 1e-9}
GAP_CAP = 1e-9
GAP_MAX_N = 800
JITTER = {"expsq_1d": 1e-8}

LOG = []                 # (what, error / bound) of every ``_check`` so far: a module reads its own slice for its report


# ------------------------------------------------------------------ the named problems
def _kernel(name):
    """(kernel, ndim, amplitude); comp_3d takes the interpreter, has six parameters and one of them frozen"""
    if name == "m32_3d":
        return 1.3 * kernels.Matern32Kernel(0.6, ndim=3), 3, np.sqrt(1.3)
    if name == "m32_1d":
        return 1.7 * kernels.Matern32Kernel(0.8), 1, np.sqrt(1.7)
    if name == "expsq_1d":
        return 0.9 * kernels.ExpSquaredKernel(0.5), 1, np.sqrt(0.9)
    k = 0.8 * kernels.Matern32Kernel([0.5, 0.7, 0.9], ndim=3) + 0.3 * kernels.ExpSquaredKernel(0.6, ndim=3)
    k.freeze_parameter(k.get_parameter_names()[2])
    return k, 3, 1.0


@functools.lru_cache(maxsize=None)
def _problem(name, n):
    """(kernel, x, yerr, r, xs): error bars 0.1 .. 0.15 of the amplitude, 300 test points"""
    kernel, ndim, amp = _kernel(name)
    rng = np.random.RandomState(1000 * ndim + n)
    x = np.sort(rng.uniform(0, 10, n))[:, None] if ndim == 1 else rng.uniform(0, 2, (n, ndim))
    yerr = amp * (0.1 + 0.05 * rng.rand(n))
    r = amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))
    xs = rng.uniform(0, 10 if ndim == 1 else 2, (300, ndim))
    return kernel, x, yerr, r, xs


# ------------------------------------------------------------------ the tolerance rule
def tolerances(g):
    return {key: min(1000.0 * max(v, 4 * EPS), CAPS.get(key, np.inf)) for key, v in g.items()}


def bounds(label, kernel, x, yerr, r, xs, u, rel_jitter, method):
    """(absolute jitter, the restatement with its gradient, tolerances) of one problem; ``xs``: the test points of the gap of
    the predictions.  Up to ``GAP_MAX_N`` points the restatement is the one the gap was taken with; beyond, the block-wise
    route on all points."""
    jitter = rel_jitter * float(np.mean(solver_np.kernel_matrix(kernel, u, diag=True)))
    k = min(len(x), GAP_MAX_N)
    g, ref, _ = inducing_ref.gaps(kernel, x[:k], yerr[:k], u, jitter, method, r[:k], xs)
    if k < len(x):
        ref = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, route="blocks")
    g["ll"] = g["quad"]
    print("gaps", label, len(x), len(u), method, {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return jitter, ref, tolerances(g)


# ------------------------------------------------------------------ parameter count x dimension
# The kernels of grad_ref.PCASES (P = 1 .. 64 in 1 .. 16 dimensions) and the depth-8 expression (P = 20, 16-D) on the inputs of
# grad_ref.problem(P, n); the depth-8 expression takes the inputs of P = 37, the first 16-D case.
PCASE_NAMES = tuple(sorted(grad_ref.PCASES)) + ("deep8",)


@functools.lru_cache(maxsize=None)
def pcase(name, n=300, m=65):
    """(kernel, x, yerr, r, xs, u): ``m`` max-min inducing points among the data, 7 test points over the inputs' range"""
    kernel, x, yerr, r = grad_ref.problem(37 if name == "deep8" else name, n)
    if name == "deep8":
        kernel = grad_ref.deep_kernel(kernels, 8)
    lo = -1.0 if x.shape[1] == 1 else 0.0
    xs = np.random.RandomState(7).uniform(lo, lo + 2.0, (7, x.shape[1]))
    u = np.ascontiguousarray(x[inducing_points(x, m)])
    return kernel, x, yerr, r, xs, u


@functools.lru_cache(maxsize=None)
def pcase_bounds(name, method):
    """``bounds`` of ``pcase(name)`` under the default relative jitter: (relative jitter, absolute jitter, restatement, tolerances)"""
    kernel, x, yerr, r, xs, u = pcase(name)
    return (1e-10,) + bounds("P=%s" % name, kernel, x, yerr, r, xs, u, 1e-10, method)


@functools.lru_cache(maxsize=None)
def m32_case(n, m, inducing="maxmin"):
    """``_problem("m32_3d", n)`` with ``m`` inducing inputs: max-min points of the data, or ("random") uniform points that are no
    data points"""
    kernel, x, yerr, r, xs = _problem("m32_3d", n)
    if inducing == "maxmin":
        u = np.ascontiguousarray(x[inducing_points(x, m)])
    else:
        u = np.random.RandomState(m).uniform(0, 2, (m, 3))
    return kernel, x, yerr, r, xs, u


@functools.lru_cache(maxsize=None)
def m32_bounds(n, m, method, inducing="maxmin"):
    kernel, x, yerr, r, xs, u = m32_case(n, m, inducing)
    return (1e-10,) + bounds("m32_3d", kernel, x, yerr, r, xs[:7], u, 1e-10, method)


def grad_lds_bytes(P, ndim):
    """the dynamic LDS of ind_grad_tile_kernel (gh_inducing.hip): two 64-point tiles of inputs and (2 P + 16) | 1 doubles a lane"""
    return 8 * (2 * 64 * ndim + 64 * ((2 * P + 16) | 1))


@functools.lru_cache(maxsize=None)
def dot_problem(n=300, m=2):
    """a kernel without parameters: (kernel, x, yerr, r, xs, u)"""
    kernel = kernels.DotProductKernel(ndim=2)
    rng = np.random.RandomState(n)
    x = rng.uniform(-1.0, 1.0, (n, 2))
    yerr = 0.1 + 0.05 * rng.rand(n)
    r = np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n)
    xs = rng.uniform(-1.0, 1.0, (7, 2))
    u = np.ascontiguousarray(x[inducing_points(x, m)])
    return kernel, x, yerr, r, xs, u


# ------------------------------------------------------------------ comparisons
def _check(what, got, want, tol, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.max(np.abs(want)) if scale is None else scale
    err = np.max(np.abs(got - want) / np.maximum(scale, np.finfo(float).tiny))
    print("%-26s error %.3g  bound %.3g" % (what, err, tol))
    LOG.append((what, err / tol))
    assert err <= tol, (what, err, tol)


def _check_grad(s, kernel, r, ref, tol):
    mask = kernel.unfrozen_mask
    g, alpha, diagA = s.grad(r, mask.astype(np.uint32))
    assert len(g) == len(mask) and np.all(g[~mask] == 0.0)
    _check("grad: kernel", g[mask], ref.kgrad[mask], tol["kgrad"], scale=ref.S[mask])
    _check("grad: alpha", alpha, ref.alpha, tol["alpha"])
    _check("grad: diagA", diagA, ref.diagA, tol["diagA"])
    return g, alpha, diagA


def _check_predict(s, kernel, r, xs, ref, tol, m_list):
    out = None
    for mm in m_list:
        mu0, var0, cov0 = ref.predict(kernel, xs[:mm])
        mu, var, cov = s.predict(kernel, r, xs[:mm], return_var=True)
        assert cov is None
        _check("predict M=%d: mean" % mm, mu, mu0, tol["mu"])
        _check("  .. variance", var, var0, tol["var"])
        assert np.array_equal(s.predict(kernel, r, xs[:mm])[0], mu)
        out = (mu, var)
    return out
