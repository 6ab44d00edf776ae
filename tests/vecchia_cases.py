"""What tests/test_gpu_vecchia_grad.py and tests/test_vecchia_grad_host.py share: the problems (the kernels of
``grad_ref.PCASES`` and the depth-8 expression, P = 1 .. 64 parameters in 1 .. 16 dimensions), the restatement of the gradient
kernel's LDS size, the tolerance rule and the comparison helpers.  Nothing here touches a device.

The tolerance rule is the one derived in the docstring of tests/test_gpu_vecchia.py, nothing new: per compared quantity
``1000 x`` the gap between ``vecchia_ref.reference`` with every predecessor in the conditioning set and ``vecchia_ref.dense`` on
the test's own inputs, a gap counting as at least ``4 eps``, no bound looser than the dense-parity bounds ``CAPS``, gradients over
the restatement's ``S``.  The full restatement costs O(N^4), so the gap is taken on the first ``GAP_N`` points; and no gap may
exceed ``GAP_CAP`` (``gaps`` asserts it), so that a badly conditioned problem fails loudly instead of widening its own bound.
A slot whose scale is zero (a metric derivative at distance 0: at N = 1 that is 61 of the 64 slots of the P = 64 kernel) must
be exactly zero, in the gap as in every comparison.  Test helper only: not a conftest.
"""
import functools

import numpy as np

from george_amd import kernels
from george_amd.solvers.vecchia import vecchia_neighbors

import grad_ref
import vecchia_ref
from inducing_cases import CAPS, EPS, GAP_CAP, PCASE_NAMES

GAP_N = 150
VM_MAX = 64              # gh_vecchia_impl.h; tests/test_vecchia_grad_host.py reads the three out of the sources
GH_EVAL_WS = 16          # gh_eval.h: 2 * GH_MAX_AXES
V_GRAD_LDS = 96 * 1024   # gh_vecchia.hip: the raised limit of vecchia_grad_kernel's dynamic LDS

LOG = []                 # (what, error / bound) of every ``_check`` so far: a module reads its own slice for its report


# ------------------------------------------------------------------ the problems
def pcase(name, n=300):
    """(kernel, x, yerr, r, xs): the inputs of ``grad_ref.problem`` ordered by their first column (stable), 7 test points over
    the inputs' range; "deep8" takes the inputs of P = 37, the first 16-D case"""
    return _pcase(name, n)


@functools.lru_cache(maxsize=None)
def _pcase(name, n):
    kernel, x, yerr, r = grad_ref.problem(37 if name == "deep8" else name, n)
    if name == "deep8":
        kernel = grad_ref.deep_kernel(kernels, 8)
    order = np.argsort(x[:, 0], kind="stable")
    x, yerr, r = np.ascontiguousarray(x[order]), np.ascontiguousarray(yerr[order]), np.ascontiguousarray(r[order])
    lo = -1.0 if x.shape[1] == 1 else 0.0
    xs = np.random.RandomState(7).uniform(lo, lo + 2.0, (7, x.shape[1]))
    return kernel, x, yerr, r, xs


def _tri(j):
    return j * (j + 1) // 2


def grad_lds_bytes(m, ndim, P):
    """the dynamic LDS of vecchia_grad_kernel: ``v_lds_doubles(m, ndim, (P + GH_EVAL_WS) | 1) * 8`` of gh_vecchia.hip -- the
    block's coordinates and error bars, its packed triangle, dinv, u and ze, the 64 weights, 64 lanes of gradient row plus
    evaluator work space, and the block's indices"""
    gp = (P + GH_EVAL_WS) | 1
    return 8 * ((m + 1) * ndim + (m + 1) + _tri(m + 1) + VM_MAX + 2 * (m + 1) + VM_MAX + VM_MAX * gp + (m + 3) // 2)


# ------------------------------------------------------------------ the tolerance rule
def _over(diff, scale):
    """max |diff| / scale over the entries with a scale; an entry without one must be exactly zero"""
    diff, scale = np.abs(np.asarray(diff, dtype=np.float64)), np.asarray(scale, dtype=np.float64)
    diff, scale = np.broadcast_arrays(diff, scale)
    zero = scale == 0.0
    assert np.all(diff[zero] == 0.0), "a value whose scale is zero must be exactly zero"
    return float(np.max(diff[~zero] / scale[~zero])) if np.any(~zero) else 0.0


def gaps(name, n=300):
    """the gap of the two CPU routes per quantity, on the first ``GAP_N`` points of ``pcase(name, n)``"""
    return dict(_gaps(name, n))


@functools.lru_cache(maxsize=None)
def _gaps(name, n):
    kernel, x, yerr, r, xs = pcase(name, n)
    k = min(n, GAP_N)
    with np.errstate(invalid="ignore", divide="ignore"):    # (vecchia_ref.gaps divides by S; its kgrad entry is replaced below)
        g, ref, d = vecchia_ref.gaps(kernel, x[:k], yerr[:k], r[:k], xs)
    assert np.array_equal(ref.S == 0.0, d["S"] == 0.0)
    g["kgrad"] = _over(ref.kgrad - d["kgrad"], d["S"])
    g["ll"] = g["quad"]
    print("gaps", name, n, {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return g


def tolerances(name, n=300):
    return {key: min(1000.0 * max(v, 4 * EPS), CAPS.get(key, np.inf)) for key, v in gaps(name, n).items()}


@functools.lru_cache(maxsize=None)
def reference(name, n, m):
    """(the restatement with its gradient, the table) of ``pcase(name, n)`` with the default table of ``m`` neighbours"""
    kernel, x, yerr, r, xs = pcase(name, n)
    nbr = vecchia_neighbors(x, m)
    return vecchia_ref.reference(kernel, x, yerr, nbr, r=r, want_grad=True), nbr


def clear():
    for f in (_pcase, _gaps, reference):
        f.cache_clear()


# ------------------------------------------------------------------ comparisons
def _check(what, got, want, tol, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    err = _over(got - want, np.max(np.abs(want)) if scale is None else scale)
    print("%-26s error %.3g  bound %.3g" % (what, err, tol))
    LOG.append((what, err / tol))
    assert err <= tol, (what, err, tol)


def check_solves(s, r, ref, tol):
    """log_determinant, dot_solve, apply_inverse with 1 and 5 columns, in place and not"""
    n = len(r)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    ll = -0.5 * (s.dot_solve(r) + s.log_determinant + n * np.log(2 * np.pi))
    _check("log_likelihood", ll, ref.log_likelihood(), tol["ll"])
    Y = np.column_stack([r] + list(np.random.RandomState(5).randn(4, n)))
    for B in (r, Y):
        out = s.apply_inverse(B)
        _check("apply_inverse nrhs=%d" % (1 if B.ndim == 1 else B.shape[1]), out, ref.apply_q(B), tol["alpha"])
        Bc = B.copy()
        assert s.apply_inverse(Bc, in_place=True) is Bc and np.array_equal(Bc, out)


def check_grad(s, r, ref, tol):
    g, alpha, diagA = s.grad(r, np.ones(len(ref.kgrad), dtype=np.uint32))
    _check("grad: kernel", g, ref.kgrad, tol["kgrad"], scale=ref.S)
    _check("grad: alpha", alpha, ref.alpha, tol["alpha"])
    _check("grad: diagA", diagA, ref.diagA, tol["diagA"])
    return g, alpha, diagA


def check_predict(s, kernel, r, xs, ref, tol, cov=True):
    mu0, var0, cov0 = ref.predict(kernel, xs)
    mu, var, none = s.predict(kernel, r, xs, return_var=True)
    assert none is None
    _check("predict: mean", mu, mu0, tol["mu"])
    _check("  .. variance", var, var0, tol["var"])
    if cov:
        mu2, none, c = s.predict(kernel, r, xs, return_cov=True)
        _check("  .. covariance", c, cov0, tol["cov"])
        assert none is None and np.array_equal(mu2, mu)
