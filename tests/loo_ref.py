"""CPU reference for leave-one-out cross-validation of a GP, and the test problems that pin it.

With ``K = k(x, x) + diag(yerr^2)``, ``alpha = K^-1 r`` and ``c_i = (K^-1)_ii`` (GPML section 5.4.2):

    resid_i = alpha_i / c_i = y_i - mu_i,    var_i = 1 / c_i,
    lpd_i   = 1/2 log c_i - 1/2 alpha_i^2 / c_i - 1/2 log 2 pi,      L = sum_i lpd_i,

and with ``u = resid``, ``w_i = 1/2 (1 + alpha_i^2 / c_i) / c_i``, ``v = K^-1 u``,
``B = 1/2 (v alpha^T + alpha v^T) - K^-1 diag(w) K^-1``:

    dL/dtheta_p = sum_ij B_ij dK_ij/dtheta_p   (full sum: lower triangle with weights 2, diagonal 1),
    dL/dK_ii    = B_ii   (``diagB``),          dL/dmean_i = v_i.

``reference()`` evaluates these independently of every HIP path: ``K`` from ``oracle.solver_np.kernel_matrix``, ``dK``
from ``oracle.kernels_np``, factor / solves / inverse from SciPy ``cho_factor`` / ``cho_solve``; the contraction runs
over the lower triangle in blocks of ``BLOCK`` rows, summed in ``np.longdouble``.  ``brute_force()`` does the N explicit
refits with one point removed.

Tolerance: the project's one rule (tests/grad_ref.py), ``|x - x_ref| <= C_TOL * U * kappa(K) * S`` with the operand
scales

    resid: max|alpha| max(1/c)        var: max(1/c)        lpd: max(1/2 |log c| + 1/2 alpha^2/c);  L: their sum
    v: max|v|                         diagB: max(|v_i alpha_i| + (|K^-1| diag(w) |K^-1|)_ii)
    gradient: S_p = sum_ij (|v_i alpha_j| + (|K^-1| diag(w) |K^-1|)_ij) D_ij,p     (D as in grad_ref.py).

``v`` and ``K^-1 diag(w) K^-1`` pass through ``K^-1`` twice, so their worst-case error grows as ``kappa^2``; on the test
problems here (error bars >= 0.1 of the kernel amplitude) every quantity, those included, is held to the first power of
``kappa``: no quantity uses ``kappa^2``.

``defect=`` runs a deliberately wrong version (tests/test_loo_reference.py checks that the rule rejects each).
Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from grad_ref import U, C_TOL, BLOCK, Ref, leaf_blocks, _as_2d
from oracle import kernels_np, solver_np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
PAD = 128                # the device layout pads N to a multiple of this with identity rows

DEFECTS = ("diag_weight_half", "outer_half_kept", "w_without_alpha_term", "v_is_u", "drop_last_row", "padded_rows_in_L")


class LooRef(object):
    """What ``reference()`` returns: ``L``, ``lpd``, ``resid``, ``var``, ``v``, ``diagB`` (N,), ``g``, ``S`` (P,), ``alpha``,
    ``c``, ``Kinv``, ``kappa`` and the scales ``S_resid``, ``S_var``, ``S_lpd``, ``S_L``, ``S_v``, ``S_diagB`` (the largest entry
    of ``mag_diagB``, the per-point magnitude)."""

    def tol(self, what):
        return C_TOL * U * self.kappa * getattr(self, "S" if what == "g" else "S_" + what)

    def ratio(self, what, value):
        """largest |error| / tolerance of quantity ``what`` (<= 1 passes)"""
        return Ref._ratio(np.asarray(value, dtype=np.float64) - getattr(self, what), self.tol(what))


def _refined_solve(cf, K, b):
    """cho_solve with one step of refinement on a residual formed in extended precision"""
    z = cho_solve(cf, b)
    res = b.astype(np.longdouble) - np.dot(K.astype(np.longdouble), z.astype(np.longdouble))
    return z + cho_solve(cf, res.astype(np.float64))


def reference(kernel, x, yerr, r, defect=None, block=BLOCK):
    """The leave-one-out reference (module docstring) for ``kernel`` at inputs ``x`` with per-point standard deviations
    ``yerr`` (white noise included) and residual ``r = y - mean``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    P = kernels_np.full_size(kernel)

    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    cf = cho_factor(K, lower=True)
    alpha = _refined_solve(cf, K, r)
    Kinv = cho_solve(cf, np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    c = np.array(np.diag(Kinv))
    resid = alpha / c
    var = 1.0 / c
    q = alpha * resid
    lpd = 0.5 * np.log(c) - 0.5 * q - HALF_LOG_2PI
    L = float(np.sum(lpd.astype(np.longdouble)))
    if defect == "padded_rows_in_L":
        L += (-(-n // PAD) * PAD - n) * (-HALF_LOG_2PI)      # identity padding: c = 1, alpha = 0
    w = 0.5 * (1.0 + (0.0 if defect == "w_without_alpha_term" else q)) / c
    v = resid.copy() if defect == "v_is_u" else _refined_solve(cf, K, resid)
    absK = np.abs(Kinv)
    M = np.dot(Kinv * w[None, :], Kinv)
    absM = np.dot(absK * w[None, :], absK)
    diagB = v * alpha - np.diag(M)

    g = np.zeros(P, dtype=np.longdouble)
    S = np.zeros(P, dtype=np.longdouble)
    blocks = [(a, b) for a, b in leaf_blocks(kernel) if b > 0]
    for s in range(0, n, block):
        e = min(n, s + block)
        G = kernels_np.gradient_general(kernel, x[s:e], x[:e])        # rows s..e-1 against columns 0..e-1
        W = 0.5 * (np.outer(v[s:e], alpha[:e]) + np.outer(alpha[s:e], v[:e])) - M[s:e, :e]
        Mag = 0.5 * (np.abs(np.outer(v[s:e], alpha[:e])) + np.abs(np.outer(alpha[s:e], v[:e]))) + absM[s:e, :e]
        rows = np.arange(s, e)[:, None]
        cols = np.arange(e)[None, :]
        wt = np.where(cols < rows, 2.0, np.where(cols == rows, 0.5 if defect == "diag_weight_half" else 1.0, 0.0))
        W = W * wt
        Mag = Mag * np.where(cols < rows, 2.0, np.where(cols == rows, 1.0, 0.0))
        if defect == "drop_last_row":
            W = np.where(rows == n - 1, 0.0, W)
        if P:
            g += np.sum(W[:, :, None] * G, axis=(0, 1), dtype=np.longdouble)
            D = np.abs(G)
            for a, b in blocks:
                D[:, :, a:a + b] = np.max(D[:, :, a:a + b], axis=2, keepdims=True)
            S += np.sum(Mag[:, :, None] * D, axis=(0, 1), dtype=np.longdouble)
    g = g.astype(np.float64)
    if defect == "outer_half_kept":
        g = 0.5 * g

    out = LooRef()
    out.L, out.lpd, out.resid, out.var, out.v, out.diagB, out.g = L, lpd, resid, var, v, diagB, g
    out.S = S.astype(np.float64)
    out.alpha, out.c, out.Kinv = alpha, c, Kinv
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(Kinv, 1))
    out.S_resid = float(np.max(np.abs(alpha)) * np.max(var))
    out.S_var = float(np.max(var))
    each = 0.5 * np.abs(np.log(c)) + 0.5 * q
    out.S_lpd = float(np.max(each))
    out.S_L = float(np.sum(each))
    out.S_v = float(np.max(np.abs(v)))
    out.mag_diagB = np.abs(v * alpha) + np.diag(absM)
    out.S_diagB = float(np.max(out.mag_diagB))
    return out


def brute_force(kernel, x, yerr, r):
    """``(L, lpd, resid, var)`` from N explicit refits, each with one point removed: the prediction of ``r_i`` from the
    other points (``K_-i`` factorised afresh) and its variance, noise of point i included."""
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    resid, var = np.empty(n), np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        if n == 1:
            mu, vi = 0.0, K[0, 0]
        else:
            cf = cho_factor(K[np.ix_(keep, keep)], lower=True)
            ks = K[i, keep]
            mu = float(np.dot(ks, cho_solve(cf, r[keep])))
            vi = float(K[i, i] - np.dot(ks, cho_solve(cf, ks)))
        resid[i], var[i] = r[i] - mu, vi
    lpd = -0.5 * np.log(var) - 0.5 * resid ** 2 / var - HALF_LOG_2PI
    return float(np.sum(lpd.astype(np.longdouble))), lpd, resid, var


# ------------------------------------------------------------------------------------ test problems
def _kernels():
    from george_amd import kernels
    return kernels


def kernel_expsq():
    K = _kernels()
    return 1.3 * K.ExpSquaredKernel(0.6)


def kernel_matern3d():
    K = _kernels()
    metric = np.array([[1.2, 0.3, -0.2], [0.3, 0.8, 0.1], [-0.2, 0.1, 1.5]])
    return 0.9 * K.Matern32Kernel(metric, ndim=3)


def kernel_hyper():
    """the 17-node composite of docs/tutorials/hyper.rst"""
    K = _kernels()
    k1 = 66.0 ** 2 * K.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * K.ExpSquaredKernel(90.0 ** 2) * K.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * K.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * K.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def kernel_2d():
    """P = 5: a product of sums in two dimensions (grad_ref.kernel_p5)"""
    import grad_ref
    return grad_ref.kernel_p5(_kernels())


def kernel_p13():
    import grad_ref
    K = _kernels()
    return (grad_ref.kernel_p5(K)
            + K.ConstantKernel(log_constant=np.log(0.5), ndim=2) * K.Matern32Kernel([0.7, 1.9], ndim=2)
            + K.ConstantKernel(log_constant=np.log(0.2), ndim=2) * K.ExpSquaredKernel(np.array([[1.1, 0.2], [0.2, 0.6]]), ndim=2)
            + K.ConstantKernel(log_constant=np.log(0.05), ndim=2))


def kernel_p17():
    import grad_ref
    return grad_ref.kernel_p17(_kernels())


# name -> (builder, input dimension, kernel amplitude: the error bars are 0.1 .. 0.15 of it)
KERNELS = {
    "expsq": (kernel_expsq, 1, np.sqrt(1.3)),
    "matern3d": (kernel_matern3d, 3, np.sqrt(0.9)),
    "hyper": (kernel_hyper, 1, 66.0),
    "2d": (kernel_2d, 2, 1.0),
    "p13": (kernel_p13, 2, 1.2),
    "p17": (kernel_p17, 4, 1.2),
}


def problem(name, n, seed=0):
    """(kernel, x, yerr, r) of the test problem (name, n); the noise grows with n past 300 as in grad_ref.problem."""
    build, ndim, amp = KERNELS[name]
    kernel = build()
    rng = np.random.RandomState(7919 * (sorted(KERNELS).index(name) + 1) + n + seed)
    if ndim == 1:
        x = np.sort(rng.uniform(0.0, 10.0, n))[:, None]
    else:
        x = rng.uniform(0.0, 2.0, (n, ndim))
        x = x[np.argsort(x[:, 0])]
    yerr = amp * (0.1 + 0.05 * rng.rand(n)) * max(1.0, np.sqrt(n / 300.0))
    r = amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))
    return kernel, x, yerr, r
