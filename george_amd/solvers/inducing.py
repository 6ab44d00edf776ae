"""``InducingSolver`` -- the inducing-point approximations DTC and FITC and the variational bound (VFE) on one MI355X, for
smooth kernels on data sets no N x N factor fits: 10^5 - 10^6 points, a few hundred to a few thousand inducing inputs.

The covariance is replaced by a low-rank term through ``m`` inducing inputs ``u`` plus a diagonal,
``C = K_fu (K_uu + jitter I)^-1 K_uf + diag(lambda)``, with ``lambda_i = yerr_i^2`` (DTC) or ``yerr_i^2`` plus the variance the
low-rank term leaves at ``x_i`` (FITC).  O(N m^2) flops in GEMM shapes, O(m^2) memory beside the data: the data points pass
through the device in strips.  It is the complement of :class:`VecchiaSolver`: near-exact where the kernel is smooth (which is
where the nearest-neighbour likelihood stays percents off), mediocre for rough kernels (where Vecchia converges fast).  Rule of
thumb: smooth kernel, inducing points; rough kernel, Vecchia; and check one against the other.  With ``u = x`` and no jitter
both methods are the dense likelihood up to rounding.  No reference counterpart.  The definition is in ``include/george_amd.h``,
the device side in ``george_amd/csrc/gh_inducing.hip``.

Prediction is the same for both methods, O(M m^2) whatever N.

``variational=True`` (with ``method="dtc"``) turns the objective into Titsias' lower bound of the exact log-likelihood,
``F = log N(r | 0, C) - 1/2 tau`` with ``tau = sum_i max(k(x_i, x_i) - q_i, 0) / yerr_i^2``: ``F`` never exceeds the dense
log-likelihood and does not decrease when an inducing input is added, which DTC and FITC do not promise.  It is the objective
under which the inducing inputs may be optimised without over-fitting: :meth:`InducingSolver.grad_inducing` gives the gradient
with respect to them (for all three objectives), ``GP.nll_and_grad_inducing`` the joint objective for an optimiser.  The
gradient costs one more pass of N m kernel input-gradient evaluations and one more pass of strip GEMMs beside ``grad``'s work
(counts, not measurements; ``include/george_amd.h`` has them).

``jitter`` is relative: the device gets ``jitter * mean_j k(u_j, u_j)`` on the diagonal of ``K_uu``, and the likelihood gradient
treats that number as a constant.

The default inducing set is greedy max-min distance over the data (:func:`inducing_points`): O(N m) NumPy on the host by
default, or ``select="device"``: one streaming kernel per pick (``george_amd/csrc/gh_inducing_select.hip``) that returns the
same points for up to 7 input dimensions.

Leave-one-out cross-validation (``loo_lowrank``, behind ``GP.loo_predict``, ``loo_log_likelihood``, ``grad_loo_log_likelihood``
and ``loo_nll_and_grad``) is that of the DTC / FITC density, exact for it, at any N: ``diag C^-1`` is one row norm per data point
of a strip the gradient already builds, and the gradient is ``grad``'s reduction with other weights; nothing N x N or N x m is
kept.  ``(y - mu) / sqrt(var)`` are the standardised residuals of the model that was fitted: the direct check of ``m``.  (Before
``loo_lowrank`` ``GP`` went through ``get_inverse()``, an N x N array, and the kernel gradient it returned for this solver was
not the derivative of its value unless ``u = x``.)

Not built: ``apply_sqrt``, a multi-device form, a Fisher information or leave-group-out form, and the gradient of the
leave-one-out score with respect to the inducing inputs.
"""
import ctypes as C
import hashlib

import numpy as np

from .. import _native as N
from .protocol import HandlePool, NativeSolver, rhs_vector

__all__ = ["InducingSolver", "inducing_points"]

M_MAX = 8192
METHODS = {"dtc": 0, "fitc": 1}


def inducing_points(x, m, device=None, return_dmin=False):
    """The indices of ``min(m, N)`` of the points ``x`` chosen by greedy max-min distance: the point nearest the centroid
    first, then each time the point whose smallest squared Euclidean distance to the chosen ones is largest, ties going to
    the lower index.  Returns an int64 array in the order chosen; with ``return_dmin`` also every point's squared distance
    to the chosen set (N doubles; its maximum is the squared fill distance).  ``m`` has no cap: ``m >= N`` orders all points.

    ``device``: ``None`` selects on the host, O(N m) NumPy on one thread; an integer runs ``gh_inducing_select`` on that
    device (one streaming kernel per pick; the first point still comes from the host, one pass over ``x``): the same
    sequence and the same ``dmin`` bit for bit for up to 7 input dimensions, and from 8 on the greedy sequence under the
    device's left-to-right sum of squares, where NumPy adds pairwise.  The device route raises ``ValueError`` for ``x`` that
    is not finite and ``RuntimeError`` without a device."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError("x must be (nsamples, ndim)")
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    n = len(x)
    k = min(m, n)
    idx = np.empty(k, dtype=np.int64)
    if n == 0:
        return (idx, np.empty(0)) if return_dmin else idx
    if device is not None and not np.isfinite(x).all():
        raise ValueError("inducing_points: the device selection needs finite x")
    d2 = ((x - x.mean(axis=0)) ** 2).sum(axis=1)
    if device is not None:
        x = np.ascontiguousarray(x)
        dmin = np.empty(n) if return_dmin else None
        N.check(N.lib.gh_inducing_select(int(device), N.ptr(x), n, x.shape[1], int(np.argmin(d2)), m, N.ptr(idx), N.ptr(dmin)))
        return (idx, dmin) if return_dmin else idx
    idx[0] = np.argmin(d2)                                  # (argmin / argmax return the first of equals: the lower index)
    dmin = ((x - x[idx[0]]) ** 2).sum(axis=1)
    for j in range(1, k):
        idx[j] = np.argmax(dmin)
        np.minimum(dmin, ((x - x[idx[j]]) ** 2).sum(axis=1), out=dmin)
    return (idx, dmin) if return_dmin else idx


class InducingSolver(NativeSolver):
    """``InducingSolver(kernel, inducing=512, method="fitc", jitter=1e-10, device=0, strip_points=0, select="host",
    variational=False)``.

    ``inducing``: an (m, ndim) array of inducing inputs, or an int ``m``: ``min(m, N)`` of the data points chosen by
    :func:`inducing_points` (kept per data set, so an optimiser pays for the selection once); 1 <= m <= 8192.  ``method``:
    ``"dtc"`` or ``"fitc"``.  ``jitter``: relative to the mean of ``k(u_j, u_j)``.  ``strip_points``: data points per
    strip on the device, 0 for a choice by memory budget (results do not depend on it beyond rounding).  ``select``: where
    an int ``inducing`` is turned into points, ``"host"`` (NumPy) or ``"device"`` (``gh_inducing_select`` on the solver's
    device: the same points for up to 7 input dimensions).  ``variational``: the variational bound; it needs ``method="dtc"``.

    Under the bound ``log_determinant`` is ``log|C| + tau`` (``trace_term`` is ``tau``, 0.0 when the bound is off): that is what
    ``GP``'s ``-1/2 (r^T C^-1 r + log_determinant + N log 2 pi)`` needs, so ``GP.log_likelihood``, ``nll_and_grad`` and the rest
    return the bound ``F`` and its gradient, with no branch in ``GP``.  It is NOT the log-determinant of a covariance then.

    A factorisation that fails raises ``numpy.linalg.LinAlgError`` like the other solvers, naming the factor;
    ``failed_factor`` is then ``"K_uu"`` or ``"A"`` and ``failed_pivot`` its 0-based pivot."""

    _CREATE, _DESTROY = "gh_inducing_create", "gh_inducing_destroy"
    _SOLVE, _DOT_SOLVE = "gh_inducing_solve", "gh_inducing_dot_solve"   # C^-1 y and y^T C^-1 y; no get_inverse, no apply_sqrt

    def __init__(self, kernel, inducing=512, method="fitc", jitter=1e-10, device=0, strip_points=0, select="host", variational=False):
        if method not in METHODS:
            raise ValueError("InducingSolver: method is 'dtc' or 'fitc'")
        variational = bool(variational)
        if variational and method != "dtc":
            raise ValueError("InducingSolver: variational=True needs method='dtc'")
        if select not in ("host", "device"):
            raise ValueError("InducingSolver: select is 'host' or 'device'")
        jitter = float(jitter)
        if not jitter >= 0.0:
            raise ValueError("InducingSolver: jitter must not be negative")
        strip_points = int(strip_points)
        if strip_points < 0:
            raise ValueError("InducingSolver: strip_points must not be negative")
        if np.ndim(inducing) == 0:
            inducing = int(inducing)
            if inducing < 1 or inducing > M_MAX:
                raise ValueError("InducingSolver: 1 <= m <= {0}, not {1}".format(M_MAX, inducing))
        else:
            inducing = N.as_f64(inducing)
            if inducing.ndim == 1:
                inducing = inducing[:, None]
            if inducing.ndim != 2 or not 1 <= len(inducing) <= M_MAX:
                raise ValueError("InducingSolver: inducing must be (m, ndim) with 1 <= m <= {0}".format(M_MAX))
        self.inducing = inducing
        self.method = method
        self.jitter = jitter
        self.select = select
        self.variational = variational
        self.trace_term = 0.0                               # tau of the last compute(); 0.0 when the bound is off
        self.failed_factor = None
        self.failed_pivot = None
        self.u = None                                       # the inducing inputs of the last compute()
        self._opts = dict(device=int(device), method=METHODS[method], strip_points=strip_points, variational=int(variational))
        super(InducingSolver, self).__init__(kernel)

    # The default inducing set depends on the inputs, m and the route only (from 8 dimensions on the two routes may differ), and
    # GP makes a new solver for every compute (one per iterate of an optimiser): the last selections are kept, keyed by a digest
    # of the inputs.
    _TABLES = []
    _TABLES_MAX = 2

    def _default_points(self, x):
        key = (x.shape, self.inducing, self.select, hashlib.blake2b(memoryview(x).cast("B"), digest_size=16).digest())
        for k, idx in InducingSolver._TABLES:
            if k == key:
                return idx
        idx = inducing_points(x, self.inducing, device=self._opts["device"] if self.select == "device" else None)
        InducingSolver._TABLES.append((key, idx))
        del InducingSolver._TABLES[:-InducingSolver._TABLES_MAX]
        return idx

    # -- lifetime.  The handle of a dropped solver (its m x m buffers on the device) is parked, at most _HPOOL_MAX per
    # (device, method, strip_points, variational), and picked up by the next solver with the same options.
    _HPOOL_MAX = 2
    _HPOOL = HandlePool(_DESTROY, _HPOOL_MAX)
    _GIVES_BACK_POOLS = (_HPOOL,)                           # out of memory: own handle, own pool and the native caches

    def _options_key(self):
        key = (self._opts["device"], self._opts["method"], self._opts["strip_points"])
        return key + (1,) if self._opts["variational"] else key

    def _native_opts(self):
        o = N.gh_inducing_opts()
        o.device, o.method, o.strip_points, o.variational = (self._opts[k] for k in ("device", "method", "strip_points", "variational"))
        return o

    def compute(self, x, yerr):
        x, yerr, _ = self._check_inputs(x, yerr)
        n = len(x)
        self.failed_factor = self.failed_pivot = None
        if isinstance(self.inducing, int):
            u = np.ascontiguousarray(x[self._default_points(x)])
        else:
            u = self.inducing
            if u.shape[1] != x.shape[1]:
                raise ValueError("InducingSolver: inducing must be (m, {0})".format(x.shape[1]))
        m = len(u)
        kd = np.empty(m)
        N.check(N.lib.gh_kernel_value_diagonal(self._dk.handle, N.ptr(u), N.ptr(u), m, N.ptr(kd)))
        jitter = self.jitter * float(np.mean(kd))
        logdet = C.c_double(0.0)
        self._n, self.u = n, u

        def run(h):
            rc = N.lib.gh_inducing_compute(h, self._dk.handle, N.ptr(x), n, x.shape[1], N.ptr(yerr), N.ptr(u), m, jitter, C.byref(logdet))
            if rc == N.GH_ERR_NOT_PD:
                info = int(N.lib.gh_inducing_info(h))
                self.failed_factor, self.failed_pivot = ("K_uu" if info > 0 else "A"), abs(info) - 1
                raise np.linalg.LinAlgError("InducingSolver: the factorisation of {0} failed at pivot {1} ({2}); raise jitter (now {3:g})"
                                            .format("K_uu + jitter I" if info > 0 else "A = I + V Lambda^-1 V^T", self.failed_pivot,
                                                    N.last_error(), self.jitter))
            N.check(rc)

        self._retry_without_parked_memory(run)
        tau = C.c_double(0.0)
        N.check(N.lib.gh_inducing_trace_term(self._handle, C.byref(tau)))
        self.trace_term = tau.value
        self._log_det = logdet.value + tau.value if self.variational else logdet.value
        self.computed = True

    # -- the solver protocol
    def _solve_target(self, y, yc, in_place):
        """``in_place``: the values are copied back into any writable array ``y``, whatever its dtype"""
        return np.empty_like(yc), (y if in_place and isinstance(y, np.ndarray) and y.flags.writeable else None)

    # -- device-resident GP glue
    def grad(self, r, which):
        """``BasicSolver.grad``'s ``(kgrad_full, alpha, diagA)`` for the DTC / FITC likelihood: the gradient over ALL kernel
        parameters (masked ones 0), ``alpha = C^-1 r`` and ``diagA_i = alpha_i^2 - (C^-1)_ii``.  With ``u = x`` and no jitter
        these are the dense values."""
        return self._grad("gh_inducing_grad", r, which)

    def grad_inducing(self, r, which=None):
        """``(kgrad_full | None, alpha, diagA, ugrad)``: :meth:`grad`'s three results (``None`` for the first without ``which``)
        and the gradient of the objective -- the DTC or FITC log-likelihood, or the bound -- with respect to the inducing
        inputs, (m, ndim).  The absolute jitter counts as a constant.  One more pass of N m input-gradient evaluations
        and a second pass of strip GEMMs beside ``grad``'s work; the first three results have ``grad``'s bits."""
        h = self._need()
        r = self._in(rhs_vector(r, self._n))
        g = None
        if which is not None:
            which = np.ascontiguousarray(which, dtype=np.uint32)
            g = np.zeros(max(self._dk.size, 1))
        alpha, diagA, ugrad = np.empty(self._n), np.empty(self._n), np.empty(self.u.shape)
        N.check(N.lib.gh_inducing_grad_u(h, self._dk.handle, N.ptr(which), N.ptr(r), N.ptr(g), N.ptr(alpha), N.ptr(diagA), N.ptr(ugrad)))
        return (None if g is None else g[:self._dk.size]), self._out(alpha), self._out(diagA), ugrad

    def loo_lowrank(self, r, which=None):
        """Leave-one-out cross-validation of the DTC / FITC density for residual ``r = y - mean`` (gh_inducing_loo), the contract of
        ``BasicSolver.loo`` and ``VecchiaSolver.loo_blocks``: ``(lpd_sum, resid, var, lpd, grad_full | None, v | None, diagB | None)``
        with ``resid = y - mu_loo``, ``var`` the leave-one-out variances, ``lpd`` the N log predictive densities and ``lpd_sum``
        their sum, all from ``c = diag C^-1`` (one row norm of a strip of ``H^T`` per point) and ``alpha = C^-1 r``.
        ``which=None``: values only, about one ``dot_solve`` and one strip pass.  With a parameter mask also ``grad_full`` =
        d lpd_sum / d theta over ALL kernel parameters (masked ones exactly 0), ``v`` = d lpd_sum / d mean_i and ``diagB`` =
        d lpd_sum / d C_ii, by two passes over the strips and ``grad``'s reduction; nothing N x m or N x N is kept.  It is the
        leave-one-out of THIS density, exact for it, and its gradient is the derivative of its value: the dense one with ``u = x``
        and no jitter, and as far from it as ``C`` is from ``K`` otherwise -- hence a name of its own: ``loo`` stays the dense
        call, which only ``BasicSolver`` offers, and ``GP`` takes this one where a solver has neither ``loo`` nor
        ``loo_blocks``.  With ``variational=True`` it is the leave-one-out of the DTC density (the solves and predictions there
        are DTC's; ``tau`` does not enter), with the bits of a ``method="dtc"`` solver."""
        self._need()
        n, size = self._n, self._dk.size
        r = self._in(rhs_vector(r, n))
        wh = g = v = diagB = None
        if which is not None:
            which = np.asarray(which)
            if which.shape != (size,):
                raise ValueError("which must have shape ({0},)".format(size))
            wh = np.zeros(max(size, 1), dtype=np.uint32)
            wh[:size] = which != 0
            g, v, diagB = np.zeros(max(size, 1)), np.empty(n), np.empty(n)
        total = C.c_double(0.0)
        resid, var, lpd = np.empty(n), np.empty(n), np.empty(n)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_inducing_loo(
            hh, self._dk.handle, N.ptr(wh), N.ptr(r), C.byref(total), N.ptr(resid), N.ptr(var), N.ptr(lpd),
            N.ptr(g), N.ptr(v), N.ptr(diagB))))
        if which is None:
            return total.value, self._out(resid), self._out(var), self._out(lpd), None, None, None
        return total.value, self._out(resid), self._out(var), self._out(lpd), g[:size], self._out(v), self._out(diagB)

    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """The predictive mean and (optionally) variance or covariance at ``xs``, the same for DTC and FITC, in strips of
        test points.  The covariance keeps three M x m blocks and the M x M result on the device and raises ``MemoryError``
        over its budget."""
        return self._predict("gh_inducing_predict", kernel, r, xs, return_var, return_cov)
