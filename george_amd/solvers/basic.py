"""``BasicSolver`` -- dense Cholesky on one MI355X.

Drop-in for the reference's ``BasicSolver`` (``src/george/solvers/basic.py``):
same constructor, methods, shapes and error behaviour, but ``compute`` builds
the covariance matrix on the device from ``(kernel, x)`` and factorises it there
(blocked fp64-MFMA Cholesky, george_amd/csrc/gh_chol.hip); the N x N matrix
never visits the host.  Extra, optional entry points (``predict``, ``grad``)
keep the GP glue of ``gp.py:482-545`` / ``:429-466`` device-resident;
:class:`george_amd.GP` uses them when present, the reference GP simply ignores
them.
"""
import ctypes as C

import numpy as np

from .. import _native as N
from ..program import DeviceKernel
from .protocol import HandlePool, NativeSolver, rhs_vector

__all__ = ["BasicSolver"]


def _fits_the_byte_budget(h):
    """The admission rule of BasicSolver's pool: a handle is parked as it is while the pool stays under _POOL_MAX_BYTES (read
    now: it may have been rebound), else trimmed to its factor-sized buffers, and refused when even that does not fit."""
    size = lambda hh: int(N.lib.gh_chol_device_bytes(hh))
    room = BasicSolver._POOL_MAX_BYTES - sum(size(p) for free in BasicSolver._POOL.values() for p in free)
    if size(h) <= room:
        return True                        # as it is: the next iterate re-uses the work arrays too
    N.lib.gh_chol_trim(h)                  # keep the factor-sized buffers, drop the work arrays
    return size(h) <= room


class BasicSolver(NativeSolver):

    _CREATE, _DESTROY = "gh_chol_create", "gh_chol_destroy"
    _SOLVE, _DOT_SOLVE, _GET_INVERSE, _APPLY_SQRT = "gh_chol_solve", "gh_chol_dot_solve", "gh_chol_get_inverse", "gh_chol_apply_sqrt"

    def __init__(self, kernel, device=0, nb=0, profile=False, lookahead=True):
        super(BasicSolver, self).__init__(kernel)
        self._opts = dict(device=int(device), nb=int(nb), profile=bool(profile), lookahead=bool(lookahead))
        self._factor_state = None

    # -- lifetime.  `GP.compute` instantiates a NEW solver on every call (gp.py:327) -- thousands of
    # times inside an optimiser loop -- so native handles (and the N x N device buffers they own)
    # are recycled through a small per-configuration pool instead of being hipMalloc'ed each time.
    # A handle keeps every buffer it ever grew (the factor, and after grad / get_inverse / predict up
    # to three more N x N work arrays: ~100 GB at N = 65536).  It is parked AS IT IS while the pool
    # stays under _POOL_MAX_BYTES of device memory in total (an optimiser iterate drops its solver
    # and the next one picks the same handle up: freeing the work arrays in between meant two or
    # three hipFree + hipMalloc of 8 N^2 bytes per iterate -- the fused objective ran 2x slower than
    # the separate calls in round 2's driver run); above that budget it is trimmed to its factor,
    # and above it still it is destroyed.  At most _POOL_MAX handles are parked per option set;
    # ``BasicSolver.release_pool()`` empties the pool, and it is emptied at interpreter exit.
    _POOL_MAX = 2
    _POOL_MAX_BYTES = 112 << 30
    _HPOOL = _POOL = HandlePool(_DESTROY, _POOL_MAX, admit=_fits_the_byte_budget)
    _HANDLES = ("_handle", "_bhandle")
    # out of memory: the pool (up to _POOL_MAX_BYTES, work arrays included) and the native block cache (up to 48 GB) go; the
    # solver's own handle stays, it may hold a factor that ``append`` and the rest still need
    _GIVES_BACK_OWN_HANDLE, _GIVES_BACK_POOLS = False, (_POOL,)
    # ``pickle`` of a computed solver carries the factor (reference behaviour, tests/test_pickle.py:21-36)
    # up to this many points (8 GB of packed lower triangle at 46340); beyond it the state drops the
    # factor and the solver comes back un-computed, like the reference's own native solver does
    # (solvers/hodlr.py:69-76).  Set to 0 to always drop, to None to always keep.
    PICKLE_FACTOR_MAX_N = 32768

    def _options_key(self):
        return tuple(sorted(self._opts.items()))

    def _native_opts(self):
        o = N.gh_chol_opts()
        o.device, o.nb = self._opts["device"], self._opts["nb"]
        o.profile, o.lookahead = int(self._opts["profile"]), int(self._opts["lookahead"])
        return o

    # the batched objective's handle (objective_batch): pooled under a key of its own, so that the factor of a GP's solver
    # handle and the bordered batch buffers never share (or evict) one another
    def _ensure_batch_handle(self):
        return self._take_handle("_bhandle", self._options_key() + (("batch", True),))

    # Pickling.  The reference's BasicSolver pickles computed (its factor is a NumPy array,
    # basic.py:68; tests/test_pickle.py:21-36); here the factor is downloaded (packed lower triangle +
    # diagonal-block inverses) into the state and uploaded again on first use after unpickling.
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_handle"] = None
        state.pop("_bhandle", None)
        state["_dk"] = None
        state.pop("_factor_state", None)
        keep = self._computed and self._handle is not None and (
            BasicSolver.PICKLE_FACTOR_MAX_N is None or self._n <= BasicSolver.PICKLE_FACTOR_MAX_N)
        if keep:
            h = self._handle
            L = np.empty(int(N.lib.gh_chol_factor_size(h)))
            dinv = np.empty(int(N.lib.gh_chol_dinv_size(h)))
            N.check(N.lib.gh_chol_export_factor(h, N.ptr(L), N.ptr(dinv)))
            state["_factor_state"] = (L, dinv)
        elif self._computed and getattr(self, "_factor_state", None) is not None:
            state["_factor_state"] = self._factor_state       # unpickled and never used: pass it on
        else:
            state["_computed"] = False
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_factor_state", None)

    def _restore(self):
        """Upload a pickled factor into a fresh native handle (first use after unpickling)."""
        L, dinv = self._factor_state
        self._dk = DeviceKernel(self.kernel)
        h = self._ensure_handle()
        N.check(N.lib.gh_chol_import_factor(h, self._n, self._x_host.shape[1], N.ptr(self._x_host), N.ptr(L), N.ptr(dinv),
                                            float(self._log_det)))
        if getattr(self, "_yerr_host", None) is not None:       # (append forms the last tile's old rows again: it needs them)
            N.check(N.lib.gh_chol_set_yerr(h, N.ptr(self._yerr_host)))
        self._factor_state = None

    # -- the solver protocol
    def _begin_compute(self, x, yerr, r=None):
        """``_check_inputs``, and a pickled factor that was never uploaded forgotten.  Returns ``(x, yerr, r)``."""
        x, yerr, r = self._check_inputs(x, yerr, r)
        self._factor_state = None
        return x, yerr, r

    def _end_compute(self, x, yerr, logdet):
        self._n = len(x)
        self._x_host = x                     # (the inputs travel with a pickled factor: predict / grad need them)
        self._yerr_host = yerr               # (... and append)
        self.log_determinant = logdet
        self.computed = True

    def _trim_grad(self, g):
        """the gradient buffer (at least one entry long) cut to the kernel's parameters"""
        return None if g is None else g[:self._dk.size]

    def compute(self, x, yerr):
        """basic.py:51-70.  ``yerr`` already contains the white noise (gp.py:330)."""
        x, yerr, _ = self._begin_compute(x, yerr)
        logdet = C.c_double(0.0)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_compute(
            hh, self._dk.handle, N.ptr(x), len(x), x.shape[1], N.ptr(yerr), C.byref(logdet))))
        self._end_compute(x, yerr, logdet.value)

    def objective(self, x, yerr, r, which=None, want_grad=True):
        """``compute(x, yerr)`` + ``r^T K^-1 r`` + (optionally) the kernel part of the gradient of the
        log-likelihood in ONE device call (gh_chol_objective; gp.py:470-480 with :303-337, :369-397,
        :429-466).  Returns ``(log_det, quad, grad_all | None, alpha | None, diagA | None)`` and leaves
        the solver computed."""
        x, yerr, r = self._begin_compute(x, yerr, r)
        n = len(x)
        logdet, quad = C.c_double(0.0), C.c_double(0.0)
        g = alpha = diagA = wh = None
        if want_grad:
            wh = np.ascontiguousarray(np.ones(max(self._dk.size, 1)) if which is None else which, dtype=np.uint32)
            g = np.zeros(max(self._dk.size, 1))
            alpha, diagA = np.empty(n), np.empty(n)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_objective(
            hh, self._dk.handle, N.ptr(x), n, x.shape[1], N.ptr(yerr), N.ptr(r), N.ptr(wh),
            C.byref(logdet), C.byref(quad), N.ptr(g), N.ptr(alpha), N.ptr(diagA))))
        self._end_compute(x, yerr, logdet.value)
        return logdet.value, quad.value, self._trim_grad(g), alpha, diagA

    # -- many parameter vectors at once (GP.log_likelihood_batch: emcee's ``vectorize=True``)
    # One chunk's bordered blocks, (Np + 128)^2 doubles per member, stay under this many bytes of device memory.
    BATCH_MAX_BYTES = 8 << 30
    # Largest N routed to the batched path by GP.log_likelihood_batch: above it one problem fills a third of the chip.
    BATCH_MAX_N = 8192

    def objective_batch(self, params, x, sigma, r):
        """B independent log-likelihood pieces over one set of points (gh_chol_objective_batch): member b has the
        kernel's structure with the FULL parameter vector ``params[b]`` (frozen entries included), standard deviations
        ``sigma[b]`` (white noise included) and residual ``r[b]``.  Returns ``(logdet (B,), quad (B,), info (B,))``;
        ``info[b] != 0`` (the 1-based failing pivot) marks a member that is not positive definite -- its logdet / quad
        are NaN.  Runs on a pooled handle of its own: this solver's factor, if any, is untouched."""
        params, x, sigma, r, _, dk, B, n = self._batch_args(params, x, sigma, r)
        logdet, quad, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int64)
        self._batch_chunks(B, self.objective_batch_bytes(n), lambda hh, b0, b1: N.lib.gh_chol_objective_batch(
            hh, dk.handle, N.ptr(params[b0:b1]), b1 - b0, N.ptr(x), n, x.shape[1], N.ptr(sigma[b0:b1]), N.ptr(r[b0:b1]),
            N.ptr(logdet[b0:]), N.ptr(quad[b0:]), N.ptr(info[b0:])))
        return logdet, quad, info

    def _batch_args(self, params, x, sigma, r, xs=None):
        """The checked, contiguous arguments of a batched call: ``(params, x, sigma (B, n), r, xs, DeviceKernel, B, n)``."""
        x = N.as_f64(x)
        if xs is None:
            if x.ndim != 2:
                raise ValueError("x must be (nsamples, ndim)")
        else:
            xs = N.as_f64(xs)
            if x.ndim != 2 or xs.ndim != 2:
                raise ValueError("x and xs must be (nsamples, ndim)")
        n = len(x)
        params = N.as_f64(params)
        B = params.shape[0] if params.ndim == 2 else -1
        dk = DeviceKernel(self.kernel)
        if B < 0 or params.shape[1] != dk.size:
            raise ValueError("params must be (B, {0})".format(dk.size))
        sigma = N.as_f64(np.broadcast_to(sigma, (B, n)))
        r = N.as_f64(r)
        if r.shape != (B, n):
            raise ValueError("dimension mismatch")
        if x.shape[1] != dk.ndim or (xs is not None and xs.shape[1] != dk.ndim):
            raise RuntimeError("dimension mismatch")
        return params, x, sigma, r, xs, dk, B, n

    def _batch_chunks(self, B, per, call):
        """Members 0 .. B - 1 in chunks whose device buffers (``per`` bytes a member) stay under BATCH_MAX_BYTES, one member
        at least: ``call(handle, b0, b1)`` returns the native status of members b0 .. b1 - 1, on the pooled batch handle."""
        chunk = int(max(1, min(B, BasicSolver.BATCH_MAX_BYTES // per)))
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            self._retry_without_parked_memory(lambda hh: N.check(call(hh, b0, b1)), ensure=self._ensure_batch_handle)

    @staticmethod
    def objective_batch_bytes(n):
        """Device bytes of one member of objective_batch: its bordered block, (Np + 128)^2, and the inverses of its diagonal
        blocks."""
        np_ = -(-n // 128) * 128
        return ((np_ + 128) ** 2 + np_ * 128) * 8

    def predict_batch(self, params, x, sigma, r, xs, return_var=False, return_cov=False):
        """B posterior predictions over one set of points (gh_chol_predict_batch): member b is objective_batch's member b,
        predicted at ``xs``.  Returns ``(mu (B, M), var (B, M) or None, cov (B, M, M) or None, info (B,))``; ``mu`` has no
        mean model (as :meth:`predict`), ``return_var`` wins over ``return_cov``, and a member with ``info[b] != 0`` has NaN
        rows.  Runs on objective_batch's pooled handle, in chunks under BATCH_MAX_BYTES."""
        params, x, sigma, r, xs, dk, B, n = self._batch_args(params, x, sigma, r, xs)
        m = len(xs)
        want_var = bool(return_var)
        want_cov = bool(return_cov) and not want_var
        mu = np.empty((B, m))
        var = np.empty((B, m)) if want_var else None
        cov = np.empty((B, m, m)) if want_cov else None
        info = np.zeros(B, dtype=np.int64)
        self._batch_chunks(B, self.predict_batch_bytes(n, m, want_var, want_cov), lambda hh, b0, b1: N.lib.gh_chol_predict_batch(
            hh, dk.handle, N.ptr(params[b0:b1]), b1 - b0, N.ptr(x), n, x.shape[1], N.ptr(sigma[b0:b1]), N.ptr(r[b0:b1]),
            N.ptr(xs), m, N.ptr(mu[b0:]), N.ptr(var[b0:]) if want_var else None,
            N.ptr(cov[b0:]) if want_cov else None, None, None, N.ptr(info[b0:])))
        return mu, var, cov, info

    @staticmethod
    def predict_batch_bytes(n, m, return_var=False, return_cov=False):
        """Device bytes of one member of predict_batch: its panel (Np + 128 + Mp rows of Np), the inverses of its diagonal
        blocks, its 128 x 128 output tiles (Mp / 128 + 1, plus the K** tiles) and its results in the caller's layout."""
        np_, mp = -(-n // 128) * 128, -(-m // 128) * 128
        mt = mp // 128
        kss = mt * (mt + 1) // 2 if return_cov and not return_var else mt if return_var else 0
        res = m + (m if return_var else m * m if return_cov else 0)
        return ((np_ + 128 + mp) * np_ + np_ * 128 + (mt + 1 + kss) * 128 * 128 + res) * 8

    def sample_conditional_batch(self, params, x, sigma, r, xs, z, tol=None, return_factor=False):
        """B sets of posterior draws over one set of points (gh_chol_sample_conditional_batch): member b is predict_batch's
        member b, its covariance factored on the device (pivoted Cholesky) and ``draws[b] = mu[b] + z[b] @ L_b.T`` for the
        caller's standard normals ``z`` (B, size, M).  Returns ``(draws (B, size, M), mu (B, M), rank (B,), info (B,))``,
        with ``fac`` (B, M, M) before ``rank`` when ``return_factor``; ``mu`` has no mean model.  A member with
        ``info[b] != 0`` has NaN rows and ``rank[b] == -1``.  ``tol=None``: each member's ``M * eps * max diag K_b(xs, xs)``.
        Runs on objective_batch's pooled handle, in chunks under BATCH_MAX_BYTES."""
        params, x, sigma, r, xs, dk, B, n = self._batch_args(params, x, sigma, r, xs)
        m = len(xs)
        z = N.as_f64(z)
        if z.ndim != 3 or z.shape[0] != B or z.shape[2] != m or z.shape[1] < 1:
            raise ValueError("z must be (B, size, {0})".format(m))
        nz = z.shape[1]
        draws, mu = np.empty((B, nz, m)), np.empty((B, m))
        fac = np.empty((B, m, m)) if return_factor else None
        rank, info = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        t = -1.0 if tol is None else float(tol)
        self._batch_chunks(B, self.sample_batch_bytes(n, m, nz), lambda hh, b0, b1: N.lib.gh_chol_sample_conditional_batch(
            hh, dk.handle, N.ptr(params[b0:b1]), b1 - b0, N.ptr(x), n, x.shape[1], N.ptr(sigma[b0:b1]), N.ptr(r[b0:b1]),
            N.ptr(xs), m, N.ptr(z[b0:b1]), nz, t, N.ptr(mu[b0:]), N.ptr(draws[b0:]),
            N.ptr(fac[b0:]) if return_factor else None, N.ptr(rank[b0:]), N.ptr(info[b0:])))
        if return_factor:
            return draws, mu, fac, rank, info
        return draws, mu, rank, info

    @staticmethod
    def sample_batch_bytes(n, m, nz):
        """Device bytes of one member of sample_conditional_batch: predict_batch's with a covariance, the padded factor, the
        padded normals and draws, their copies in the caller's layout, and the factor kernel's work arrays (its columns; above
        M = 512 also the padded matrix it updates)."""
        mp, zp = -(-m // 128) * 128, -(-nz // 128) * 128
        work = (min(m, 512) if m <= 512 else 128) * mp + mp + (mp * mp if m > 512 else 0)
        return BasicSolver.predict_batch_bytes(n, m, return_cov=True) + (
            mp * mp + 2 * zp * mp + 2 * m + nz * m + m * m + work) * 8

    def objective_grad_batch(self, params, x, sigma, r, which=None):
        """B log-likelihood pieces and kernel gradients over one set of points (gh_chol_objective_grad_batch): member b is
        objective_batch's member b.  ``which``: the kernel's parameter mask (all by default), shared by the members.
        Returns ``(logdet (B,), quad (B,), grad (B, kernel.full_size), alpha (B, N), diagA (B, N), info (B,))`` with
        ``grad[b] = 1/2 sum_ij A_ij dK_ij/dtheta`` (masked entries 0), ``alpha[b] = K_b^-1 r_b`` and ``diagA[b] =
        diag(alpha alpha^T - K_b^-1)``; a member with ``info[b] != 0`` has NaN rows.  Runs on objective_batch's pooled
        handle, in chunks under BATCH_MAX_BYTES."""
        params, x, sigma, r, _, dk, B, n = self._batch_args(params, x, sigma, r)
        wh = np.ones(max(dk.size, 1), dtype=np.uint32)
        if which is not None:
            which = np.asarray(which)
            if which.shape != (dk.size,):
                raise ValueError("which must have shape ({0},)".format(dk.size))
            wh[:dk.size] = which != 0
        logdet, quad, info = np.empty(B), np.empty(B), np.zeros(B, dtype=np.int64)
        grad, alpha, diagA = np.zeros((B, max(dk.size, 1))), np.empty((B, n)), np.empty((B, n))
        self._batch_chunks(B, self.grad_batch_bytes(n), lambda hh, b0, b1: N.lib.gh_chol_objective_grad_batch(
            hh, dk.handle, N.ptr(params[b0:b1]), b1 - b0, N.ptr(x), n, x.shape[1], N.ptr(sigma[b0:b1]),
            N.ptr(r[b0:b1]), N.ptr(wh), N.ptr(logdet[b0:]), N.ptr(quad[b0:]), N.ptr(grad[b0:]), N.ptr(alpha[b0:]),
            N.ptr(diagA[b0:]), N.ptr(info[b0:])))
        return logdet, quad, grad[:, :dk.size], alpha, diagA, info

    @staticmethod
    def grad_batch_bytes(n):
        """Device bytes of one member of objective_grad_batch: its panel (2 Np + 128 rows of Np: K, the residual tile, the
        identity rows that become L^-T), the inverses of its diagonal blocks, its 128 x 128 output tiles (Np / 128 + 1 for
        -z^T z and -alpha, the lower tiles of -K^-1), its results (grad, alpha, diagA) and the partial rows of the gradient
        reduction, both counted at the largest parameter count (64)."""
        np_ = -(-n // 128) * 128
        nt, gm = np_ // 128, -(-n // 64)
        q = nt + 1 + nt * (nt + 1) // 2
        return ((2 * np_ + 128) * np_ + np_ * 128 + q * 128 * 128 + 64 + 2 * n + gm * (gm + 1) // 2 * 64) * 8

    def _need(self):
        if self._computed and self._handle is None and getattr(self, "_factor_state", None) is not None:
            self._restore()
        return super(BasicSolver, self)._need()

    # -- sequential use (no reference counterpart: basic.py:51-70 always refactorises)
    @property
    def appendable(self):
        """Does the solver hold what ``append`` needs beside the factor -- the error bars of its points?  (Not when it was
        restored from a state pickled without them; ``GP.append`` then computes afresh.)"""
        return getattr(self, "_yerr_host", None) is not None

    def append(self, x_new, yerr_new):
        """Extend the computed factor by the points ``x_new`` (m, ndim) with standard deviations ``yerr_new`` (white noise
        included), gh_chol_append: the rows of the full 128-row tiles are not touched.  The kernel is the one of
        ``compute``.  ``LinAlgError`` (the extended matrix is not positive definite) leaves the solver as it was."""
        self._need()
        if not self.appendable:
            raise RuntimeError("this solver was restored without the error bars of its points: compute() again")
        x_new = N.as_f64(x_new)
        if x_new.ndim != 2:
            raise ValueError("x_new must be (nsamples, ndim)")
        if x_new.shape[1] != self._x_host.shape[1]:
            raise RuntimeError("dimension mismatch")
        m = len(x_new)
        if m == 0:
            return
        yerr_new = N.as_f64(np.zeros(m) + yerr_new)
        logdet = C.c_double(0.0)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_append(
            hh, self._dk.handle, N.ptr(x_new), m, N.ptr(yerr_new), C.byref(logdet))))
        self._n += m
        self._x_host = np.ascontiguousarray(np.concatenate([self._x_host, x_new]))
        self._yerr_host = np.ascontiguousarray(np.concatenate([self._yerr_host, yerr_new]))
        self.log_determinant = logdet.value

    def truncate(self, n):
        """Keep the first ``n`` points of the computed factor (gh_chol_truncate): data movement and one log-det reduction."""
        self._need()
        n = int(n)
        if not 0 < n <= self._n:
            raise ValueError("truncate: n must be in 1 .. {0}".format(self._n))
        if n == self._n:
            return
        logdet = C.c_double(0.0)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_truncate(hh, n, C.byref(logdet))))
        self._n = n
        self._x_host = np.ascontiguousarray(self._x_host[:n])
        if self.appendable:
            self._yerr_host = np.ascontiguousarray(self._yerr_host[:n])
        self.log_determinant = logdet.value

    # Where ``remove`` computes afresh on the kept points instead of updating the factor: above REMOVE_MAX_POINTS removed points,
    # below REMOVE_MIN_N points in the factor.  NOT yet set from a measurement: scripts/bench_remove.py writes the table
    # (profiles/remove/remove_time.json) these are to be read from, and that file does not exist yet.  Until then, from the
    # counts ("Removing points"): a pass of up to 128 points costs at most N^2 * 512 flops against
    # compute's N^3 / 3, so eight passes stay below compute from N = 12288 up; no lower bound on N.
    REMOVE_MAX_POINTS = 1024
    REMOVE_MIN_N = 0

    def remove(self, indices):
        """Take the points ``indices`` (strictly increasing integers in ``0 .. n-1``, fewer than ``n``) out of the computed
        factor, gh_chol_remove: a rank-m update of the gathered factor -- no kernel evaluations, no error bars; the rows in
        front of the first removed index keep their bits.  A trailing run is ``truncate``.  More than ``REMOVE_MAX_POINTS``
        points, or a factor below ``REMOVE_MIN_N``, are computed afresh on the kept points by this solver's own ``compute``
        (which needs the error bars: ``RuntimeError`` when the solver is not ``appendable``).  ``last_remove_path`` records
        which way the call went: "update", "truncate" or "compute".  Any exception leaves the solver as it was."""
        h = self._need()
        idx = np.ascontiguousarray(np.atleast_1d(np.asarray(indices)))
        if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
            raise ValueError("remove: indices must be a one-dimensional integer array")
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        m, n = len(idx), self._n
        N.check(N.lib.gh_debug_check_remove_args(n, N.ptr(idx), m))      # (the native rule, before any routing)
        trailing = int(idx[0]) == n - m
        keep = np.ones(n, dtype=bool)
        keep[idx] = False
        rc = N.GH_REFACTORIZE
        if trailing or (m <= self.REMOVE_MAX_POINTS and n >= self.REMOVE_MIN_N):
            logdet = C.c_double(0.0)

            def call(hh):
                rc = N.lib.gh_chol_remove(hh, N.ptr(idx), m, C.byref(logdet))
                if rc != N.GH_REFACTORIZE:
                    N.check(rc)
                return rc
            rc = self._retry_without_parked_memory(call)
        if rc == N.GH_REFACTORIZE:
            if not self.appendable:
                raise RuntimeError("this solver was restored without the error bars of its points: compute() again")
            # (on a solver of its own, adopted only once it is computed: whatever compute() raises leaves this one as it was)
            fresh = type(self)(self.kernel, **self._opts)
            fresh.compute(self._x_host[keep], self._yerr_host[keep])
            self.__dict__, fresh.__dict__ = fresh.__dict__, self.__dict__
            del fresh                                     # (the old handle goes back to the pool)
            self.last_remove_path = "compute"
            return
        self._n = n - m
        self._x_host = np.ascontiguousarray(self._x_host[keep])
        if self.appendable:
            self._yerr_host = np.ascontiguousarray(self._yerr_host[keep])
        self.log_determinant = logdet.value
        self.last_remove_path = "truncate" if trailing else "update"

    def _solve_target(self, y, yc, in_place):
        """``in_place``: the solve writes straight into a writable contiguous float64 ``y``; any other array gets the values
        copied back"""
        if not (in_place and isinstance(y, np.ndarray)):
            return np.empty_like(yc), None
        if y.dtype == np.float64 and y.flags.c_contiguous and y.flags.writeable:
            return y, None
        return np.empty_like(yc), y

    # -- fused, device-resident GP glue (optional protocol extensions)
    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """mean / variance / covariance terms of gp.py:532-545 for residual ``r = y - mean``:
        returns ``K* K^-1 r`` and (optionally) ``diag`` or full ``K** - K* K^-1 K*^T``."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = rhs_vector(r, self._n), N.as_f64(xs)
        m = len(xs)
        mu = np.empty(m)
        var = np.empty(m) if return_var else None
        cov = np.empty((m, m)) if return_cov else None
        N.check(N.lib.gh_chol_predict(h, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(var), N.ptr(cov)))
        return mu, var, cov

    def predict_gradient(self, kernel, r, xs, return_var=False, return_value=True):
        """:meth:`predict` and its derivatives with respect to the test points for residual ``r = y - mean``
        (gh_chol_predict_grad, one device call): returns ``(mu (M,), var | None, dmu (M, ndim), dvar | None)`` with
        ``dmu[c, d] = sum_i G[c, i, d] alpha[i]`` and ``dvar[c, d] = D[c, d] - 2 sum_i G[c, i, d] (K^-1 K(x, xs))[i, c]``,
        ``G = kernel.get_x1_gradient(xs, x)`` (never stored) and ``D`` the x1- plus x2-gradient of the kernel at
        ``(xs_c, xs_c)``; ``mu`` and ``var`` are :meth:`predict`'s bit for bit, without a mean model.  ``return_value=False``
        leaves ``mu`` and ``var`` out (``None``); without ``return_var`` too the call needs ``alpha`` only -- two sweeps instead
        of a substitution with M right-hand sides -- and ``dmu`` has the same bits."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = rhs_vector(r, self._n), N.as_f64(xs)
        if xs.ndim != 2 or xs.shape[1] != dk.ndim:
            raise ValueError("xs must be (M, {0})".format(dk.ndim))
        m = len(xs)
        dmu = np.empty((m, dk.ndim))
        mu = np.empty(m) if return_value else None
        var = np.empty(m) if (return_var and return_value) else None
        dvar = np.empty((m, dk.ndim)) if return_var else None
        if m > 0:
            self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_predict_grad(
                hh, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(var), N.ptr(dmu), N.ptr(dvar))))
        return mu, var, dmu, dvar

    def sample_conditional(self, kernel, r, xs, z, tol=None, return_factor=False):
        """Posterior draws for residual ``r = y - mean`` at ``xs`` (gh_chol_sample_conditional): the mean and covariance of
        :meth:`predict`, the covariance factored on the device by a pivoted Cholesky with rank truncation (it never reaches
        the host), ``draws = mu + z @ L.T`` for the caller's standard normals ``z`` (size, M).  Returns
        ``(draws (size, M), mu (M,), rank)``, with ``L`` (M, M) before ``rank`` when ``return_factor``; ``mu`` has no mean
        model.  ``tol=None``: ``M * eps * max diag K(xs, xs)``."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = rhs_vector(r, self._n), N.as_f64(xs)
        m = len(xs)
        z = N.as_f64(z)
        if z.ndim != 2 or z.shape[1] != m or z.shape[0] < 1:
            raise ValueError("z must be (size, {0})".format(m))
        draws, mu = np.empty_like(z), np.empty(m)
        fac = np.empty((m, m)) if return_factor else None
        rank = np.zeros(1, dtype=np.int64)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_sample_conditional(
            hh, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(z), len(z), -1.0 if tol is None else float(tol),
            N.ptr(mu), N.ptr(draws), N.ptr(fac), N.ptr(rank))))
        if return_factor:
            return draws, mu, fac, int(rank[0])
        return draws, mu, int(rank[0])

    def grad(self, r, which):
        """kernel part of gp.py:429-466: returns (grad over ALL kernel params (masked ones 0),
        alpha = K^-1 r, diag(alpha alpha^T - K^-1))."""
        return self._grad("gh_chol_grad", r, which)

    # -- leave-one-out cross-validation (no reference counterpart; GPML 5.4.2)
    def _cv_grad_outputs(self, which):
        """``(wh, g, v, diagB)`` of :meth:`loo` and :meth:`lgo`: the parameter mask as the device reads it and the buffers of
        the gradient outputs (:meth:`_trim_grad` cuts ``g``); all ``None`` without a mask."""
        if which is None:
            return None, None, None, None
        size, n = self._dk.size, self._n
        which = np.asarray(which)
        if which.shape != (size,):
            raise ValueError("which must have shape ({0},)".format(size))
        wh = np.zeros(max(size, 1), dtype=np.uint32)
        wh[:size] = which != 0
        return wh, np.zeros(max(size, 1)), np.empty(n), np.empty(n)

    def loo(self, r, which=None):
        """Leave-one-out quantities of the computed factor for residual ``r = y - mean`` (gh_chol_loo).  Returns
        ``(lpd_sum, resid, var, lpd, grad_full | None, v | None, diagB | None)``: ``resid = y - mu_loo``, ``var`` the
        leave-one-out variances, ``lpd`` the N log predictive densities and ``lpd_sum`` their sum.  ``which=None``: values only
        -- K^-1 is not formed.  With a parameter mask also ``grad_full`` = d lpd_sum / d theta over ALL kernel parameters
        (masked ones exactly 0), ``v`` = d lpd_sum / d mean_i and ``diagB`` = d lpd_sum / d K_ii."""
        h = self._need()
        r = rhs_vector(r, self._n)
        n = self._n
        total = C.c_double(0.0)
        resid, var, lpd = np.empty(n), np.empty(n), np.empty(n)
        wh, g, v, diagB = self._cv_grad_outputs(which)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_loo(
            hh, self._dk.handle, N.ptr(wh), N.ptr(r), C.byref(total), N.ptr(resid), N.ptr(var), N.ptr(lpd),
            N.ptr(g), N.ptr(v), N.ptr(diagB))))
        return total.value, resid, var, lpd, self._trim_grad(g), v, diagB

    def loo_objective(self, x, yerr, r, which=None, want_grad=True):
        """``compute(x, yerr)`` + :meth:`loo` in ONE device call (gh_chol_loo_objective), the leave-one-out analogue of
        :meth:`objective`.  Returns ``(log_det, lpd_sum, resid, var, grad_full | None, v | None, diagB | None)`` and leaves
        the solver computed."""
        x, yerr, r = self._begin_compute(x, yerr, r)
        n = len(x)
        logdet, total = C.c_double(0.0), C.c_double(0.0)
        resid, var = np.empty(n), np.empty(n)
        g = v = diagB = wh = None
        if want_grad:
            wh = np.ascontiguousarray(np.ones(max(self._dk.size, 1)) if which is None else which, dtype=np.uint32)
            g = np.zeros(max(self._dk.size, 1))
            v, diagB = np.empty(n), np.empty(n)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_loo_objective(
            hh, self._dk.handle, N.ptr(x), n, x.shape[1], N.ptr(yerr), N.ptr(r), N.ptr(wh),
            C.byref(logdet), C.byref(total), N.ptr(resid), N.ptr(var), N.ptr(g), N.ptr(v), N.ptr(diagB))))
        self._end_compute(x, yerr, logdet.value)
        return logdet.value, total.value, resid, var, self._trim_grad(g), v, diagB

    # -- leave-group-out cross-validation (no reference counterpart)
    LGO_MAX_GROUP = 128      # points of one group in the device form: one tile of the batched Cholesky

    def lgo(self, r, order, start, which=None, want_cov=False):
        """Leave-group-out quantities of the computed factor for residual ``r = y - mean`` (gh_chol_lgo).  ``order`` (n)
        lists the point indices sorted by group, ``start`` (G + 1) the groups' offsets into it; a group has at most
        ``LGO_MAX_GROUP`` points.  Returns ``(lpd_sum, resid, var, lpd, cov_blocks | None, grad_full | None, v | None,
        diagB | None)``: ``resid = y - mu`` of every point predicted jointly with its group from all other groups and ``var``
        its variance, both in the caller's point order, ``lpd`` the G joint log predictive densities, ``cov_blocks`` (with
        ``want_cov``) the G predictive covariances, rows in the order of ``order``.  ``which=None``: values only -- K^-1 is not
        formed.  With a parameter mask also ``grad_full`` = d lpd_sum / d theta over ALL kernel parameters (masked ones
        exactly 0), ``v`` = d lpd_sum / d mean_i and ``diagB`` = d lpd_sum / d K_ii."""
        h = self._need()
        n = self._n
        r = rhs_vector(r, n)
        order = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
        start = np.ascontiguousarray(start, dtype=np.int64).reshape(-1)
        if len(order) != n or len(start) < 2:
            raise ValueError("order must have one entry per point and start one more than there are groups")
        G = len(start) - 1
        total = C.c_double(0.0)
        resid, var, lpd = np.empty(n), np.empty(n), np.empty(G)
        sizes = np.diff(start)
        cov = None
        if want_cov:
            if G > n or np.any(sizes < 0) or np.any(sizes > self.LGO_MAX_GROUP):
                raise ValueError("a group is empty or has more than {0} points".format(self.LGO_MAX_GROUP))
            cov = np.empty(int(np.sum(sizes ** 2)))
        wh, g, v, diagB = self._cv_grad_outputs(which)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_lgo(
            hh, self._dk.handle, N.ptr(wh), N.ptr(r), N.ptr(order), N.ptr(start), G, C.byref(total), N.ptr(resid), N.ptr(var),
            N.ptr(lpd), N.ptr(cov), N.ptr(g), N.ptr(v), N.ptr(diagB))))
        blocks = None
        if want_cov:
            at = np.concatenate([[0], np.cumsum(sizes ** 2)])
            blocks = [cov[at[i]:at[i + 1]].reshape(sizes[i], sizes[i]) for i in range(G)]
        return total.value, resid, var, lpd, blocks, self._trim_grad(g), v, diagB

    # -- expected information of the hyper-parameters (no reference counterpart)
    # The default budget of fisher().  Nobody has measured a good value: it stands on what _POOL_MAX_BYTES already assumes
    # about the card -- that solver handles may hold that much of it, work arrays included.  The planes belong to the handle
    # and are parked with it; a call that grew them beyond this would only have its handle trimmed or destroyed at the next
    # park.  Blocking only ever adds products (every plane behind a block is formed again for it), so a larger budget is
    # only ever faster.
    FISHER_MAX_BYTES = _POOL_MAX_BYTES

    @staticmethod
    def fisher_bytes(n, n_planes):
        """Device bytes of :meth:`fisher` with ``n_planes`` derivative planes resident beside L^-1 and the intermediate
        product: ``(2 + n_planes) * 8 * Np^2``, Np = n rounded up to 128.  As ``max_bytes`` it makes the call keep exactly
        that many planes (a block of ``n_planes - 1`` and one scratch plane when there are more parameters)."""
        np_ = -(-n // 128) * 128
        return (2 + int(n_planes)) * 8 * np_ * np_

    def fisher(self, which=None, diag_rows=None, max_bytes=None):
        """Expected (Fisher) information ``F[a, b] = 1/2 tr(K^-1 D_a K^-1 D_b)`` of the computed factor (gh_chol_fisher):
        ``(n_diag + size, n_diag + size)`` over the ``n_diag`` diagonal derivative matrices ``diag(diag_rows[p])`` followed by
        ALL kernel parameters (those masked out by ``which`` have rows and columns of exactly 0; ``which=None``: all of
        them).  ``max_bytes`` (default ``FISHER_MAX_BYTES``) bounds the call's work arrays (:meth:`fisher_bytes`); the result
        has the same bits for every budget the call accepts and ``MemoryError`` is raised when not even two planes fit."""
        h = self._need()
        size = self._dk.size
        wh = np.ones(max(size, 1), dtype=np.uint32)
        if which is not None:
            which = np.asarray(which)
            if which.shape != (size,):
                raise ValueError("which must have shape ({0},)".format(size))
            wh[:size] = which != 0
        rows = None
        n_diag = 0
        if diag_rows is not None:
            rows = N.as_f64(diag_rows)
            if rows.ndim != 2 or rows.shape[1] != self._n:
                raise ValueError("diag_rows must be (n_diag, {0})".format(self._n))
            n_diag = rows.shape[0]
            if n_diag > 64:
                raise ValueError("at most 64 diagonal parameters")
        p = n_diag + size
        out = np.zeros((p, p))
        if p == 0:
            return out
        budget = int(self.FISHER_MAX_BYTES if max_bytes is None else max_bytes)
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_chol_fisher(
            hh, self._dk.handle, N.ptr(wh), N.ptr(rows) if n_diag else None, n_diag, budget, N.ptr(out))))
        return out

    def profile(self):
        p = N.gh_chol_profile()
        N.check(N.lib.gh_chol_get_profile(self._need(), C.byref(p)))
        return dict(ms_total=p.ms_total, ms_build=p.ms_build, ms_panel=p.ms_panel, ms_trailing=p.ms_trailing,
                    trailing_flops=p.trailing_flops, n_trailing=p.n_trailing, ms_solve=p.ms_solve,
                    ms_append_relayout=p.ms_append_relayout, ms_remove_gather=p.reserved[0])
