"""``HODLRSolver`` -- level-batched HODLR factorisation on one MI355X.

Drop-in for the reference's ``HODLRSolver`` (``src/george/solvers/hodlr.py:13-76``
over ``_hodlr.cpp`` / ``include/george/hodlr.h``): same constructor keywords
(``min_size=100, tol=0.1, seed=42``), same methods, ``apply_sqrt`` raises
``NotImplementedError`` (hodlr.py:62-64), pickling drops the factor (:69-76).
"""
import ctypes as C
import warnings

from .. import _native as N
from .basic import BasicSolver
from .protocol import HandlePool, NativeSolver

__all__ = ["HODLRSolver"]


class HODLRSolver(NativeSolver):

    _CREATE, _DESTROY = "gh_hodlr_create", "gh_hodlr_destroy"
    _SOLVE, _DOT_SOLVE, _GET_INVERSE = "gh_hodlr_solve", "gh_hodlr_dot_solve", "gh_hodlr_get_inverse"

    # hodlr.h:147 lets a block's rank grow to min(rows, cols); the level-batched ACA here stops at 1024
    # columns.  A block that needs more (3-D inputs at tight tolerances: docs/user/solvers.rst:40-42) is
    # not low-rank in any useful sense -- the reference then spends O(N r^2) on it -- and up to this many
    # points the solver answers with the EXACT dense device factorisation instead (BasicSolver on the
    # same GPU: every tolerance is met; ``dense_fallback`` is set and a warning is issued); beyond it,
    # or when an explicit ``max_rank`` is too small, compute() raises ValueError.  Never a truncation.
    DENSE_FALLBACK_MAX_N = 98304          # 8 N^2 = 77 GB of the 288 GB

    def __init__(self, kernel, min_size=100, tol=0.1, seed=42, device=0, max_rank=0):
        # max_rank = 0: ranks grow as far as ``tol`` asks (hodlr.h:147), up to the solver's ceiling of
        # 1024 (then: dense fallback, above); an explicit ``max_rank`` that is too small raises ValueError.
        self.dense_fallback = False
        self._dense = None
        self.min_size = min_size
        self.tol = tol
        self.seed = seed
        self._opts = dict(device=int(device), max_rank=int(max_rank))
        super(HODLRSolver, self).__init__(kernel)

    # A native handle keeps its tree, its per-level job tables on the device and the measured schedule of its
    # last compute(): inside an optimiser loop (GP makes a NEW solver object per compute, gp.py:327) a fresh handle
    # per iterate cost 3 of the 8.4 ms of a C4 step through this class.  Handles of dropped solvers are parked per
    # option set (at most _HPOOL_MAX each) and picked up by the next solver with the same options.
    _HPOOL_MAX = 2
    _HPOOL_TOTAL = 4           # over all option sets: a scan over tolerances must not leave a trail of parked handles
    _HPOOL = HandlePool(_DESTROY, _HPOOL_MAX, _HPOOL_TOTAL)
    # out of memory: this solver's own handle first, then what dead solvers left parked: both handle pools and the native
    # block cache
    _GIVES_BACK_POOLS = (_HPOOL, BasicSolver._POOL)

    def _options_key(self):
        return (self._opts["device"], int(self.min_size), int(self.seed), self._opts["max_rank"], float(self.tol))

    def _native_opts(self):
        o = N.gh_hodlr_opts()
        o.device, o.min_size, o.seed, o.max_rank, o.tol = self._options_key()
        return o

    def compute(self, x, yerr):
        x, yerr, _ = self._check_inputs(x, yerr)
        if self._handle is not None and self._handle_key != self._options_key():
            self._park_handle()               # options were changed on the instance
        logdet = C.c_double(0.0)
        self.dense_fallback, self._dense = False, None
        try:
            self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_hodlr_compute(
                hh, self._dk.handle, N.ptr(x), len(x), x.shape[1], N.ptr(yerr), C.byref(logdet))))
        except N.RankCeilingError as e:
            if len(x) > HODLRSolver.DENSE_FALLBACK_MAX_N:
                raise
            warnings.warn("HODLRSolver: %s -- answering with the dense device solver (exact)" % (e,), RuntimeWarning)
            self._destroy_handle()                        # (frees the HODLR scratch before the N x N matrix is built)
            self._dense = BasicSolver(self.kernel, device=self._opts["device"])
            self._dense.compute(x, yerr)
            self.dense_fallback = True
        self._n = len(x)
        self._log_det = self._dense.log_determinant if self.dense_fallback else logdet.value
        self.computed = True

    # -- the solver protocol: a dense-fallback solver answers with the dense forms
    def apply_inverse(self, y, in_place=False):
        # the reference's pybind/Eigen binding always returns a fresh array: the base's policy
        if self._computed and self._dense is not None:
            return self._dense.apply_inverse(y, in_place=False)
        return super(HODLRSolver, self).apply_inverse(y)

    def dot_solve(self, y):
        if self._computed and self._dense is not None:
            return self._dense.dot_solve(y)
        return super(HODLRSolver, self).dot_solve(y)

    def get_inverse(self):
        if self._computed and self._dense is not None:
            return self._dense.get_inverse()
        return super(HODLRSolver, self).get_inverse()

    def ranks(self):
        if self._computed and self._dense is not None:
            return []                             # (no low-rank blocks: the dense factorisation answered)
        buf = (C.c_int32 * 65536)()
        cnt = C.c_int32(0)
        N.check(N.lib.gh_hodlr_ranks(self._need(), buf, 65536, C.byref(cnt)))
        return list(buf[:cnt.value])

    # pickling drops the factor and flags the solver un-computed (hodlr.py:69-76)
    def __getstate__(self):
        state = super(HODLRSolver, self).__getstate__()
        state["_dense"] = None
        state["dense_fallback"] = False          # (it described the factor that is not pickled)
        return state

    # -- fused, device-resident GP glue on the factor (gh_hodlr_predict / gh_hodlr_grad: column strips, no M x N or N x N
    #    array on the host); a dense-fallback solver answers with the dense forms
    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """``BasicSolver.predict`` on the HODLR factor: ``K* K^-1 r`` and (optionally) the diagonal or the whole of
        ``K** - K* K^-1 K*^T`` (gp.py:532-545).  The covariance keeps two N x M blocks on the device and raises
        ``MemoryError`` when they do not fit."""
        if self._computed and self._dense is not None:
            return self._dense.predict(kernel, r, xs, return_var=return_var, return_cov=return_cov)
        return self._predict("gh_hodlr_predict", kernel, r, xs, return_var, return_cov)

    def grad(self, r, which):
        """``BasicSolver.grad`` on the HODLR factor: (grad over ALL kernel parameters (masked ones 0), alpha = K^-1 r,
        diag(alpha alpha^T - K^-1)) with the solver's own K^-1, a strip of its columns at a time (gp.py:429-466)."""
        if self._computed and self._dense is not None:
            return self._dense.grad(r, which)
        return self._grad("gh_hodlr_grad", r, which)
