"""``VecchiaSolver`` -- the nearest-neighbour (Vecchia) approximation on one MI355X, for data sets no N x N factor fits:
10^5 - 10^6 points in any number of input dimensions.

The joint density is replaced by a product of conditionals, ``p(y) ~ prod_i p(y_i | y_c(i))``, where ``c(i)`` holds at most
``m`` points among the predecessors of ``i`` in a fixed order.  That is a proper Gaussian density with the sparse precision
``Q = (I - B)^T F^-1 (I - B)``: O(N m^3) flops, O(N m) memory, no probe vectors, no iteration counts.  With every predecessor
in the conditioning set (``m >= N - 1``) it is the dense likelihood up to rounding; smooth kernels with little noise need a
larger ``m`` than rough or noisy ones.  No reference counterpart.  The device side is ``george_amd/csrc/gh_vecchia.hip``.

Not built: ordering strategies beyond the three of ``order=`` (max-min and the like), and ``apply_sqrt``.
"""
import atexit
import ctypes as C
import hashlib

import numpy as np

from .. import _native as N
from .protocol import NativeSolver, rhs_matrix, rhs_vector

__all__ = ["VecchiaSolver", "vecchia_neighbors"]

M_MAX = 64


def _nearest_predecessors(x, rows, cand, m):
    """For each row ``i`` of ``rows`` the ``min(#, m)`` nearest of its candidates ``cand`` (len(rows), k; entries >= i or
    >= len(x) do not count) by squared Euclidean distance, ties to the lower index: ``(table (len(rows), m) sorted
    ascending and padded with -1, the m-th smallest distance or inf)``."""
    n = len(x)
    valid = cand < rows[:, None]
    safe = np.where(valid, cand, 0)
    d2 = ((x[safe] - x[rows][:, None, :]) ** 2).sum(axis=-1)
    d2 = np.where(valid, d2, np.inf)
    key = np.where(valid, cand, n)
    pick = np.lexsort((key, d2), axis=1)[:, :m]                     # by distance, then by index
    sel = np.take_along_axis(key, pick, axis=1)
    dm = np.take_along_axis(d2, pick, axis=1)
    if sel.shape[1] < m:
        sel = np.concatenate([sel, np.full((len(rows), m - sel.shape[1]), n)], axis=1)
        dm = np.concatenate([dm, np.full((len(rows), m - dm.shape[1]), np.inf)], axis=1)
    sel = np.sort(sel, axis=1)                                      # (the fill value n sorts last)
    return np.where(sel >= n, -1, sel).astype(np.int32), dm[:, m - 1]


def vecchia_neighbors(x, m):
    """The default conditioning sets: row ``i`` holds the ``min(i, m)`` nearest predecessors of point ``i`` under the
    Euclidean distance on ``x`` as given, ties going to the lower index, sorted ascending and padded with -1.  (N, m)
    int32.  The table depends on ``x`` only, so it stays fixed while an optimiser moves the hyper-parameters.

    Exact for every N: it equals the brute-force search.  Strictly increasing 1-D input takes the previous ``m`` points;
    everything else goes through ``scipy.spatial.cKDTree`` with a query size that grows until the ``m`` nearest
    predecessors are certain, and a direct search for the first rows."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError("x must be (nsamples, ndim)")
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    n = len(x)
    table = np.full((n, m), -1, dtype=np.int32)
    if n == 0:
        return table
    if x.shape[1] == 1 and np.all(np.diff(x[:, 0]) > 0):
        idx = np.arange(n)[:, None] - np.arange(m, 0, -1)[None, :]          # i - m .. i - 1
        idx = np.where(idx >= 0, idx, n)
        idx.sort(axis=1)
        return np.where(idx >= n, -1, idx).astype(np.int32)
    # the first rows directly: every predecessor is a candidate
    n0 = min(n, 4 * m + 64)
    rows = np.arange(n0)
    table[:n0] = _nearest_predecessors(x, rows, np.broadcast_to(np.arange(n0)[None, :], (n0, n0)), m)[0]
    if n0 == n:
        return table
    from scipy.spatial import cKDTree
    tree = cKDTree(x)
    todo, k = np.arange(n0, n), min(n, 2 * m + 2)
    while len(todo):
        again = []
        step = max(1, (1 << 22) // (k * x.shape[1]))                        # rows per query: the candidates' coordinates in 32 MB
        for s in range(0, len(todo), step):
            rows = todo[s:s + step]
            dist, cand = tree.query(x[rows], k=k)
            if k == 1:
                dist, cand = dist[:, None], cand[:, None]
            tab, dm = _nearest_predecessors(x, rows, cand, m)
            # every point the query left out is at least dist[:, -1] away: the choice is certain when the m-th chosen one is
            # nearer than that by more than the two routes' rounding (or when the query returned every point)
            sure = (np.sqrt(dm) < dist[:, -1] * (1.0 - 1e-9)) if k < n else np.ones(len(rows), dtype=bool)
            table[rows[sure]] = tab[sure]
            again.append(rows[~sure])
        todo, k = np.concatenate(again), min(n, 2 * k)
    return table


def _check_neighbors(nbr, n, m):
    """the (n, m) table as contiguous int32: every entry of row i is -1 or in [0, i), none twice in a row"""
    nbr = np.asarray(nbr)
    if nbr.shape != (n, m) or nbr.dtype.kind not in "iu":
        raise ValueError("neighbors must be an integer table of shape ({0}, {1})".format(n, m))
    if n == 0:
        return np.ascontiguousarray(nbr, dtype=np.int32)
    if np.any(nbr < -1) or np.any(nbr >= np.arange(n)[:, None]):
        raise ValueError("neighbors: every entry of row i must be -1 or one of the predecessors 0 .. i - 1")
    s = np.sort(nbr, axis=1)
    if np.any((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)):
        raise ValueError("neighbors: an entry appears twice in a row")
    return np.ascontiguousarray(nbr, dtype=np.int32)


class VecchiaSolver(NativeSolver):
    """``VecchiaSolver(kernel, m=32, order=None, neighbors=None, device=0)``.

    ``m``: neighbours per point, 1 .. 64.  ``order``: ``None`` (the caller's order), ``"coordinate"`` (a stable argsort of
    the first input column) or a permutation array (solver position -> caller's index); the solver permutes its inputs on
    the way in and un-permutes ``alpha``, ``diagA`` and solve results on the way out.  ``neighbors``: ``None``
    (:func:`vecchia_neighbors` of the ordered inputs) or an (N, m) integer table IN SOLVER ORDER, padded with -1; entries
    need not be sorted."""

    def __init__(self, kernel, m=32, order=None, neighbors=None, device=0):
        m = int(m)
        if m < 1 or m > M_MAX:
            raise ValueError("VecchiaSolver: 1 <= m <= {0}, not {1}".format(M_MAX, m))
        if isinstance(order, str) and order != "coordinate":
            raise ValueError("VecchiaSolver: order is None, 'coordinate' or a permutation")
        self.m = m
        self.order = order
        self.neighbors = neighbors
        self.failed_point = None
        self._vopts = dict(device=int(device))
        self._perm = None
        super(VecchiaSolver, self).__init__(kernel)

    # The default table depends on the ordered inputs and m only, and GP makes a new solver for every compute (one per iterate
    # of an optimiser): the last tables are kept, keyed by a digest of the inputs.
    _TABLES = []
    _TABLES_MAX = 2

    def _default_table(self, x):
        key = (x.shape, self.m, hashlib.blake2b(memoryview(x).cast("B"), digest_size=16).digest())
        for k, tab in VecchiaSolver._TABLES:
            if k == key:
                return tab
        tab = vecchia_neighbors(x, self.m)
        VecchiaSolver._TABLES.append((key, tab))
        del VecchiaSolver._TABLES[:-VecchiaSolver._TABLES_MAX]
        return tab

    # -- lifetime.  GP makes a new solver for every compute: the handle of a dropped solver (its neighbour table checked, indexed
    # and on the device) is parked, at most _HPOOL_MAX per (device, m), and picked up by the next solver with the same options.
    _HPOOL = {}
    _HPOOL_MAX = 2

    def _ensure_handle(self):
        if self._handle is None:
            self._hkey = (self._vopts["device"], self.m)
            free = VecchiaSolver._HPOOL.get(self._hkey)
            if free:
                self._handle = free.pop()
                return self._handle
            o = N.gh_vecchia_opts()
            o.device, o.m = self._hkey
            h = N._vp()
            N.check(N.lib.gh_vecchia_create(C.byref(o), C.byref(h)))
            self._handle = h
        return self._handle

    def _destroy_handle(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None and h.value:
            N.lib.gh_vecchia_destroy(h)

    def __del__(self):
        try:
            h, self._handle = getattr(self, "_handle", None), None
            if h is not None and h.value:
                free = VecchiaSolver._HPOOL.setdefault(self._hkey, [])
                if len(free) < VecchiaSolver._HPOOL_MAX:
                    free.append(h)
                else:
                    N.lib.gh_vecchia_destroy(h)
        except Exception:
            pass

    @classmethod
    def release_pool(cls):
        """Destroy every parked native handle (frees their device memory)."""
        for free in cls._HPOOL.values():
            while free:
                try:
                    N.lib.gh_vecchia_destroy(free.pop())
                except Exception:
                    pass
        cls._HPOOL.clear()

    def _release_parked_memory(self):
        self._destroy_handle()
        VecchiaSolver.release_pool()
        N.lib.gh_release_caches(self._vopts["device"])

    def __getstate__(self):
        state = super(VecchiaSolver, self).__getstate__()
        state["_perm"] = None
        return state

    def _permutation(self, x):
        """``order`` as an index array (solver position -> caller's index), or None for the caller's order"""
        if self.order is None:
            return None
        n = len(x)
        if isinstance(self.order, str):
            return np.argsort(x[:, 0], kind="stable")
        perm = np.asarray(self.order)
        if perm.shape != (n,) or perm.dtype.kind not in "iu" or not np.array_equal(np.sort(perm), np.arange(n)):
            raise ValueError("VecchiaSolver: order must be a permutation of 0 .. {0}".format(n - 1))
        return perm.astype(np.int64)

    def compute(self, x, yerr):
        x, yerr, _ = self._check_inputs(x, yerr)
        n = len(x)
        self.failed_point = None
        perm = self._permutation(x)
        if perm is not None:
            x, yerr = np.ascontiguousarray(x[perm]), np.ascontiguousarray(yerr[perm])
        nbr = self._default_table(x) if self.neighbors is None else _check_neighbors(self.neighbors, n, self.m)
        logdet = C.c_double(0.0)
        self._perm, self._n = perm, n

        def run(h):
            rc = N.lib.gh_vecchia_compute(h, self._dk.handle, N.ptr(x), n, x.shape[1], N.ptr(yerr), N.ptr(nbr), C.byref(logdet))
            if rc == N.GH_ERR_NOT_PD:
                at = int(N.lib.gh_vecchia_info(h)) - 1
                self.failed_point = int(perm[at]) if perm is not None else at
            N.check(rc)

        self._retry_without_parked_memory(run)
        self._log_det = logdet.value
        self.computed = True

    # -- the solver protocol
    def _in(self, a):
        return a if self._perm is None else np.ascontiguousarray(a[self._perm])

    def _out(self, a):
        if self._perm is None:
            return a
        b = np.empty_like(a)
        b[self._perm] = a
        return b

    def apply_inverse(self, y, in_place=False):
        """``Q y`` for ``y`` of shape (n,) or (n, nrhs); ``in_place`` writes the values back into a writable array ``y``."""
        h = self._need()
        yc, nrhs = rhs_matrix(y, self._n)
        ys = self._in(yc)
        out = np.empty_like(ys)
        if nrhs > 0:
            N.check(N.lib.gh_vecchia_solve(h, N.ptr(ys), nrhs, N.ptr(out)))
        out = self._out(out)
        if in_place and isinstance(y, np.ndarray) and y.flags.writeable:
            try:
                y[...] = out
                return y
            except (ValueError, TypeError):
                pass
        return out

    def dot_solve(self, y):
        """``y^T Q y = sum_i e_i^2 / f_i``."""
        h = self._need()
        y = self._in(rhs_vector(y, self._n))
        out = C.c_double(0.0)
        N.check(N.lib.gh_vecchia_dot_solve(h, N.ptr(y), C.byref(out)))
        return out.value

    def apply_sqrt(self, r):
        raise NotImplementedError("apply_sqrt is not implemented for the VecchiaSolver")

    def get_inverse(self):
        """The precision ``Q`` as a dense matrix: ``apply_inverse`` of the identity.  O(N^2 m) time and N^2 memory: meant
        for small N."""
        self._need()
        return self.apply_inverse(np.eye(self._n))

    # -- device-resident GP glue
    def grad(self, r, which):
        """``BasicSolver.grad``'s ``(kgrad_full, alpha, diagA)`` for the Vecchia likelihood: the gradient over ALL kernel
        parameters (masked ones 0), ``alpha = Q r`` and ``diagA_j = 2 sum W_jj`` over the blocks that hold ``j``.  At
        ``m >= N - 1`` these are the dense values."""
        h = self._need()
        r = self._in(rhs_vector(r, self._n))
        which = np.ascontiguousarray(which, dtype=np.uint32)
        g = np.zeros(max(self._dk.size, 1))
        alpha, diagA = np.empty(self._n), np.empty(self._n)
        N.check(N.lib.gh_vecchia_grad(h, self._dk.handle, N.ptr(which), N.ptr(r), N.ptr(g), N.ptr(alpha), N.ptr(diagA)))
        return g[:self._dk.size], self._out(alpha), self._out(diagA)

    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """``K* Q r`` and (optionally) the diagonal or the whole of ``K** - K* Q K*^T``, in strips of test points.  The
        covariance keeps two N x M blocks and the M x M result on the device and raises ``MemoryError`` over its budget."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = self._in(rhs_vector(r, self._n)), N.as_f64(xs)
        want_var = bool(return_var)
        want_cov = bool(return_cov) and not want_var
        m = len(xs)
        mu = np.empty(m)
        var = np.empty(m) if want_var else None
        cov = np.empty((m, m)) if want_cov else None
        if m > 0:
            N.check(N.lib.gh_vecchia_predict(h, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(var), N.ptr(cov)))
        return mu, var, cov


atexit.register(VecchiaSolver.release_pool)
