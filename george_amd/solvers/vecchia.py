"""``VecchiaSolver`` -- the nearest-neighbour (Vecchia) approximation on one MI355X, for data sets no N x N factor fits:
10^5 - 10^6 points in any number of input dimensions.

The joint density is replaced by a product of conditionals, ``p(y) ~ prod_i p(y_i | y_c(i))``, where ``c(i)`` holds at most
``m`` points among the predecessors of ``i`` in a fixed order.  That is a proper Gaussian density with the sparse precision
``Q = (I - B)^T F^-1 (I - B)``: O(N m^3) flops, O(N m) memory, no probe vectors, no iteration counts.  With every predecessor
in the conditioning set (``m >= N - 1``) it is the dense likelihood up to rounding; smooth kernels with little noise need a
larger ``m`` than rough or noisy ones.  No reference counterpart.  The device side is ``george_amd/csrc/gh_vecchia.hip``.

Two predictors.  ``predict`` conditions every test point on all N data points through ``Q`` (the default, ``predict="global"``):
O(N M) kernel values, and a variance ``k** - K* Q K*^T`` that is only as good as ``Q`` -- it goes negative when ``m`` is too
small for the kernel.  ``predict_local`` (``predict="local"``) conditions each test point on its ``m`` nearest data points
alone: a proper conditional variance, O(M m^3) whatever N, no joint covariance between test points.

The neighbour search.  Both tables -- the predecessors of ``compute`` (:func:`vecchia_neighbors`) and the nearest data points
of local prediction (:func:`vecchia_query_neighbors`) -- are exact and come from the host by default (``search="host"``:
``scipy.spatial.cKDTree`` on one thread, which dominates ``predict_local`` at large M) or from the device
(``search="device"``, ``george_amd/csrc/gh_vecchia_search.hip``: a cell grid over the first three coordinates, one query per
wavefront).  For up to 7 input dimensions the two give the same table, near-ties included, and so the same bits everywhere; from
8 dimensions on NumPy adds the squared differences in another order than the device, and a device row is a nearest set under the
device's own distances (the two can differ where two distances agree to rounding).

The expected (Fisher) information of the hyper-parameters (``fisher_blocks``, behind ``GP.fisher_information`` and
``GP.parameter_covariance``): the likelihood is a product of Gaussian conditionals, so its information is a sum of one closed form
per point over the blocks the gradient already builds (Guinness 2021) -- one pass, no N x N array, about the cost of one
``grad``.  It is the information of THIS likelihood: the dense one when every predecessor is a neighbour, another quantity when not.

Leave-one-out cross-validation (``loo_blocks``, behind ``GP.loo_predict``, ``loo_log_likelihood``, ``grad_loo_log_likelihood``
and ``loo_nll_and_grad``): the density has the precision ``Q = sum_i u_i u_i^T / f_i``, so ``c = diag Q`` is a gather over the
columns of ``B``, ``alpha = Q r`` one application, and the values ``resid = alpha / c``, ``var = 1 / c`` and ``lpd`` cost O(N m);
the gradient is again a sum of one closed form per block over the blocks the likelihood gradient builds, about the cost of one
``grad``, with no N x N array.  It is the leave-one-out of THIS density, exact for it: the dense one when every predecessor is a
neighbour, and as far from the dense one as ``Q`` is from ``K^-1`` when not -- which is what makes the per-point residuals a
direct check of ``m``.

Not built: ordering strategies beyond the three of ``order=`` (max-min and the like: tried in NumPy, they moved the error of the
log-likelihood by a factor of about 2 at most), the observed information, ``apply_sqrt``, a joint covariance between the test
points of local prediction, and leave-group-out cross-validation (``GP.lgo_*`` takes the generic N x N branch here).
"""
import ctypes as C
import hashlib

import numpy as np

from .. import _native as N
from .protocol import HandlePool, NativeSolver, rhs_vector

__all__ = ["VecchiaSolver", "vecchia_neighbors", "vecchia_query_neighbors"]

M_MAX = 64


def _nearest_candidates(x, q, limit, cand, m):
    """For each query point ``q[i]`` the ``min(#, m)`` nearest of its candidates ``cand`` (len(q), k; entries >= limit[i] do
    not count) among the points ``x`` by squared Euclidean distance, ties to the lower index: ``(table (len(q), m) sorted
    ascending and padded with -1, the m-th smallest distance or inf)``.  ``limit[i] = i`` ranks predecessors, ``len(x)``
    every point."""
    n = len(x)
    valid = cand < limit[:, None]
    safe = np.where(valid, cand, 0)
    d2 = ((x[safe] - q[:, None, :]) ** 2).sum(axis=-1)
    d2 = np.where(valid, d2, np.inf)
    key = np.where(valid, cand, n)
    pick = np.lexsort((key, d2), axis=1)[:, :m]                     # by distance, then by index
    sel = np.take_along_axis(key, pick, axis=1)
    dm = np.take_along_axis(d2, pick, axis=1)
    if sel.shape[1] < m:
        sel = np.concatenate([sel, np.full((len(q), m - sel.shape[1]), n)], axis=1)
        dm = np.concatenate([dm, np.full((len(q), m - dm.shape[1]), np.inf)], axis=1)
    sel = np.sort(sel, axis=1)                                      # (the fill value n sorts last)
    return np.where(sel >= n, -1, sel).astype(np.int32), dm[:, m - 1]


def _certain(dm, dist, k, n):
    """Is the choice among the ``k`` points a tree query returned certain?  Every point the query left out is at least
    ``dist[:, -1]`` away: yes when the m-th chosen one (squared distance ``dm``) is nearer than that by more than the two
    routes' rounding, or when the query returned every point."""
    return (np.sqrt(dm) < dist[:, -1] * (1.0 - 1e-9)) if k < n else np.ones(len(dm), dtype=bool)


def _device_search(x, q, limit, m, device, occupancy=0):
    """``gh_vecchia_search``: the (len(q), m) table of the points ``x`` nearest to the queries ``q`` among those below
    ``limit`` (None: all)"""
    table = np.empty((len(q), m), dtype=np.int32)
    if m > M_MAX:
        raise ValueError("the device search takes 1 <= m <= {0}, not {1}".format(M_MAX, m))
    x, q = np.ascontiguousarray(x), np.ascontiguousarray(q)
    if limit is not None:
        limit = np.ascontiguousarray(limit, dtype=np.int64)
    N.check(N.lib.gh_vecchia_search(int(device), N.ptr(x), len(x), x.shape[1], N.ptr(q), len(q), N.ptr(limit), m, int(occupancy),
                                    N.ptr(table)))
    return table


def vecchia_neighbors(x, m, device=None):
    """The default conditioning sets: row ``i`` holds the ``min(i, m)`` nearest predecessors of point ``i`` under the
    Euclidean distance on ``x`` as given, ties going to the lower index, sorted ascending and padded with -1.  (N, m)
    int32.  The table depends on ``x`` only, so it stays fixed while an optimiser moves the hyper-parameters.

    Exact for every N: it equals the brute-force search.  Strictly increasing 1-D input takes the previous ``m`` points;
    everything else goes through ``scipy.spatial.cKDTree`` with a query size that grows until the ``m`` nearest
    predecessors are certain, and a direct search for the first rows.

    ``device``: ``None`` searches on the host as described; an integer runs the exact search on that device
    (``gh_vecchia_search`` with the limit ``i`` for row ``i``; m <= 64): the same table for up to 7 input dimensions, and
    from 8 on a nearest set under the device's own distances, which NumPy adds in another order.  No device: RuntimeError."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError("x must be (nsamples, ndim)")
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    n = len(x)
    if device is not None:
        return _device_search(x, x, np.arange(n, dtype=np.int64), m, device)
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
    table[:n0] = _nearest_candidates(x, x[rows], rows, np.broadcast_to(np.arange(n0)[None, :], (n0, n0)), m)[0]
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
            tab, dm = _nearest_candidates(x, x[rows], rows, cand, m)
            sure = _certain(dm, dist, k, n)
            table[rows[sure]] = tab[sure]
            again.append(rows[~sure])
        todo, k = np.concatenate(again), min(n, 2 * k)
    return table


# The tree of a data set is built once and kept, keyed by a digest of the inputs, the way VecchiaSolver._TABLES keeps tables.
_TREES = []
_TREES_MAX = 2


def _tree(x):
    key = (x.shape, hashlib.blake2b(memoryview(np.ascontiguousarray(x)).cast("B"), digest_size=16).digest())
    for k, tree in _TREES:
        if k == key:
            return tree
    from scipy.spatial import cKDTree
    tree = cKDTree(x)
    _TREES.append((key, tree))
    del _TREES[:-_TREES_MAX]
    return tree


def vecchia_query_neighbors(x, t, m, device=None):
    """The conditioning sets of local prediction: row ``c`` holds the ``min(N, m)`` data points ``x`` nearest to the test
    point ``t[c]`` under the Euclidean distance on the inputs as given, ties going to the lower index, sorted ascending and
    padded with -1.  (M, m) int32.

    Exact for every input: it equals the brute-force search.  Strictly increasing 1-D ``x`` goes through ``searchsorted``
    and a window of ``2 m`` points around the test point; everything else goes through ``scipy.spatial.cKDTree`` (built
    once per data set and kept) with a query size that grows until the ``m`` nearest points are certain, and a direct
    search when N is small.  The search runs on the host, O(M m log N): for large M it takes longer than the device call
    it feeds.

    ``device``: ``None`` searches on the host as described; an integer runs the exact search on that device
    (``gh_vecchia_search``; m <= 64): the same table for up to 7 input dimensions, and from 8 on a nearest set under the
    device's own distances, which NumPy adds in another order.  No device: RuntimeError."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if t.ndim == 1:
        t = t[:, None]
    if x.ndim != 2 or t.ndim != 2 or x.shape[1] != t.shape[1]:
        raise ValueError("x must be (nsamples, ndim) and t (ntest, ndim)")
    m = int(m)
    if m < 1:
        raise ValueError("m must be at least 1")
    n, nt = len(x), len(t)
    if device is not None:
        return _device_search(x, t, None, m, device)
    table = np.full((nt, m), -1, dtype=np.int32)
    if n == 0 or nt == 0:
        return table
    limit = np.full(nt, n)
    if x.shape[1] == 1 and np.all(np.diff(x[:, 0]) > 0):
        # the m nearest points of a sorted line are consecutive and lie among the m before and the m after the test point
        step = max(1, (1 << 22) // (2 * m))
        for s in range(0, nt, step):
            rows = slice(s, s + step)
            cand = np.searchsorted(x[:, 0], t[rows, 0])[:, None] + np.arange(-m, m)[None, :]
            cand = np.where((cand >= 0) & (cand < n), cand, n)
            table[rows] = _nearest_candidates(x, t[rows], limit[rows], cand, m)[0]
        return table
    if n <= 4 * m + 64:                                                     # directly: every point is a candidate
        step = max(1, (1 << 22) // (n * x.shape[1]))
        for s in range(0, nt, step):
            rows = slice(s, s + step)
            table[rows] = _nearest_candidates(x, t[rows], limit[rows], np.broadcast_to(np.arange(n)[None, :], (len(t[rows]), n)), m)[0]
        return table
    tree = _tree(x)
    todo, k = np.arange(nt), min(n, m + 1)
    while len(todo):
        again = []
        step = max(1, (1 << 22) // (k * x.shape[1]))                        # rows per query: the candidates' coordinates in 32 MB
        for s in range(0, len(todo), step):
            rows = todo[s:s + step]
            dist, cand = tree.query(t[rows], k=k)
            if k == 1:
                dist, cand = dist[:, None], cand[:, None]
            tab, dm = _nearest_candidates(x, t[rows], limit[rows], cand, m)
            sure = _certain(dm, dist, k, n)
            table[rows[sure]] = tab[sure]
            again.append(rows[~sure])
        todo, k = np.concatenate(again), min(n, 2 * k)
    return table


def _check_query_neighbors(nbr, nt, m, n):
    """the (nt, m) query table as contiguous int32: every entry is -1 or in [0, n), none twice in a row"""
    nbr = np.asarray(nbr)
    if nbr.shape != (nt, m) or nbr.dtype.kind not in "iu":
        raise ValueError("neighbors must be an integer table of shape ({0}, {1})".format(nt, m))
    if np.any(nbr < -1) or np.any(nbr >= n):
        raise ValueError("neighbors: every entry must be -1 or one of the data points 0 .. {0}".format(n - 1))
    s = np.sort(nbr, axis=1)
    if np.any((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0)):
        raise ValueError("neighbors: an entry appears twice in a row")
    return np.ascontiguousarray(nbr, dtype=np.int32)


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
    """``VecchiaSolver(kernel, m=32, order=None, neighbors=None, device=0, predict="global", search="host")``.

    ``m``: neighbours per point, 1 .. 64.  ``order``: ``None`` (the caller's order), ``"coordinate"`` (a stable argsort of
    the first input column) or a permutation array (solver position -> caller's index); the solver permutes its inputs on
    the way in and un-permutes ``alpha``, ``diagA`` and solve results on the way out.  ``neighbors``: ``None``
    (:func:`vecchia_neighbors` of the ordered inputs) or an (N, m) integer table IN SOLVER ORDER, padded with -1; entries
    need not be sorted.  ``predict``: what :meth:`predict` -- and with it ``GP.predict`` -- computes: ``"global"``, every
    test point conditioned on all data points through ``Q``, or ``"local"``, :meth:`predict_local`.  ``search``: where the
    default tables of ``compute`` and of ``predict_local`` are made, ``"host"`` or ``"device"`` (the same tables for up to 7
    input dimensions; see the module's text)."""

    _CREATE, _DESTROY = "gh_vecchia_create", "gh_vecchia_destroy"
    _SOLVE, _DOT_SOLVE = "gh_vecchia_solve", "gh_vecchia_dot_solve"     # Q y and y^T Q y = sum_i e_i^2 / f_i; no get_inverse, no apply_sqrt

    def __init__(self, kernel, m=32, order=None, neighbors=None, device=0, predict="global", search="host"):
        m = int(m)
        if m < 1 or m > M_MAX:
            raise ValueError("VecchiaSolver: 1 <= m <= {0}, not {1}".format(M_MAX, m))
        if isinstance(order, str) and order != "coordinate":
            raise ValueError("VecchiaSolver: order is None, 'coordinate' or a permutation")
        if predict not in ("global", "local"):
            raise ValueError("VecchiaSolver: predict is 'global' or 'local'")
        if search not in ("host", "device"):
            raise ValueError("VecchiaSolver: search is 'host' or 'device'")
        self.m = m
        self.order = order
        self.neighbors = neighbors
        self.predict_mode = predict
        self.search = search
        self.failed_point = None
        self.failed_test_point = None
        self._opts = dict(device=int(device))
        self._perm = None
        self._xo = None                                     # the ordered host inputs of compute(): what predict_local searches
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
        tab = vecchia_neighbors(x, self.m, device=self._opts["device"] if self.search == "device" else None)
        VecchiaSolver._TABLES.append((key, tab))
        del VecchiaSolver._TABLES[:-VecchiaSolver._TABLES_MAX]
        return tab

    # -- lifetime.  GP makes a new solver for every compute: the handle of a dropped solver (its neighbour table checked, indexed
    # and on the device) is parked, at most _HPOOL_MAX per (device, m), and picked up by the next solver with the same options.
    _HPOOL_MAX = 2
    _HPOOL = HandlePool(_DESTROY, _HPOOL_MAX)
    _GIVES_BACK_POOLS = (_HPOOL,)                           # out of memory: own handle, own pool and the native caches

    def _options_key(self):
        return (self._opts["device"], self.m)

    def _native_opts(self):
        o = N.gh_vecchia_opts()
        o.device, o.m = self._options_key()
        return o

    def __getstate__(self):
        state = super(VecchiaSolver, self).__getstate__()
        state["_perm"] = None
        state["_xo"] = None
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
        self.failed_point = self.failed_test_point = None
        perm = self._permutation(x)
        if perm is not None:
            x, yerr = np.ascontiguousarray(x[perm]), np.ascontiguousarray(yerr[perm])
        nbr = self._default_table(x) if self.neighbors is None else _check_neighbors(self.neighbors, n, self.m)
        logdet = C.c_double(0.0)
        self._perm, self._n, self._xo = perm, n, x

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

    def _solve_target(self, y, yc, in_place):
        """``in_place``: the values are copied back into any writable array ``y``, whatever its dtype"""
        return np.empty_like(yc), (y if in_place and isinstance(y, np.ndarray) and y.flags.writeable else None)

    # -- device-resident GP glue
    def grad(self, r, which):
        """``BasicSolver.grad``'s ``(kgrad_full, alpha, diagA)`` for the Vecchia likelihood: the gradient over ALL kernel
        parameters (masked ones 0), ``alpha = Q r`` and ``diagA_j = 2 sum W_jj`` over the blocks that hold ``j``.  At
        ``m >= N - 1`` these are the dense values."""
        return self._grad("gh_vecchia_grad", r, which)

    def fisher_blocks(self, which=None, diag_rows=None):
        """Expected (Fisher) information of the Vecchia likelihood (gh_vecchia_fisher; Guinness 2021), the contract of
        ``BasicSolver.fisher``: ``(n_diag + size, n_diag + size)`` over the ``n_diag`` diagonal derivative matrices
        ``diag(diag_rows[p])`` (in the caller's point order) followed by ALL kernel parameters (those masked out by ``which``
        have rows and columns of exactly 0; ``which=None``: all of them).  A sum of one closed form per block, about the cost
        of one :meth:`grad`, with no N x N array anywhere.  At ``m >= N - 1`` it is the dense ``1/2 tr(K^-1 D_a K^-1 D_b)``;
        for smaller ``m`` it is the information of the approximate likelihood, not an approximation of known quality to the
        dense one -- hence a name of its own: ``fisher`` stays the dense call, which only ``BasicSolver`` offers, and ``GP``
        takes this one where a solver has no ``fisher``.  At most 64 planes -- ``n_diag`` plus the unmasked kernel parameters -- else ``ValueError``."""
        self._need()
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
            if self._perm is not None:
                rows = np.ascontiguousarray(rows[:, self._perm])
        p = n_diag + size
        out = np.zeros((p, p))
        if p == 0:
            return out
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_vecchia_fisher(
            hh, self._dk.handle, N.ptr(wh), N.ptr(rows) if n_diag else None, n_diag, N.ptr(out))))
        return out

    def loo_blocks(self, r, which=None):
        """Leave-one-out cross-validation of the Vecchia density for residual ``r = y - mean`` (gh_vecchia_loo), the contract of
        ``BasicSolver.loo``: ``(lpd_sum, resid, var, lpd, grad_full | None, v | None, diagB | None)`` with ``resid = y - mu_loo``,
        ``var`` the leave-one-out variances, ``lpd`` the N log predictive densities and ``lpd_sum`` their sum, all from
        ``c = diag Q`` and ``alpha = Q r``.  ``which=None``: values only, O(N m).  With a parameter mask also ``grad_full`` =
        d lpd_sum / d theta over ALL kernel parameters (masked ones exactly 0), ``v`` = d lpd_sum / d mean_i and ``diagB`` =
        d lpd_sum / d K_ii: a sum of one closed form per block, about the cost of one :meth:`grad`, with no N x N array anywhere.
        The N-vectors are in the caller's point order.  It is the leave-one-out of THIS density, exact for it: the dense one at
        ``m >= N - 1``, and as far from it as ``Q`` is from ``K^-1`` otherwise -- hence a name of its own: ``loo`` stays the
        dense call, which only ``BasicSolver`` offers, and ``GP`` takes this one where a solver has no ``loo``."""
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
        self._retry_without_parked_memory(lambda hh: N.check(N.lib.gh_vecchia_loo(
            hh, self._dk.handle, N.ptr(wh), N.ptr(r), C.byref(total), N.ptr(resid), N.ptr(var), N.ptr(lpd),
            N.ptr(g), N.ptr(v), N.ptr(diagB))))
        if which is None:
            return total.value, self._out(resid), self._out(var), self._out(lpd), None, None, None
        return total.value, self._out(resid), self._out(var), self._out(lpd), g[:size], self._out(v), self._out(diagB)

    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """``K* Q r`` and (optionally) the diagonal or the whole of ``K** - K* Q K*^T``, in strips of test points.  The
        covariance keeps two N x M blocks and the M x M result on the device and raises ``MemoryError`` over its budget.

        With ``predict="local"`` this is :meth:`predict_local` with its defaults; a covariance is then a ``ValueError``
        (and so is ``GP.sample_conditional``, which asks for one)."""
        if self.predict_mode == "local":
            if return_cov and not return_var:
                raise ValueError("VecchiaSolver(predict='local') has no covariance between test points: they are conditionally "
                                 "independent given their neighbours; ask for return_var=True or return_cov=False")
            mu, var = self.predict_local(kernel, r, xs, return_var=return_var)
            return mu, var, None
        return self._predict("gh_vecchia_predict", kernel, r, xs, return_var, return_cov)

    def predict_local(self, kernel, r, xs, return_var=False, neighbors=None, m=None, search=None):
        """Nearest-neighbour prediction: test point ``c`` conditioned on the data points of row ``c`` of ``neighbors`` alone,
        ``mu = k_c^T (K_cc + yerr^2)^-1 r_c`` and ``var = k** - k_c^T (K_cc + yerr^2)^-1 k_c``.  Returns ``(mu, var | None)``.

        ``var`` is a proper conditional variance: positive, never below the dense one, never above ``k**``.  One Cholesky of at
        most ``m x m`` per test point, O(M m^3) whatever N.  ``K_cc`` comes from the solver's kernel as of ``compute``, ``k_c``
        and ``k**`` from ``kernel`` (a component of it, for instance).  ``m``: 1 .. 64, the solver's by default.
        ``neighbors``: ``None`` (:func:`vecchia_query_neighbors` of the solver's ordered inputs, a host search that dominates
        the call at large M) or an (M, m) integer table in the CALLER's point numbering, padded with -1 anywhere, entries in
        any order; a row without entries gives ``mu = 0``, ``var = k**``.  A block that is not positive definite raises
        ``numpy.linalg.LinAlgError`` with ``failed_test_point`` set; the solver stays computed.

        ``search``: ``"host"``, ``"device"`` or ``None`` (the solver's setting), where the table of ``neighbors=None`` is
        made.  ``"device"`` is one call: the search runs over the solver's points on the device (their grid is built at the
        first call after a ``compute`` on other points) and its table never leaves it.  An explicit ``neighbors`` ignores it."""
        search = self.search if search is None else search
        if search not in ("host", "device"):
            raise ValueError("predict_local: search is 'host' or 'device'")
        m = self.m if m is None else int(m)
        if m < 1 or m > M_MAX:
            raise ValueError("predict_local: 1 <= m <= {0}, not {1}".format(M_MAX, m))
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = self._in(rhs_vector(r, self._n)), N.as_f64(xs)
        if xs.ndim == 1:
            xs = xs[:, None]
        if xs.ndim != 2 or xs.shape[1] != self._xo.shape[1]:
            raise ValueError("xs must be (ntest, {0})".format(self._xo.shape[1]))
        nt = len(xs)
        fused = neighbors is None and search == "device"
        if fused:
            nbr = None
        elif neighbors is None:
            nbr = vecchia_query_neighbors(self._xo, xs, m)
        else:
            nbr = _check_query_neighbors(neighbors, nt, m, self._n)
            if self._perm is not None:                      # caller's index -> solver position
                inv = np.empty(self._n, dtype=np.int32)
                inv[self._perm] = np.arange(self._n, dtype=np.int32)
                nbr = np.ascontiguousarray(np.where(nbr >= 0, inv[nbr], -1), dtype=np.int32)
        self.failed_test_point = None
        mu = np.empty(nt)
        var = np.empty(nt) if return_var else None
        if nt > 0:
            if fused:
                rc = N.lib.gh_vecchia_predict_local_search(h, self._dk.handle, dk.handle, N.ptr(r), N.ptr(xs), nt, m, 0, N.ptr(mu), N.ptr(var), None)
            else:
                rc = N.lib.gh_vecchia_predict_local(h, self._dk.handle, dk.handle, N.ptr(r), N.ptr(xs), nt, N.ptr(nbr), m, N.ptr(mu), N.ptr(var))
            if rc == N.GH_ERR_NOT_PD:
                self.failed_test_point = int(N.lib.gh_vecchia_info(h)) - 1
            N.check(rc)
        return mu, var

