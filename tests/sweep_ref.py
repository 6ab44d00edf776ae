"""CPU reference for the solve-side sweeps of the dense solver (``apply_inverse``, ``get_inverse``, ``apply_sqrt``,
``predict``), the test problems that reach the edges of ``trsm_multi`` and the criteria an answer is held to.  NumPy and
SciPy only; no device.  ``tests/test_sweep_reference.py`` shows on the CPU that SciPy's answers meet every criterion with
room to spare and that subtly wrong answers do not; ``tests/test_gpu_sweeps.py`` applies the same criteria to the device.

Criteria (``u = 2^-53``, ``n`` points, ``kappa = |K|_inf |K^-1|_inf``):

* backward error of a solve, per checked column: ``|b_j - K x_j|_inf / (|K|_inf |x_j|_inf + |b_j|_inf) <= n u``, the residual
  formed in ``np.longdouble``.  ``n u`` is the first-order constant of one length-n inner product, which every entry of
  these sweeps is.
* forward error against SciPy, every entry: ``forward_bound(kappa, n, scale) = 2 kappa n u scale`` -- two answers whose
  backward errors are each at most ``n u`` differ by at most that, to first order.  ``scale`` is the largest entry of the
  reference for a solve and the largest sum of the magnitudes of the terms for a product.
* right residual of the inverse, per checked column: ``|e_j - K x_j|_inf <= kappa n u`` (an inverse formed as
  ``L^-T L^-1`` has a right residual proportional to kappa: Higham, Accuracy and Stability of Numerical Algorithms,
  chapter 14).
* exact properties: the inverse is symmetric bit for bit, ``e_i @ U`` is exactly zero left of column ``i``.

A longdouble product has no BLAS, so residuals are formed on ``checked_cols`` only: the first and the last column, both
sides of every 128-column border and four seeded random ones -- every 128-column tile has at least two.

Every criterion comes back as a ``Check(name, value, bound, where)``; ``where`` names the 128 x 128 tile (tile row, tile
column) of the worst entry, which tells a far update from a clipped range from a diagonal step.
Test helper only: not a conftest.
"""
import collections
import functools

import numpy as np
from scipy.linalg import cho_solve, cholesky

from oracle import kernels_np

# the residuals below are only worth something in a format well past double: fail loudly where longdouble is double
assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no extended format here: eps = %g" % np.finfo(np.longdouble).eps

U = 2.0 ** -53
T = 128                  # rows of a tile
SB = 8                   # tiles of a super-block of trsm_multi
# N: np, tiles.  128: one tile.  1024: exactly one super-block.  1152: one super-block and a tile (far updates with
# M = 128).  1300: 1408, 11, ragged and a partial super-block.  2100: 2176, 17, two super-blocks and a tile, ragged.
# 8400: 8448, 66, the chain's dist > 64 and predict's column reduction in 64 chunks of 132 rows.
SIZES = (128, 1024, 1152, 1300, 2100, 8400)
KINDS = ("m32", "expsq")


def kind_of(n):
    """the kernel of size ``n``: the two kinds in turn over SIZES"""
    return KINDS[SIZES.index(n) % 2]


class Check(collections.namedtuple("Check", "name value bound where")):
    """One criterion: it holds when ``value <= bound``.  ``where``: the worst entry's place, for the failure message."""

    @property
    def ratio(self):
        if self.bound > 0.0:
            return float(self.value) / float(self.bound)
        return np.inf if self.value > 0.0 else 0.0


def forward_bound(kappa, n, scale):
    return 2.0 * kappa * n * U * scale


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


Problem = collections.namedtuple("Problem", "n kind kernel x yerr K L Kinv kappa normK")


@functools.lru_cache(maxsize=None)
def problem(n, kind):
    """One test problem, computed once and read-only: ``n`` sorted points uniform on [0, n / 20] (a constant density keeps
    the condition number flat as n grows), error bars uniform in [0.8, 1.2], ``K`` with ``yerr^2`` on the diagonal, SciPy's
    lower factor ``L``, ``Kinv = cho_solve(L, I)`` and ``kappa = |K|_inf |Kinv|_inf``."""
    from george_amd import kernels
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0.0, n / 20.0, n))[:, None]
    yerr = rng.uniform(0.8, 1.2, n)
    kernel = 1.5 * {"m32": kernels.Matern32Kernel, "expsq": kernels.ExpSquaredKernel}[kind](1.0)
    K = np.array(kernels_np.value_symmetric(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    L = cholesky(K, lower=True)
    Kinv = cho_solve((L, True), np.eye(n))
    normK = float(np.max(np.sum(np.abs(K), axis=1)))
    kappa = normK * float(np.max(np.sum(np.abs(Kinv), axis=1)))
    _freeze(x, yerr, K, L, Kinv)
    return Problem(n, kind, kernel, x, yerr, K, L, Kinv, kappa, normK)


def checked_cols(ncols, seed=0):
    """The columns residuals are formed on: first, last, both sides of every 128-column border, four seeded random ones."""
    cols = {0, ncols - 1}
    for b in range(T, ncols, T):
        cols.update((b - 1, b))
    cols.update(int(c) for c in np.random.RandomState(7919 * ncols + seed).randint(0, ncols, 4))
    return np.array(sorted(cols))


def _2d(a):
    a = np.asarray(a)
    return a.reshape(len(a), -1)


def residual(K, X, B, cols, block=256):
    """``B[:, cols] - K @ X[:, cols]`` in ``np.longdouble``, ``K`` converted a block of rows at a time"""
    X, B = _2d(X), _2d(B)
    Xl = X[:, cols].astype(np.longdouble)
    R = np.empty((len(K), len(cols)), dtype=np.longdouble)
    for r0 in range(0, len(K), block):
        r1 = min(r0 + block, len(K))
        R[r0:r1] = B[r0:r1][:, cols].astype(np.longdouble) - np.dot(K[r0:r1].astype(np.longdouble), Xl)
    return R


def residual_eta(K, X, B, cols):
    """per checked column, the normwise backward error ``|b_j - K x_j|_inf / (|K|_inf |x_j|_inf + |b_j|_inf)``"""
    return _eta(K, X, B, cols)[0]


def _eta(K, X, B, cols):
    X, B = _2d(X), _2d(B)
    R = np.abs(residual(K, X, B, cols))
    normK = np.max(np.sum(np.abs(K), axis=1))
    with np.errstate(invalid="ignore"):
        eta = (np.max(R, axis=0) / (normK * np.max(np.abs(X[:, cols]), axis=0) + np.max(np.abs(B[:, cols]), axis=0))).astype(np.float64)
    eta[~np.isfinite(eta)] = np.inf
    return eta, _where_cols(R, cols)


def _where_cols(R, cols):
    """the place of the largest entry of ``R``, whose columns are the columns ``cols`` of the full array"""
    R = np.where(np.isfinite(R), R, np.inf)
    i, k = np.unravel_index(int(np.argmax(R)), R.shape)
    return "tile row %d, tile column %d (entry %d, %d)" % (i // T, cols[k] // T, i, cols[k])


def worst_tile(err):
    """the place of the largest entry of ``err`` (NaN counts as largest)"""
    err = _2d(np.where(np.isfinite(err), np.abs(err), np.inf))
    i, j = np.unravel_index(int(np.argmax(err)), err.shape)
    return "tile row %d, tile column %d (entry %d, %d)" % (i // T, j // T, i, j)


def _forward(name, got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return Check(name, np.inf, bound, "shape %r, not %r" % (got.shape, want.shape))
    if got.size == 0:
        return Check(name, 0.0, bound, "empty")
    err = np.where(np.isfinite(got), np.abs(got - want), np.inf)
    return Check(name, float(np.max(err)), bound, worst_tile(err))


# ---------------------------------------------------------------- apply_inverse
SolveCase = collections.namedtuple("SolveCase", "p B X cols")


@functools.lru_cache(maxsize=None)
def solve_case(n, nrhs):
    """a random right-hand side ((n,) for nrhs = 1, else (n, nrhs)), SciPy's solution and the checked columns"""
    p = problem(n, kind_of(n))
    B = np.random.RandomState(1000 * n + nrhs).randn(n, nrhs)
    if nrhs == 1:
        B = B[:, 0].copy()
    X = cho_solve((p.L, True), B)
    _freeze(B, X)
    return SolveCase(p, B, X, checked_cols(nrhs))


def check_solve(case, X):
    p = case.p
    if np.shape(X) != case.X.shape:
        return [Check("shape", np.inf, 0.0, "shape %r, not %r" % (np.shape(X), case.X.shape))]
    eta, where = _eta(p.K, X, case.B, case.cols)
    return [Check("eta", float(np.max(eta)), p.n * U, where),
            _forward("forward", X, case.X, forward_bound(p.kappa, p.n, np.max(np.abs(case.X))))]


# ---------------------------------------------------------------- get_inverse
def check_inverse(p, X):
    X = np.asarray(X)
    if X.shape != p.Kinv.shape:
        return [Check("shape", np.inf, 0.0, "shape %r, not %r" % (X.shape, p.Kinv.shape))]
    cols = checked_cols(p.n)
    R = np.abs(residual(p.K, X, np.eye(p.n), cols))
    R = np.where(np.isfinite(R), R, np.inf)
    asym = np.where(X == X.T, 0.0, 1.0)
    return [_forward("forward", X, p.Kinv, forward_bound(p.kappa, p.n, np.max(np.abs(p.Kinv)))),
            Check("right residual", float(np.max(R)), p.kappa * p.n * U, _where_cols(R, cols)),
            Check("asymmetric entries", float(np.sum(asym)), 0.0, worst_tile(asym))]


# ---------------------------------------------------------------- apply_sqrt
SqrtCase = collections.namedtuple("SqrtCase", "p r out scale")
UNIT_ROWS = (0, 127, 128, 1023, 1024, -1)


@functools.lru_cache(maxsize=None)
def sqrt_case(n, nrows):
    """random rows ``r`` (nrows, n), ``r @ L^T`` and the largest sum of the magnitudes of the terms of one entry"""
    p = problem(n, kind_of(n))
    r = np.random.RandomState(2000 * n + nrows).randn(nrows, n)
    out = np.dot(r, p.L.T)
    scale = float(np.max(np.dot(np.abs(r), np.abs(p.L).T)))
    _freeze(r, out)
    return SqrtCase(p, r, out, scale)


def check_sqrt(case, out):
    return [_forward("forward", out, case.out, forward_bound(case.p.kappa, case.p.n, case.scale))]


def unit_rows(n):
    """the indices ``i`` of the unit rows ``e_i``: both sides of the first tile border and of the first super-block border,
    the first and the last row -- those that exist"""
    return sorted({i % n for i in UNIT_ROWS if -n <= i < n})


def check_sqrt_units(p, idx, rows):
    """``rows[k] = e_idx[k] @ U``: exactly zero left of column ``idx[k]`` (the K range of the product ends at the diagonal),
    and right of it column ``idx[k]`` of a factor of ``K`` -- compared with SciPy's under the forward bound."""
    rows = np.asarray(rows)
    left = np.zeros(rows.shape)
    for k, i in enumerate(idx):
        left[k, :i] = np.where(rows[k, :i] == 0.0, 0.0, 1.0)
    scale = float(np.max(np.abs(p.L)))
    return [Check("non-zeros left of the diagonal", float(np.sum(left)), 0.0, worst_tile(left)),
            _forward("forward", rows, p.L[:, idx].T, forward_bound(p.kappa, p.n, scale))]


def check_sqrt_gram(p, G, idx):
    """``G = I @ U``, all the unit rows at once: row ``k`` is ``e_k @ U``, so ``G`` is ``U`` itself.  Exactly zero below the
    diagonal, and its COLUMNS reproduce ``K``: ``K_ij = sum_k U_ki U_kj`` within ``n u |U_:i| |U_:j|`` for i, j in ``idx``
    (the backward error of a Cholesky factor, ``|K - U^T U| <= gamma_(n+1) |U^T| |U|``, with Cauchy-Schwarz on the right),
    the sums formed in longdouble."""
    G = np.asarray(G)
    low = np.where(np.tril(G, -1) == 0.0, 0.0, 1.0)
    C = G[:, idx].astype(np.longdouble)
    gram = np.dot(C.T, C)
    norms = np.sqrt(np.diag(gram))
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = (np.abs(gram - p.K[np.ix_(idx, idx)]) / np.outer(norms, norms)).astype(np.float64)
    rel[~np.isfinite(rel)] = np.inf
    a, b = np.unravel_index(int(np.argmax(rel)), rel.shape)
    return [Check("non-zeros below the diagonal", float(np.sum(low)), 0.0, worst_tile(low)),
            Check("gram", float(np.max(rel)), p.n * U, "K[%d, %d]: tile row %d, tile column %d" % (idx[a], idx[b], idx[a] // T, idx[b] // T))]


# ---------------------------------------------------------------- predict
PredictCase = collections.namedtuple("PredictCase", "p y xs mu var cov scale_mu scale_cov")


@functools.lru_cache(maxsize=None)
def predict_case(n, m):
    """``m`` test points uniform over the span of ``x``, a random residual ``y`` and the float64 definitions through SciPy:
    ``mu = K* alpha``, ``cov = K** - K* K^-1 K*^T``, ``var = diag(cov)``, with the magnitudes of the terms summed as scales"""
    p = problem(n, kind_of(n))
    rng = np.random.RandomState(3000 * n + m)
    y = rng.randn(n)
    xs = rng.uniform(p.x[0, 0], p.x[-1, 0], m)[:, None]
    Ks = np.array(kernels_np.value_general(p.kernel, xs, p.x), dtype=np.float64)
    Kss = np.array(kernels_np.value_general(p.kernel, xs, xs), dtype=np.float64)
    alpha = cho_solve((p.L, True), y)
    W = cho_solve((p.L, True), Ks.T)
    mu = np.dot(Ks, alpha)
    cov = Kss - np.dot(Ks, W)
    var = np.diag(Kss) - np.sum(Ks * W.T, axis=1)
    scale_mu = float(np.max(np.dot(np.abs(Ks), np.abs(alpha))))
    scale_cov = float(np.max(Kss) + np.max(np.sum(np.abs(Ks) * np.abs(W.T), axis=1)))
    _freeze(y, xs, mu, var, cov)
    return PredictCase(p, y, xs, mu, var, cov, scale_mu, scale_cov)


def check_predict(case, mu, var, cov):
    p = case.p
    bound = forward_bound(p.kappa, p.n, case.scale_cov)
    return [_forward("mu", mu, case.mu, forward_bound(p.kappa, p.n, case.scale_mu)),
            _forward("var", var, case.var, bound),
            _forward("cov", cov, case.cov, bound),
            _forward("var against diag(cov)", var, np.diag(np.asarray(cov)), bound)]
