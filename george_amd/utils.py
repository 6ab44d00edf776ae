"""Small host-side helpers (sampling, sorting, finite differences) with the
signatures of the reference's ``src/george/utils.py:11-92``.  Not on the hot path."""
import numpy as np

__all__ = ["multivariate_gaussian_samples", "pivoted_cholesky", "nd_sort_samples", "numerical_gradient", "check_gradient"]


def multivariate_gaussian_samples(matrix, N, mean=None):
    """Draw ``N`` samples from N(mean, matrix); one sample is returned 1-D."""
    mean = np.zeros(len(matrix)) if mean is None else mean
    draws = np.random.multivariate_normal(mean, matrix, N)
    return draws[0] if N == 1 else draws


def pivoted_cholesky(a, tol=None):
    """Diagonally pivoted Cholesky with rank truncation of the symmetric matrix ``a`` (LAPACK ``dpstrf``'s job), without
    row or column swaps: returns ``(L, piv, rank)`` with ``L @ L.T`` approximating ``a`` directly -- every entry within
    ``tol`` in exact arithmetic -- ``L[:, rank:] == 0`` exactly, ``L`` lower triangular in pivot order
    (``L[piv[i], j] == 0`` for ``i < j``) and ``piv[:rank]`` the pivots in the order they were taken (``-1`` behind them).
    ``tol`` is the absolute stop threshold on the remaining diagonal; ``None`` or a negative value mean
    ``m * eps * max(diag(a).max(), 0)``.  A non-finite diagonal gives ``rank = -1`` and NaN in ``L``.  This is, line for
    line, the definition the device kernel implements (``gh_dev_pstrf``, george_amd/csrc/gh_pstrf.hip): the NumPy branch
    of ``GP.sample*(factor="cholesky")`` and the restatement the tests hold the device against."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError("pivoted_cholesky: a square matrix is needed")
    m = a.shape[0]
    L = np.zeros((m, m))
    piv = np.full(m, -1, dtype=np.int64)
    d = np.array(np.diagonal(a), dtype=np.float64)
    if not np.all(np.isfinite(d)):
        L[:] = np.nan
        return L, piv, -1
    if tol is None or tol < 0:
        tol = m * np.finfo(np.float64).eps * max(d.max(), 0.0)
    free = np.ones(m, dtype=bool)
    rank = 0
    for j in range(m):
        p = int(np.argmax(np.where(free, d, -np.inf)))          # (the first of equal entries: the lowest index)
        if not free[p] or not d[p] > tol:
            break
        c = a[:, p] - L[:, :j] @ L[p, :j]                       # the pivot column, updated
        if not (c[p] > 0 and np.isfinite(c[p])):
            break
        c[~free] = 0.0
        s = np.sqrt(c[p])
        L[:, j] = c / s
        L[p, j] = s
        d -= L[:, j] ** 2
        free[p] = False
        piv[j] = p
        rank = j + 1
    return L, piv, rank


def nd_sort_samples(samples):
    """Indices ordering N-dimensional points by distance from the first one (KD-tree
    query, as the reference does), which keeps HODLR off-diagonal blocks low rank."""
    from scipy.spatial import cKDTree
    samples = np.asarray(samples)
    assert samples.ndim == 2
    _, order = cKDTree(samples).query(samples[0], k=len(samples))
    return np.atleast_1d(order)


def numerical_gradient(f, x, dx=1.234e-6):
    x = np.array(x, dtype=np.float64)
    g = np.empty_like(x)
    for i in range(len(x)):
        x[i] += dx
        fp = f(x)
        x[i] -= 2 * dx
        fm = f(x)
        x[i] += dx
        g[i] = 0.5 * (fp - fm) / dx
    return g


def check_gradient(obj, *args, **kwargs):
    eps = kwargs.pop("eps", 1.23e-5)
    g0 = obj.get_gradient(*args, **kwargs)
    theta = obj.get_parameter_vector()
    for i, t in enumerate(theta):
        theta[i] = t + eps
        obj.set_parameter_vector(theta)
        fp = obj.get_value(*args, **kwargs)
        theta[i] = t - eps
        obj.set_parameter_vector(theta)
        fm = obj.get_value(*args, **kwargs)
        theta[i] = t
        obj.set_parameter_vector(theta)
        assert np.allclose(0.5 * (fp - fm) / eps, g0[i])
