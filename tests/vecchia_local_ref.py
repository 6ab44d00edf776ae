"""NumPy restatement of local (nearest-neighbour) prediction (``VecchiaSolver.predict_local``, ``vecchia_local_kernel`` of
george_amd/csrc/gh_vecchia.hip): a plain loop over test points.

For test point ``t`` with the data points ``c`` of its row of the table, ``K`` the data kernel plus ``yerr^2`` on its diagonal:

    mu = k_c^T K_cc^-1 r_c,     var = k** - k_c^T K_cc^-1 k_c,     k_c = k_cross(x_c, t),   k** = k_cross(t, t)

and ``mu = 0``, ``var = k**`` for an empty row.  Kernel values come from ``oracle.solver_np``, the data point as the first
argument (``K_cc`` on the index-sorted set: the lower index first); block solves are SciPy ``cho_factor`` / ``cho_solve``.
``query_neighbors`` is the brute-force search the library's ``vecchia_query_neighbors`` must equal.  Test helper only: not a
conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import solver_np

import vecchia_ref


def _as_2d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def query_neighbors(x, t, m):
    """row c: the min(N, m) data points nearest to t[c] (squared Euclidean distance, ties to the lower index), ascending, padded -1"""
    x, t = _as_2d(x), _as_2d(t)
    out = np.full((len(t), m), -1, dtype=np.int32)
    for c in range(len(t)):
        d2 = ((x - t[c]) ** 2).sum(axis=1)
        near = np.sort(np.argsort(d2, kind="stable")[:m])
        out[c, :len(near)] = near
    return out


def predict(data_spec, cross_spec, x, yerr, r, t, nbr):
    """(mu, var) of the test points t for the table nbr (M, m): -1 anywhere is padding, entries in any order"""
    x, t = _as_2d(x), _as_2d(t)
    yerr = np.zeros(len(x)) + yerr
    r = np.asarray(r, dtype=np.float64)
    kss = solver_np.kernel_matrix(cross_spec, t, diag=True)
    mu, var = np.zeros(len(t)), np.array(kss, dtype=np.float64)
    for i in range(len(t)):
        c = np.sort(nbr[i][nbr[i] >= 0])
        if not len(c):
            continue
        Kcc = solver_np.kernel_matrix(data_spec, x[c])
        Kcc[np.diag_indices_from(Kcc)] += yerr[c] ** 2
        kc = solver_np.kernel_matrix(cross_spec, x[c], t[i:i + 1])[:, 0]
        cf = cho_factor(Kcc, lower=True)
        mu[i] = np.dot(kc, cho_solve(cf, r[c]))
        var[i] = kss[i] - np.dot(kc, cho_solve(cf, kc))
    return mu, var


def full_table(n, ntest):
    """every data point in every set (n <= 64 on the device)"""
    return np.tile(np.arange(n, dtype=np.int32), (ntest, 1))


def gaps(spec, x, yerr, r, xs):
    """What two float64 routes on the CPU differ by on the same inputs with every data point in every conditioning set: this
    restatement against dense LAPACK (``vecchia_ref.dense``); ``mu`` over its largest absolute entry, ``var`` over its largest
    entry.  Returns (dict(mu, var), (mu, var) of the restatement, the dense dict)."""
    x, xs = _as_2d(x), _as_2d(xs)
    mu, var = predict(spec, spec, x, yerr, r, xs, full_table(len(x), len(xs)))
    d = vecchia_ref.dense(spec, x, yerr, r, xs)
    return dict(mu=vecchia_ref.rel(mu, d["mu"]), var=vecchia_ref.rel(var, d["var"])), (mu, var), d
