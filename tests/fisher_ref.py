"""CPU reference for the expected (Fisher) information of a GP's hyper-parameters, and the tolerance that pins it.

With ``K = k(x, x) + diag(yerr^2)`` and derivative matrices ``D_a`` -- first the diagonal ones ``diag(diag_rows[p])`` (how a
white-noise model enters), then ``dK/dtheta`` of every kernel parameter --

    F_ab = 1/2 tr(K^-1 D_a K^-1 D_b) = 1/2 sum_ij M_a[i, j] M_b[j, i],      M_a = K^-1 D_a.

``reference()`` evaluates it independently of every HIP path: ``K`` from ``oracle.solver_np.kernel_matrix``, ``dK`` from
``oracle.kernels_np.gradient_general``, the inverse from SciPy ``cho_factor`` / ``cho_solve`` refined by two Newton steps
``X += X (I - K X)`` in ``np.longdouble``; the products and the contraction run in ``np.longdouble`` too.

Tolerance: the project's one rule (tests/grad_ref.py), ``|F_ab - ref| <= C_TOL * U * kappa(K) * S_ab`` with the scale

    S_ab = sqrt(F_aa F_bb).

F is positive semidefinite, so ``|F_ab| <= S_ab``: the scale is that of the result's own diagonal.  A zero scale (a masked
parameter) asks for an exact 0, as ``Ref._ratio`` does.  The operand scale of the other references,
``1/2 sum (|K^-1| |D_a|)(|K^-1| |D_b|)``, must not be used here: on these problems it lets errors of 35 % through (hyper,
N = 300).  Two independent fp64 routes (via K^-1 and via L^-1 D L^-T) differ from the long-double value by at most 1.8e-13
relative to ``S_ab`` on the problems used (kappa up to 1e5): at most 5e-4 of the tolerance.

The problems are those of tests/loo_ref.py (error bars at least 0.1 of the amplitude); ``diag_rows_for`` gives the two
diagonal parameters of the tests, one constant and one varying along x.  ``defect=`` runs a deliberately wrong version
(tests/test_fisher_reference.py checks that the rule rejects each).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from grad_ref import U, C_TOL, Ref, _as_2d
from loo_ref import problem, KERNELS, PAD        # noqa: F401  (the problems are shared)
from oracle import kernels_np, solver_np

LD = np.longdouble
TILE = 64

DEFECTS = ("factor_one", "no_transpose", "drop_last_row", "drop_offdiag_tile", "padded_rows", "diag_as_kernel_only")


class FisherRef(object):
    """What ``reference()`` returns: ``F`` (P, P) with P = n_diag + full kernel size, ``S`` (P, P), ``kappa``, ``n_diag``."""

    def tol(self):
        return C_TOL * U * self.kappa * self.S

    def ratio(self, value, keep=None):
        """largest |error| / tolerance (<= 1 passes); ``keep``: the rows / columns of the reference that ``value`` covers"""
        F, tol = self.F, self.tol()
        if keep is not None:
            keep = np.asarray(keep)
            F, tol = F[np.ix_(keep, keep)], tol[np.ix_(keep, keep)]
        return Ref._ratio(np.asarray(value, dtype=np.float64) - F, tol)


def diag_rows_for(x, yerr):
    """the two diagonal parameters of the tests: a constant white noise ``exp(w)``, ``w = log(0.5 min yerr^2)``, and a
    log-variance ramp along the first coordinate, ``exp(w + 0.1 x_0) * x_0``"""
    x = _as_2d(x)
    w = np.log(0.5 * np.min(np.asarray(yerr, dtype=np.float64) ** 2))
    return np.stack([np.full(len(x), np.exp(w)), np.exp(w + 0.1 * x[:, 0]) * x[:, 0]])


def refined_inverse(K):
    """K^-1 in long double: LAPACK's inverse and two Newton steps on it"""
    n = len(K)
    X = cho_solve(cho_factor(K, lower=True), np.eye(n)).astype(LD)
    Kl = K.astype(LD)
    eye = np.eye(n, dtype=LD)
    for _ in range(2):
        X = X + np.dot(X, eye - np.dot(Kl, X))
    return X


def planes(kernel, x, yerr, diag_rows=None):
    """``(K, X = K^-1 (long double), M (P, N, N) long double, n_diag)``: the undamaged pieces of the reference"""
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    X = refined_inverse(K)
    rows = np.zeros((0, n)) if diag_rows is None else np.atleast_2d(np.asarray(diag_rows, dtype=np.float64))
    if rows.shape[1] != n:
        raise ValueError("diag_rows must be (n_diag, n)")
    G = np.asarray(kernels_np.gradient_general(kernel, x, x), dtype=np.float64)
    M = [X * r.astype(LD)[None, :] for r in rows]
    M += [np.dot(X, G[:, :, p].astype(LD)) for p in range(G.shape[2])]
    return K, X, (np.stack(M) if M else np.zeros((0, n, n), dtype=LD)), len(rows)


def contract(M, transpose=True):
    P = len(M)
    F = np.zeros((P, P), dtype=LD)
    for a in range(P):
        for b in range(a, P):
            F[a, b] = F[b, a] = 0.5 * np.sum(M[a] * (M[b].T if transpose else M[b]), dtype=LD)
    return F


def reference(kernel, x, yerr, diag_rows=None, defect=None, pieces=None):
    """The information reference (module docstring) for ``kernel`` at inputs ``x`` with per-point standard deviations
    ``yerr`` (white noise included).  ``pieces``: what ``planes()`` returned for the same arguments (the long-double products
    are the expensive part; the defects share them)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    K, X, M, n_diag = pieces if pieces is not None else planes(kernel, x, yerr, diag_rows)
    n = len(K)
    if defect in ("padded_rows", "diag_as_kernel_only") and n_diag == 0:
        raise ValueError("defect %s needs diag_rows" % defect)
    good = contract(M)
    F = good.copy()
    if defect == "factor_one":
        F = 2.0 * F
    elif defect == "no_transpose":
        F = contract(M, transpose=False)
    elif defect == "drop_last_row":
        W = M.copy()
        W[:, n - 1, :] = 0.0
        F = contract(W)
    elif defect == "drop_offdiag_tile":
        if n <= TILE:
            raise ValueError("defect drop_offdiag_tile needs more than one tile")
        W = M.copy()
        W[len(M) - 1, TILE:2 * TILE, :TILE] = 0.0
        F = contract(W)
    elif defect == "padded_rows":
        # identity rows of the padded K^-1 against a diagonal plane whose entries continue past n with the last value
        npad = -(-n // PAD) * PAD - n
        rows = np.atleast_2d(np.asarray(diag_rows, dtype=np.float64))
        for a in range(n_diag):
            for b in range(n_diag):
                F[a, b] += 0.5 * npad * LD(rows[a, -1]) * LD(rows[b, -1])
    elif defect == "diag_as_kernel_only":
        F[:n_diag, n_diag:] = 0.0
        F[n_diag:, :n_diag] = 0.0

    out = FisherRef()
    out.F = F.astype(np.float64)
    d = np.sqrt(np.diag(good).astype(np.float64))
    out.S = np.outer(d, d)
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(X.astype(np.float64), 1))
    out.n_diag = n_diag
    return out


_CACHE = {}


def cached(name, n, with_diag=True):
    """``(kernel, x, yerr, diag_rows, reference)`` of the test problem (name, n), computed once per process and left unchanged"""
    key = (name, n, with_diag)
    if key not in _CACHE:
        kernel, x, yerr, _ = problem(name, n)
        rows = diag_rows_for(x, yerr) if with_diag else None
        _CACHE[key] = (kernel, x, yerr, rows, reference(kernel, x, yerr, rows))
    return _CACHE[key]
