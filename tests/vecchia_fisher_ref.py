"""NumPy restatement of ``VecchiaSolver.fisher_blocks`` (gh_vecchia_fisher, george_amd/csrc/gh_vecchia.hip): the expected (Fisher)
information of the Vecchia likelihood as a plain loop over points, and what the tests of it share -- the problems, the bound and
the LDS size of the device kernel.  Nothing here touches a device.

For point ``i`` with neighbour list ``c`` and the block ``A = K[c + {i}, c + {i}]`` (``yerr^2`` on the diagonal, ``i`` last):
``b = K_cc^-1 k_ci``, ``f = k_ii - k_ci^T b``, ``u = [-b; 1]``, ``L`` the Cholesky factor of ``K_cc``, and for every derivative
plane ``D_a`` restricted to the block -- first the diagonal ones ``diag(diag_rows[p])``, then ``dK/dtheta`` of every kernel
parameter (the lower index is the first argument) --

    v_a = D_a u,    df_a = u^T v_a,    w_a = L^-1 (v_a)[:c],    F_ab += 1/2 df_a df_b / f^2 + (w_a . w_b) / f.

With every predecessor in ``c`` this is the dense ``1/2 tr(K^-1 D_a K^-1 D_b)`` of tests/fisher_ref.py; for smaller sets it is a
different quantity (the information of the approximate likelihood), so the device is compared with THIS formula.  The scale of an
error is ``S_ab = sqrt(F_aa F_bb)``, as in fisher_ref.

The bound is the rule of tests/vecchia_cases.py, nothing new: per problem ``1000 x`` the gap -- over ``S_ab`` -- between this
restatement with every predecessor in the set and ``fisher_ref.reference`` (dense, long double) on the first ``GAP_N`` = 150 points
of the problem's own inputs, a gap counting as at least ``4 eps`` and asserted not to exceed ``GAP_CAP`` = 1e-9.  An entry whose
scale is zero must be exactly zero.

``defect=`` runs a deliberately wrong version (tests/test_vecchia_fisher_host.py checks that the bound rejects each):

===================  ==============================================================================================
``no_mean_term``     ``(w_a . w_b) / f`` left out: only the variance term of each conditional
``factor_one``       ``df_a df_b / f^2`` without its 1/2
``drop_last_slot``   the block's last slot (the point itself) left out of ``df_a``: a sum over ``c`` instead of ``c + 1``
``diag_unpermuted``  the diagonal rows read at the slot's position in the block instead of at the point's index: rows that
                     did not follow the points into the solver's order
===================  ==============================================================================================

Test helper only: not a conftest.
"""
import functools

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import fisher_ref
import grad_ref
import vecchia_cases as VC
from george_amd import kernels
from george_amd.solvers.vecchia import vecchia_neighbors
from oracle import solver_np

DEFECTS = ("no_mean_term", "factor_one", "drop_last_slot", "diag_unpermuted")
EPS = VC.EPS
GAP_N = VC.GAP_N
GAP_CAP = VC.GAP_CAP
V_FISHER_LDS = 128 * 1024    # gh_vecchia.hip: the raised limit of vecchia_fisher_kernel's dynamic LDS
V_FISHER_PLANES = 64         # .. and the planes of one call
CHUNK = 256


class VecchiaFisherRef(object):
    """``F`` (P, P) with P = n_diag + full kernel size, ``S`` (P, P) = sqrt(F_aa F_bb) of the undamaged formula, ``n_diag``"""


def full_table(n):
    """every predecessor in the conditioning set"""
    full = np.full((n, max(n - 1, 1)), -1, dtype=np.int32)
    for i in range(1, n):
        full[i, :i] = np.arange(i)
    return full


def reference(spec, x, yerr, nbr, diag_rows=None, which=None, defect=None):
    """The information of the Vecchia likelihood with the table ``nbr`` (module docstring).  ``diag_rows``: (n_diag, n) in the
    order of ``x``; ``which``: the kernel parameters kept (the others have rows and columns of 0)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    n = len(x)
    nbr = np.asarray(nbr)
    yerr = np.zeros(n) + yerr
    rows = np.zeros((0, n)) if diag_rows is None else np.atleast_2d(np.asarray(diag_rows, dtype=np.float64))
    if rows.shape[1] != n:
        raise ValueError("diag_rows must be (n_diag, n)")
    if defect == "diag_unpermuted" and len(rows) == 0:
        raise ValueError("defect diag_unpermuted needs diag_rows")
    n_diag, F, good = len(rows), None, None
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        tab = nbr[lo:hi]
        pts = np.unique(np.concatenate([tab[tab >= 0], np.arange(lo, hi)]))        # index-sorted: lower index first
        Ku = solver_np.kernel_matrix(spec, x[pts])
        Ku[np.diag_indices_from(Ku)] += yerr[pts] ** 2
        dKu = solver_np.kernel_gradient(spec, x[pts])
        for i in range(lo, hi):
            c = nbr[i][nbr[i] >= 0]
            idx = np.concatenate([c, [i]])
            blk = np.searchsorted(pts, idx)
            A, nc = Ku[np.ix_(blk, blk)], len(c)
            L = cholesky(A[:nc, :nc], lower=True) if nc else np.zeros((0, 0))
            b = solve_triangular(L, solve_triangular(L, A[:nc, nc], lower=True), lower=True, trans=1) if nc else np.zeros(0)
            f = A[nc, nc] - np.dot(A[:nc, nc], b)
            u = np.concatenate([-b, [1.0]])
            dA = dKu[np.ix_(blk, blk)]
            V = np.concatenate([rows[:, idx] * u[None, :], np.einsum("jkp,k->pj", dA, u)])     # (P, c + 1)
            for damaged in (False, True):
                if damaged:
                    V[:n_diag] = rows[:, :nc + 1] * u[None, :]
                df = np.dot(V, u)
                W = solve_triangular(L, V[:, :nc].T, lower=True).T if nc else np.zeros((len(V), 0))
                term = 0.5 * np.outer(df, df) / (f * f) + np.dot(W, W.T) / f
                if not damaged:
                    good = term if good is None else good + term
                if defect != "diag_unpermuted":
                    break
            if defect == "no_mean_term":
                term = 0.5 * np.outer(df, df) / (f * f)
            elif defect == "factor_one":
                term = np.outer(df, df) / (f * f) + np.dot(W, W.T) / f
            elif defect == "drop_last_slot":
                dfd = np.dot(V[:, :nc], u[:nc])
                term = 0.5 * np.outer(dfd, dfd) / (f * f) + np.dot(W, W.T) / f
            F = term if F is None else F + term
    if which is not None:
        gone = n_diag + np.flatnonzero(~np.asarray(which, dtype=bool))
        for M in (F, good):
            M[gone, :] = 0.0
            M[:, gone] = 0.0
    out = VecchiaFisherRef()
    out.F = 0.5 * (F + F.T)
    d = np.sqrt(np.diag(good))
    out.S = np.outer(d, d)
    out.n_diag = n_diag
    return out


# ------------------------------------------------------------------ the problems
def kernel_p62(K):
    """``grad_ref.kernel_p64`` without its last two one-parameter terms: 62 parameters in 16 dimensions, which with two diagonal
    rows are the 64 planes one call takes"""
    R = grad_ref
    return (R.kernel_p37(K)
            + R._amp(K, 0.3) * K.Matern32Kernel(R._spd(5, 23, 1.2), ndim=16, axes=list(range(8, 13)))
            + R._amp(K, 0.2) * K.Matern52Kernel([0.5, 0.8, 1.1, 1.4, 1.7, 2.0, 2.3, 2.6], ndim=16, axes=list(range(8, 16))))


CASES = (1, 5, 16, 17, 37, 62)


def problem(case, n=300):
    """(kernel, x, yerr, diag_rows): the inputs of ``vecchia_cases.pcase`` (case 62: those of P = 64 with ``kernel_p62``) and the
    two diagonal rows of ``fisher_ref.diag_rows_for``"""
    return _problem(case, n)


@functools.lru_cache(maxsize=None)
def _problem(case, n):
    kernel, x, yerr, r, xs = VC.pcase(64 if case == 62 else case, n)
    if case == 62:
        kernel = kernel_p62(kernels)
    return kernel, x, yerr, fisher_ref.diag_rows_for(x, yerr)


def _over(diff, scale):
    return VC._over(diff, scale)


def gap(case, n=300):
    """what the two CPU routes differ by over ``S_ab`` on the first ``GAP_N`` points of ``problem(case, n)``"""
    return _gap(case, n)


@functools.lru_cache(maxsize=None)
def _gap(case, n):
    kernel, x, yerr, rows = problem(case, n)
    k = min(n, GAP_N)
    dense = fisher_ref.reference(kernel, x[:k], yerr[:k], rows[:, :k])
    ref = reference(kernel, x[:k], yerr[:k], full_table(k), rows[:, :k])
    assert np.array_equal(ref.S == 0.0, dense.S == 0.0)
    g = _over(ref.F - dense.F, dense.S)
    print("gap", case, n, "%.1e" % g)
    assert g <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return g


def bound(case, n=300):
    return 1000.0 * max(gap(case, n), 4 * EPS)


@functools.lru_cache(maxsize=None)
def cached(case, n, m):
    """(the restatement with both diagonal rows, the table) of ``problem(case, n)`` with the default table of ``m`` neighbours"""
    kernel, x, yerr, rows = problem(case, n)
    nbr = vecchia_neighbors(x, m)
    return reference(kernel, x, yerr, nbr, rows), nbr


def clear():
    for f in (_problem, _gap, cached):
        f.cache_clear()


# ------------------------------------------------------------------ the device kernel's LDS
def fisher_lds_bytes(m, ndim, P, Q):
    """the dynamic LDS of vecchia_fisher_kernel for a kernel of ``P`` parameters and ``Q`` planes: what the gradient kernel
    takes (``vecchia_cases.grad_lds_bytes``), the plane area of ``Q`` rows of the odd pitch ``(m + 1) | 1``, the 64 values
    ``df_a`` and the ``Q (Q + 1) / 2`` packed pairs"""
    return VC.grad_lds_bytes(m, ndim, P) + 8 * (Q * ((m + 1) | 1) + VC.VM_MAX + Q * (Q + 1) // 2)
