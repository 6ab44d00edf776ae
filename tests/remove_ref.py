"""NumPy restatement of the blocked rank-k Cholesky update behind ``gh_chol_remove`` (george_amd/csrc/gh_chol_update.hip, "removing
points"), tile edge ``T`` a parameter.  Not a test: imported by tests/test_remove_host.py and tests/test_gpu_remove.py.

With ``keep`` / ``rem`` the kept / removed indices (both increasing) and L the current factor,

    K[keep, keep] = L[keep, :] L[keep, :]^T = Lk Lk^T + W W^T,      Lk = L[keep, keep],   W = L[keep, rem]

so the factor of the kept points is a rank-k UPDATE of Lk.  Per pass of at most ``kmax`` columns of W, and per diagonal tile j
from the tile that holds the first affected row (Wj: the tile's rows of W):

    V   = Ljj^-1 Wj
    L'  = chol(Ljj Ljj^T + Wj Wj^T)
    R^T R = I + V^T V,   Ri = R^-1
    Q   = [[Ljj^T L'^-T, -V Ri], [Wj^T L'^-T, Ri]]              (orthogonal)
    [Lij' | Wi'] = [Lij | Wi] Q   for every tile row i below j;   Wj is spent.

The columns of later passes are plain data of the OLD factor and are not transformed by earlier passes.
"""
import numpy as np


def split(n, removed):
    """(keep, rem): increasing int64 index arrays of the kept and the removed points of 0 .. n-1"""
    rem = np.unique(np.asarray(removed, dtype=np.int64))
    if len(rem) and (rem[0] < 0 or rem[-1] >= n):
        raise IndexError("index out of range")
    mask = np.ones(n, dtype=bool)
    mask[rem] = False
    return np.flatnonzero(mask).astype(np.int64), rem


def first_tile(removed, T):
    """j0: the rows in front of it keep their bits (T * (number of kept points before the first removed index) // T)"""
    return T * (int(np.min(removed)) // T)


def remove_ref(L, removed, T=128, kmax=128):
    """The lower Cholesky factor of K[keep, keep] from the lower factor ``L`` of K (n x n) by the blocked update."""
    L = np.tril(np.asarray(L, dtype=np.float64))
    n = len(L)
    keep, rem = split(n, removed)
    n2 = len(keep)
    if n2 == 0:
        raise ValueError("every point removed")
    if len(rem) == 0:
        return L.copy()
    npad = -(-n2 // T) * T
    A = np.eye(npad)
    A[:n2, :n2] = L[np.ix_(keep, keep)]
    for c0 in range(0, len(rem), kmax):
        rc = rem[c0:c0 + kmax]
        kc = len(rc)
        p0 = int(rc[0]) - c0                              # kept points in front of this pass's first column
        if p0 >= n2:
            break
        W = np.zeros((npad, kc))
        W[:n2] = L[np.ix_(keep, rc)] * (rc[None, :] < keep[:, None])
        for j in range(p0 // T, npad // T):
            s = slice(j * T, (j + 1) * T)
            Ljj, Wj = A[s, s].copy(), W[s].copy()
            Lnew = np.linalg.cholesky(Ljj @ Ljj.T + Wj @ Wj.T)
            A[s, s] = Lnew
            W[s] = 0.0
            if (j + 1) * T >= npad:
                break
            V = np.linalg.solve(Ljj, Wj)
            Ri = np.linalg.inv(np.linalg.cholesky(np.eye(kc) + V.T @ V).T)
            Lit = np.linalg.inv(Lnew).T
            Q = np.block([[Ljj.T @ Lit, -V @ Ri], [Wj.T @ Lit, Ri]])
            below = slice((j + 1) * T, npad)
            slab = np.hstack([A[below, s], W[below]]) @ Q
            A[below, s], W[below] = slab[:, :T], slab[:, T:]
    return np.tril(A[:n2, :n2])
