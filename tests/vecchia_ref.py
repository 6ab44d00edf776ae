"""NumPy restatement of the Vecchia solver (``george_amd.VecchiaSolver``, george_amd/csrc/gh_vecchia.hip): a plain loop over points.

For point ``i`` with neighbour list ``c`` (predecessors of ``i``, at most ``m``) and the block ``A = K[c + {i}, c + {i}]``,
``K`` including ``yerr^2`` on its diagonal:

    b_i = K_cc^-1 k_ci,   f_i = k_ii - k_ci^T b_i,   u = [-b_i; 1],   e_i = r_i - b_i^T r_c,   z = K_cc^-1 r_c,  ze = [z; 0]
    log|K| ~ sum_i log f_i,     r^T K^-1 r ~ sum_i e_i^2 / f_i,     K^-1 ~ Q = (I - B)^T F^-1 (I - B)
    W(i) = 1/2 (e^2/f^2 - 1/f) u u^T + 1/2 (e/f) (ze u^T + u ze^T),     d log p(y_i | y_c) / dtheta = sum_jk W(i)_jk dA_jk/dtheta

``kgrad[a] = sum_i sum_jk W(i)_jk dk(x_j, x_k)/dtheta_a``, ``alpha = Q r``, ``diagA_j = 2 sum_{blocks with j} W_jj``: the layout of
``BasicSolver.grad``, so that ``GP._assemble_grad`` applies unchanged; with every predecessor in ``c`` these are the dense values.
``S[a]`` is the same sum over absolute values: the scale a gradient error is measured against.  Prediction:
``mu = K* alpha``, ``V = F^-1/2 (I - B) K*^T``, ``var = k** - colsumsq(V)``, ``cov = K** - V^T V``.

Kernel values and gradients come from ``oracle.solver_np`` (symmetric calls on index-sorted points: the lower index is the first
argument), a chunk of points at a time on the union of the chunk's blocks; block solves are SciPy ``cho_factor`` / ``cho_solve``.
Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import solver_np

CHUNK = 256


def brute_force_neighbors(x, m):
    """row i: the min(i, m) nearest predecessors of i (squared Euclidean distance, ties to the lower index), ascending, padded -1"""
    x = np.asarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    out = np.full((len(x), m), -1, dtype=np.int32)
    for i in range(1, len(x)):
        d2 = ((x[:i] - x[i]) ** 2).sum(axis=1)
        c = np.sort(np.argsort(d2, kind="stable")[:m])
        out[i, :len(c)] = c
    return out


class VecchiaRef(object):
    """``B`` (n, m) in the table's slots (zero where it is padded), ``f``, ``logdet``; with a residual also ``e``, ``quad``,
    ``alpha``; with ``want_grad`` also ``kgrad``, ``S`` (P,) and ``diagA``."""

    def lists(self):
        return [row[row >= 0] for row in self.nbr]

    def forward(self, R, power=0.0):
        """F^-power (I - B) R for R of shape (n,) or (n, k)"""
        R = np.asarray(R, dtype=np.float64)
        out = R.copy()
        for i, c in enumerate(self.lists()):
            if len(c):
                out[i] -= np.tensordot(self.B[i, self.nbr[i] >= 0], R[c], axes=(0, 0))
        scale = self.f ** -power
        return out * (scale if R.ndim == 1 else scale[:, None])

    def apply_q(self, R):
        W = self.forward(R, power=1.0)
        out = W.copy()
        for i, c in enumerate(self.lists()):
            if len(c):
                out[c] -= np.multiply.outer(self.B[i, self.nbr[i] >= 0], W[i])
        return out

    def log_likelihood(self):
        return -0.5 * (self.quad + self.logdet + len(self.f) * np.log(2.0 * np.pi))

    def predict(self, spec, xs):
        Kx = solver_np.kernel_matrix(spec, self.x, xs)                      # K*^T, (n, M)
        V = self.forward(Kx, power=0.5)
        mu = np.dot(Kx.T, self.alpha)
        var = solver_np.kernel_matrix(spec, xs, diag=True) - np.sum(V * V, axis=0)
        cov = solver_np.kernel_matrix(spec, xs) - np.dot(V.T, V)
        return mu, var, cov


def reference(spec, x, yerr, nbr, r=None, want_grad=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    n, m = nbr.shape
    yerr = np.zeros(n) + yerr
    ref = VecchiaRef()
    ref.x, ref.nbr = x, np.asarray(nbr)
    ref.B, ref.f = np.zeros((n, m)), np.empty(n)
    if r is not None:
        ref.e = np.empty(n)
    if want_grad:
        ref.diagA = np.zeros(n)
        ref.kgrad = ref.S = None
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        rows = ref.nbr[lo:hi]
        pts = np.unique(np.concatenate([rows[rows >= 0], np.arange(lo, hi)]))      # index-sorted: lower index first
        Ku = solver_np.kernel_matrix(spec, x[pts])
        Ku[np.diag_indices_from(Ku)] += yerr[pts] ** 2
        dKu = solver_np.kernel_gradient(spec, x[pts]) if want_grad else None
        for i in range(lo, hi):
            slots = ref.nbr[i] >= 0
            c = ref.nbr[i][slots]
            blk = np.searchsorted(pts, np.concatenate([c, [i]]))
            A = Ku[np.ix_(blk, blk)]
            nc = len(c)
            b = z = np.zeros(0)
            if nc:
                cf = cho_factor(A[:nc, :nc], lower=True)
                b = cho_solve(cf, A[:nc, nc])
            f = A[nc, nc] - np.dot(A[:nc, nc], b)
            ref.B[i, slots], ref.f[i] = b, f
            if r is None:
                continue
            e = r[i] - np.dot(b, r[c])
            ref.e[i] = e
            if not want_grad:
                continue
            if nc:
                z = cho_solve(cf, r[c])
            u, ze = np.concatenate([-b, [1.0]]), np.concatenate([z, [0.0]])
            W = 0.5 * (e * e / (f * f) - 1.0 / f) * np.outer(u, u) + 0.5 * (e / f) * (np.outer(ze, u) + np.outer(u, ze))
            dA = dKu[np.ix_(blk, blk)]
            g, s = np.einsum("jk,jkp->p", W, dA), np.einsum("jk,jkp->p", np.abs(W), np.abs(dA))
            ref.kgrad = g if ref.kgrad is None else ref.kgrad + g
            ref.S = s if ref.S is None else ref.S + s
            np.add.at(ref.diagA, np.concatenate([c, [i]]), 2.0 * np.diag(W))
    ref.logdet = np.sum(np.log(ref.f))
    if r is not None:
        ref.quad = np.sum(ref.e ** 2 / ref.f)
        ref.alpha = ref.apply_q(r)
    return ref


def dense(spec, x, yerr, r, xs=None):
    """The dense answers by LAPACK: dict(logdet, quad, Kinv, alpha, kgrad = 1/2 sum A_ij dK_ij, S, diagA, and mu / var / cov)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    K = solver_np.kernel_matrix(spec, x)
    K[np.diag_indices_from(K)] += (np.zeros(len(x)) + yerr) ** 2
    cf = cho_factor(K, lower=True)
    Kinv = cho_solve(cf, np.eye(len(x)))
    alpha = cho_solve(cf, r)
    Am = np.outer(alpha, alpha) - Kinv
    dK = solver_np.kernel_gradient(spec, x)
    out = dict(logdet=2.0 * np.sum(np.log(np.diag(cf[0]))), quad=np.dot(r, alpha), Kinv=Kinv, alpha=alpha,
               kgrad=0.5 * np.einsum("ij,ijp->p", Am, dK), S=0.5 * np.einsum("ij,ijp->p", np.abs(Am), np.abs(dK)), diagA=np.diag(Am).copy())
    if xs is not None:
        Kx = solver_np.kernel_matrix(spec, x, xs)
        W = cho_solve(cf, Kx)
        out.update(mu=np.dot(Kx.T, alpha), var=solver_np.kernel_matrix(spec, xs, diag=True) - np.sum(Kx * W, axis=0),
                   cov=solver_np.kernel_matrix(spec, xs) - np.dot(Kx.T, W))
    return out


def rel(a, b):
    """largest |a - b| over the largest |b| (scalars: the relative difference)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def gaps(spec, x, yerr, r, xs):
    """What two float64 routes on the CPU differ by for the same inputs with every predecessor in the conditioning set: the
    restatement against dense LAPACK, per compared quantity (vectors and matrices over their largest entry, the gradient over
    its sum of absolute terms)."""
    n = len(x)
    full = np.full((n, max(n - 1, 1)), -1, dtype=np.int32)
    for i in range(1, n):
        full[i, :i] = np.arange(i)
    ref = reference(spec, x, yerr, full, r=r, want_grad=True)
    d = dense(spec, x, yerr, r, xs)
    mu, var, cov = ref.predict(spec, xs)
    return dict(logdet=rel(ref.logdet, d["logdet"]), quad=rel(ref.quad, d["quad"]), alpha=rel(ref.alpha, d["alpha"]),
                Kinv=rel(ref.apply_q(np.eye(n)), d["Kinv"]), kgrad=float(np.max(np.abs(ref.kgrad - d["kgrad"]) / d["S"])),
                diagA=rel(ref.diagA, d["diagA"]), mu=rel(mu, d["mu"]), var=rel(var, d["var"]), cov=rel(cov, d["cov"])), ref, d
