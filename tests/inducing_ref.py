"""NumPy restatement of the inducing-point solver (``george_amd.InducingSolver``, george_amd/csrc/gh_inducing.hip), formula by
formula as include/george_amd.h defines it.  With ``s_i = yerr_i^2``, inducing inputs ``u``, an absolute ``jitter`` and
``phi = 0`` (DTC) or ``1`` (FITC):

    K_uu + jitter I = L_u L_u^T,   V = L_u^-1 K_uf,   q_i = |V[:, i]|^2,   lambda_i = s_i + phi max(k(x_i, x_i) - q_i, 0)
    C = V^T V + diag(lambda),   A = I + V Lambda^-1 V^T = L_A L_A^T,   H = L_A^-1 V
    log|C| = sum log lambda_i + 2 sum log diag L_A,   t(b) = H Lambda^-1 b,   C^-1 b = Lambda^-1 b - Lambda^-1 H^T t(b)
    alpha = C^-1 r,   diagA_i = alpha_i^2 - (1/lambda_i - |H[:, i]|^2 / lambda_i^2)
    P = K_uu^-1 K_uf,   T = (P alpha) alpha^T - P C^-1,   Z = T - phi P diag(diagA),   W = -1/2 Z P^T
    kgrad[a] = sum_ij Z_ji dk(x_i, u_j)/da + sum_jj' W_jj' dk(u_j, u_j')/da + 1/2 phi sum_i diagA_i dk(x_i, x_i)/da
    V* = L_u^-1 K(u, xs),  H* = L_A^-1 V*:   mu = H*^T t(r),  var = k** - colsumsq(V*) + colsumsq(H*),  cov = K** - V*^T V* + H*^T H*

``kgrad``, ``alpha`` and ``diagA`` have the layout of ``BasicSolver.grad``, so that ``GP._assemble_grad`` applies unchanged.
``S[a]`` is the sum of the absolute values of the terms of ``kgrad[a]``: the scale a gradient error is measured against.

Kernel values and gradients come from ``oracle.solver_np``: ``K_fu = K(x, u)`` with the data point as the first argument, and
the gradients from one symmetric call on the stacked points ``[x; u]`` (the lower index is the first argument: ``x_i`` before
``u_j``, ``u_j`` before ``u_j'`` for ``j < j'``).  ``dense_model`` gives the same quantities from the explicit N x N matrix
``C`` by LAPACK, the gradient as ``1/2 sum_ij (alpha alpha^T - C^-1)_ij dC_ij/da`` with ``dC`` differentiated term by term: an
independent route.

``route="blocks"`` never forms the stacked ((N + m), (N + m), P) tensor: per block of at most ``BLOCK`` data points it takes
``dk(x_i, u_j)`` and ``dk(x_i, x_i)`` from one symmetric call on ``[x_block; u]``, and ``dk(u_j, u_j')`` from one call on ``u``;
``kgrad`` and ``S`` are the same einsum sums, block after block (N = 4200, m = 65, two parameters: 0.2 s against 4.3 s, the two
routes 3e-17 of ``S`` apart).  ``defect=`` runs a deliberately wrong gradient (``DEFECTS``; tests/test_inducing_host.py checks
that the bound of the device tests rejects each one).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, cholesky, solve_triangular

from oracle import solver_np

PHI = {"dtc": 0.0, "fitc": 1.0}
BLOCK = 256              # data points per block of route="blocks"
TILE = 64                # edge of a tile of the device reduction (gh_inducing.hip IND_GT)
DIAG_POINTS = TILE * TILE    # data points per workgroup of the device's FITC diagonal term

# Deliberately wrong gradients.  The last four change nothing under DTC (phi = 0 already), and ``fitc_first_4096`` nothing up
# to 4096 points.
DEFECTS = ("drop_last_tile",         # the rectangular term without its last tile: the last tile row x the last tile column
           "drop_last_pair",         # .. without the single pair (x_{N-1}, u_{m-1})
           "kuu_lower_once",         # the K_uu term with W not symmetrised: the lower triangle counted once
           "fitc_first_4096",        # the FITC diagonal term over the first 4096 points only (one workgroup of the device kernel)
           "fitc_weight_one",        # the FITC diagonal term with weight 1 instead of 1/2
           "z_phi_zero")             # Z (and W with it) without its FITC part


def _two_d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def max_min_points(x, m):
    """brute-force greedy max-min selection: nearest the centroid first, then the largest minimum squared distance to the chosen
    set, ties to the lower index"""
    x = _two_d(x)
    n = len(x)
    c = x.mean(axis=0)
    chosen = [min(range(n), key=lambda i: (((x[i] - c) ** 2).sum(), i))]
    while len(chosen) < min(m, n):
        best, best_d = -1, -1.0
        for i in range(n):
            d = min(((x[i] - x[j]) ** 2).sum() for j in chosen)
            if d > best_d:
                best, best_d = i, d
        chosen.append(best)
    return np.array(chosen, dtype=np.int64)


class InducingRef(object):
    """``lam``, ``logdet``, the factors; with a residual ``quad``, ``alpha``, ``t``; with ``want_grad`` also ``diagA``,
    ``kgrad`` and ``S`` (P,)."""

    def solve(self, b):
        b = np.asarray(b, dtype=np.float64)
        lam = self.lam if b.ndim == 1 else self.lam[:, None]
        t = np.dot(self.H, b / lam)
        return b / lam - np.dot(self.H.T, t) / lam

    def log_likelihood(self):
        return -0.5 * (self.quad + self.logdet + len(self.lam) * np.log(2.0 * np.pi))

    def predict(self, spec, xs):
        xs = _two_d(xs)
        Vs = solve_triangular(self.Lu, solver_np.kernel_matrix(spec, xs, self.u).T, lower=True)
        Hs = solve_triangular(self.LA, Vs, lower=True)
        mu = np.dot(Hs.T, self.t)
        var = solver_np.kernel_matrix(spec, xs, diag=True) - np.sum(Vs * Vs, axis=0) + np.sum(Hs * Hs, axis=0)
        cov = solver_np.kernel_matrix(spec, xs) - np.dot(Vs.T, Vs) + np.dot(Hs.T, Hs)
        return mu, var, cov


def reference(spec, x, yerr, u, jitter, method, r=None, want_grad=False, route="stacked", defect=None):
    if route not in ("stacked", "blocks") or (defect is not None and defect not in DEFECTS):
        raise ValueError((route, defect))
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    phi = PHI[method]
    ref = InducingRef()
    ref.x, ref.u = x, u
    Kuu = solver_np.kernel_matrix(spec, u) + jitter * np.eye(m)
    Kfu = solver_np.kernel_matrix(spec, x, u)
    ref.Lu = cholesky(Kuu, lower=True)
    V = solve_triangular(ref.Lu, Kfu.T, lower=True)
    q = np.sum(V * V, axis=0)
    ref.lam = (np.zeros(n) + yerr) ** 2 + phi * np.maximum(solver_np.kernel_matrix(spec, x, diag=True) - q, 0.0)
    ref.LA = cholesky(np.eye(m) + np.dot(V / ref.lam, V.T), lower=True)
    ref.H = solve_triangular(ref.LA, V, lower=True)
    ref.logdet = np.sum(np.log(ref.lam)) + 2.0 * np.sum(np.log(np.diag(ref.LA)))
    if r is None:
        return ref
    r = np.asarray(r, dtype=np.float64)
    ref.t = np.dot(ref.H, r / ref.lam)
    ref.quad = np.sum(r * r / ref.lam) - np.dot(ref.t, ref.t)
    ref.alpha = ref.solve(r)
    if not want_grad:
        return ref
    ref.diagA = ref.alpha ** 2 - (1.0 / ref.lam - np.sum(ref.H * ref.H, axis=0) / ref.lam ** 2)
    P = cho_solve((ref.Lu, True), Kfu.T)                                        # (m, n)
    PCinv = ref.solve(P.T).T
    Z = np.outer(np.dot(P, ref.alpha), ref.alpha) - PCinv - (0.0 if defect == "z_phi_zero" else phi) * P * ref.diagA[None, :]
    W = -0.5 * np.dot(Z, P.T)
    wd = phi * (1.0 if defect == "fitc_weight_one" else 0.5) * ref.diagA       # the weights of dk(x_i, x_i)
    if defect == "drop_last_tile":
        Z[TILE * ((m - 1) // TILE):, TILE * ((n - 1) // TILE):] = 0.0
    if defect == "drop_last_pair":
        Z[m - 1, n - 1] = 0.0
    if defect == "kuu_lower_once":
        W = np.tril(W)
    if defect == "fitc_first_4096":
        wd[DIAG_POINTS:] = 0.0
    if route == "stacked":
        dK = solver_np.kernel_gradient(spec, np.vstack([x, u]))                 # ((n + m), (n + m), P): x first, u behind
        parts = [(0, n, dK[:n, n:], dK[np.arange(n), np.arange(n)])]
        duu = dK[n:, n:]
    else:
        parts = []
        for s in range(0, n, BLOCK):
            e = min(n, s + BLOCK)
            dK = solver_np.kernel_gradient(spec, np.vstack([x[s:e], u]))
            parts.append((s, e, dK[:e - s, e - s:], dK[np.arange(e - s), np.arange(e - s)]))
        duu = solver_np.kernel_gradient(spec, u)
    # the three terms, each summed over the blocks first: rectangular, K_uu, FITC diagonal
    ref.kgrad = (sum(np.einsum("ji,ijp->p", Z[:, s:e], dfu) for s, e, dfu, _ in parts) + np.einsum("jk,jkp->p", W, duu) +
                 sum(np.einsum("i,ip->p", wd[s:e], dff) for s, e, _, dff in parts))
    ref.S = (sum(np.einsum("ji,ijp->p", np.abs(Z[:, s:e]), np.abs(dfu)) for s, e, dfu, _ in parts) +
             np.einsum("jk,jkp->p", np.abs(W), np.abs(duu)) +
             sum(np.einsum("i,ip->p", np.abs(wd[s:e]), np.abs(dff)) for s, e, _, dff in parts))
    return ref


def dense_model(spec, x, yerr, u, jitter, method, r, xs=None, want_grad=True):
    """The same quantities from the explicit C by LAPACK: dict(C, logdet, quad, Cinv, alpha, diagA, kgrad, and mu / var / cov)."""
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    phi = PHI[method]
    r = np.asarray(r, dtype=np.float64)
    Kuu = solver_np.kernel_matrix(spec, u) + jitter * np.eye(m)
    Kfu = solver_np.kernel_matrix(spec, x, u)
    cu = cho_factor(Kuu, lower=True)
    P = cho_solve(cu, Kfu.T)                                                    # K_uu^-1 K_uf
    Q = np.dot(Kfu, P)
    lam = (np.zeros(n) + yerr) ** 2 + phi * np.maximum(solver_np.kernel_matrix(spec, x, diag=True) - np.diag(Q), 0.0)
    Cm = Q + np.diag(lam)
    cf = cho_factor(Cm, lower=True)
    Cinv = cho_solve(cf, np.eye(n))
    alpha = cho_solve(cf, r)
    Am = np.outer(alpha, alpha) - Cinv
    out = dict(C=Cm, lam=lam, logdet=2.0 * np.sum(np.log(np.diag(cf[0]))), quad=np.dot(r, alpha), Cinv=Cinv, alpha=alpha,
               diagA=np.diag(Am).copy())
    if want_grad:
        dK = solver_np.kernel_gradient(spec, np.vstack([x, u]))
        dfu, duu, dff = dK[:n, n:], dK[n:, n:], dK[np.arange(n), np.arange(n)]
        g = np.empty(dK.shape[2])
        for a in range(dK.shape[2]):
            dQ = np.dot(dfu[:, :, a], P)
            dQ = dQ + dQ.T - np.dot(P.T, np.dot(duu[:, :, a], P))
            dC = dQ + phi * np.diag(dff[:, a] - np.diag(dQ))
            g[a] = 0.5 * np.sum(Am * dC)
        out["kgrad"] = g
    if xs is not None:
        xs = _two_d(xs)
        Qsf = np.dot(solver_np.kernel_matrix(spec, xs, u), P)                   # K*u K_uu^-1 K_uf
        Wm = cho_solve(cf, Qsf.T)
        out.update(mu=np.dot(Qsf, alpha), var=solver_np.kernel_matrix(spec, xs, diag=True) - np.sum(Qsf.T * Wm, axis=0),
                   cov=solver_np.kernel_matrix(spec, xs) - np.dot(Qsf, Wm))
    return out


def rel(a, b):
    """largest |a - b| over the largest |b| (scalars: the relative difference)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny))


def gaps(spec, x, yerr, u, jitter, method, r, xs):
    """What two float64 routes on the CPU differ by for the same inputs: the restatement against ``dense_model``, per compared
    quantity (vectors and matrices over their largest entry, the gradient over its sum of absolute terms; 0 for a kernel
    without parameters).  Returns ``(gaps, ref, dense)``."""
    ref = reference(spec, x, yerr, u, jitter, method, r=r, want_grad=True)
    d = dense_model(spec, x, yerr, u, jitter, method, r, xs)
    mu, var, cov = ref.predict(spec, xs)
    g = dict(logdet=rel(ref.logdet, d["logdet"]), quad=rel(ref.quad, d["quad"]), alpha=rel(ref.alpha, d["alpha"]),
             Cinv=rel(ref.solve(np.eye(len(ref.lam))), d["Cinv"]), kgrad=float(np.max(np.abs(ref.kgrad - d["kgrad"]) / np.maximum(ref.S, np.finfo(float).tiny), initial=0.0)),
             diagA=rel(ref.diagA, d["diagA"]), mu=rel(mu, d["mu"]), var=rel(var, d["var"]), cov=rel(cov, d["cov"]))
    return g, ref, d
