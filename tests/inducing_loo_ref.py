"""NumPy restatement of ``InducingSolver.loo_lowrank`` (gh_inducing_loo, george_amd/csrc/gh_inducing.hip): leave-one-out
cross-validation of the DTC / FITC density ``N(r | 0, C)``, ``C = K_fu K_uu^-1 K_uf + diag(lambda)``, exact for it, in two routes.

``reference`` is the low-rank route on the factors of ``inducing_ref.reference``.  With ``D = Lambda^-1``, ``R = H D`` (m x N),
``P = K_uu^-1 K_uf`` and ``phi = 0`` (DTC) or ``1`` (FITC), ``C^-1 = D - R^T R`` and

    c_i     = 1/lambda_i - |H[:, i]|^2 / lambda_i^2,   alpha = C^-1 r,   resid = alpha / c,   var = 1 / c
    lpd_i   = 1/2 log c_i - 1/2 alpha_i resid_i - 1/2 log 2 pi,   L = sum_i lpd_i
    w       = 1/2 (1 + alpha resid) / c,   v = C^-1 resid
    S_w     = R diag(w) R^T,   G1 = R P^T,   G3 = R diag(w D) P^T
    d2_i    = w_i D_i^2 - 2 w_i D_i |R[:, i]|^2 + R[:, i]^T S_w R[:, i]              (= (C^-1 diag(w) C^-1)_ii)
    diagB_i = alpha_i v_i - d2_i                                                    (= dL / dC_ii)
    (C^-1 diag(w) C^-1 P^T) = diag(w D^2) P^T - diag(w D) R^T G1 - R^T G3 + R^T S_w G1
    Z^T     = alpha (P v)^T + v (P alpha)^T - 2 (C^-1 diag(w) C^-1 P^T) - 2 phi diag(diagB) P^T,   W = -1/2 Z P^T,   wd = phi diagB
    kgrad[a] = sum_ij Z_ji dk(x_i, u_j)/da + sum_jj' W_jj' dk(u_j, u_j')/da + sum_i wd_i dk(x_i, x_i)/da

(the clamp in ``lambda`` counts as inactive, the absolute jitter as a constant).  ``v`` is ``dL / dmean`` and ``diagB`` is
``dL / dC_ii``: the layout of ``BasicSolver.loo``, so that ``GP._assemble_grad(v, diagB, kgrad, diag_weight=1.0)`` applies
unchanged.  ``S[a]`` is the sum of the absolute values of the terms of ``kgrad[a]``: the scale a gradient error is measured against.
Kernel gradients come as in ``inducing_ref``: ``route="stacked"`` from one symmetric call on ``[x; u]``, ``route="blocks"`` per
block of ``inducing_ref.BLOCK`` data points.

``dense_model`` is the independent route: the explicit N x N ``C``, ``C^-1`` by LAPACK, ``B = 1/2 (v alpha^T + alpha v^T) -
C^-1 diag(w) C^-1`` formed whole and contracted with ``dC`` differentiated term by term as ``inducing_ref.dense_model`` does.

``tolerances`` is the rule of tests/inducing_cases.py: per quantity (``L, resid, var, lpd, v, diagB, kgrad``) ``1000 x`` the gap
between the two routes on the test's own inputs (the first ``GAP_MAX_N`` points beyond that size), a gap counting as at least
``4 eps``, vectors over their largest entry, the gradient over ``S``; no gap may exceed ``GAP_CAP`` (asserted: an ill-conditioned
problem is replaced, not loosened).  ``defect=`` runs a deliberately wrong gradient (``DEFECTS``;
tests/test_inducing_loo_host.py checks that the bound of the device tests rejects each).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

import inducing_ref
from inducing_cases import EPS, GAP_CAP, GAP_MAX_N
from inducing_ref import BLOCK, PHI, TILE, _two_d, rel
from oracle import solver_np

QUANTITIES = ("L", "resid", "var", "lpd", "v", "diagB", "kgrad")
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# Deliberately wrong gradients.  ``fitc_weight_half`` and ``z_phi_zero`` change nothing under DTC (phi = 0 already).
DEFECTS = ("z_without_v_half",       # Z without its v_J (P alpha)^T half
           "d2_without_s",           # d2 (and diagB, and Z's FITC part with it) without the S_w term
           "fitc_weight_half",       # the FITC diagonal term with weight 1/2 diagB instead of diagB
           "z_phi_zero",             # Z (and W with it) without its FITC part
           "drop_last_tile")         # the rectangular term without its last tile: the last tile row x the last tile column


class InducingLooRef(object):
    """``base`` (the ``InducingRef``), ``c``, ``alpha``, ``L``, ``resid``, ``var``, ``lpd`` and, with ``want_grad``, ``kgrad``,
    ``S`` (P,), ``v``, ``diagB``"""

    def outputs(self):
        """the tuple ``loo_lowrank`` returns with a mask of ones"""
        return self.L, self.resid, self.var, self.lpd, self.kgrad, self.v, self.diagB


def _values(out, c, alpha):
    out.c, out.alpha = c, alpha
    out.resid = alpha / c
    out.var = 1.0 / c
    out.lpd = 0.5 * np.log(c) - 0.5 * alpha * out.resid - HALF_LOG_2PI
    out.L = float(np.sum(out.lpd))
    out.kgrad = out.S = out.v = out.diagB = None
    return 0.5 * (1.0 + alpha * out.resid) / c


def reference(spec, x, yerr, u, jitter, method, r, want_grad=True, route="stacked", defect=None):
    if route not in ("stacked", "blocks") or (defect is not None and defect not in DEFECTS):
        raise ValueError((route, defect))
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    phi = PHI[method]
    base = inducing_ref.reference(spec, x, yerr, u, jitter, method, r=r)
    out = InducingLooRef()
    out.base = base
    D = 1.0 / base.lam
    R = base.H * D[None, :]
    w = _values(out, D - np.sum(base.H * R, axis=0) * D, base.alpha)
    if not want_grad:
        return out
    alpha = base.alpha
    out.v = v = base.solve(out.resid)
    P = cho_solve((base.Lu, True), solver_np.kernel_matrix(spec, x, u).T)       # (m, n)
    Sw = np.dot(R * w[None, :], R.T)
    G1 = np.dot(R, P.T)
    G3 = np.dot(R * (w * D)[None, :], P.T)
    d2 = w * D * D - 2.0 * w * D * np.sum(R * R, axis=0)
    if defect != "d2_without_s":
        d2 = d2 + np.sum(R * np.dot(Sw, R), axis=0)
    out.diagB = diagB = alpha * v - d2
    CWCP = (P * (w * D * D)[None, :]).T - (w * D)[:, None] * np.dot(R.T, G1) - np.dot(R.T, G3) + np.dot(R.T, np.dot(Sw, G1))    # (n, m)
    Zt = np.outer(alpha, np.dot(P, v)) - 2.0 * CWCP
    if defect != "z_without_v_half":
        Zt = Zt + np.outer(v, np.dot(P, alpha))
    if defect != "z_phi_zero":
        Zt = Zt - 2.0 * phi * diagB[:, None] * P.T
    Z = Zt.T
    W = -0.5 * np.dot(Z, P.T)
    wd = phi * (0.5 if defect == "fitc_weight_half" else 1.0) * diagB
    if defect == "drop_last_tile":
        Z = Z.copy()
        Z[TILE * ((m - 1) // TILE):, TILE * ((n - 1) // TILE):] = 0.0
    out.kgrad, out.S = _contract(spec, x, u, Z, W, wd, route)
    return out


def _contract(spec, x, u, Z, W, wd, route):
    """the three terms of ``inducing_ref.reference``'s gradient, each summed over the blocks first, and their absolute sum"""
    n = len(x)
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
    kgrad = (sum(np.einsum("ji,ijp->p", Z[:, s:e], dfu) for s, e, dfu, _ in parts) + np.einsum("jk,jkp->p", W, duu) +
             sum(np.einsum("i,ip->p", wd[s:e], dff) for s, e, _, dff in parts))
    S = (sum(np.einsum("ji,ijp->p", np.abs(Z[:, s:e]), np.abs(dfu)) for s, e, dfu, _ in parts) +
         np.einsum("jk,jkp->p", np.abs(W), np.abs(duu)) +
         sum(np.einsum("i,ip->p", np.abs(wd[s:e]), np.abs(dff)) for s, e, _, dff in parts))
    return kgrad, S


def dense_model(spec, x, yerr, u, jitter, method, r, want_grad=True):
    """The same quantities from the explicit C by LAPACK (an ``InducingLooRef`` without ``S``); ``B`` is kept as ``B``."""
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    phi = PHI[method]
    r = np.asarray(r, dtype=np.float64)
    Kuu = solver_np.kernel_matrix(spec, u) + jitter * np.eye(m)
    Kfu = solver_np.kernel_matrix(spec, x, u)
    P = cho_solve(cho_factor(Kuu, lower=True), Kfu.T)
    Q = np.dot(Kfu, P)
    lam = (np.zeros(n) + yerr) ** 2 + phi * np.maximum(solver_np.kernel_matrix(spec, x, diag=True) - np.diag(Q), 0.0)
    Cm = Q + np.diag(lam)
    Cm = 0.5 * (Cm + Cm.T)
    cf = cho_factor(Cm, lower=True)
    Cinv = cho_solve(cf, np.eye(n))
    Cinv = 0.5 * (Cinv + Cinv.T)
    out = InducingLooRef()
    out.C, out.Cinv = Cm, Cinv
    alpha = cho_solve(cf, r)
    w = _values(out, np.diag(Cinv).copy(), alpha)
    if not want_grad:
        return out
    out.v = v = cho_solve(cf, out.resid)
    out.B = B = 0.5 * (np.outer(v, alpha) + np.outer(alpha, v)) - np.dot(Cinv * w[None, :], Cinv)
    out.diagB = np.diag(B).copy()
    dK = solver_np.kernel_gradient(spec, np.vstack([x, u]))
    dfu, duu, dff = dK[:n, n:], dK[n:, n:], dK[np.arange(n), np.arange(n)]
    g = np.empty(dK.shape[2])
    for a in range(dK.shape[2]):
        dQ = np.dot(dfu[:, :, a], P)
        dQ = dQ + dQ.T - np.dot(P.T, np.dot(duu[:, :, a], P))
        dC = dQ + phi * np.diag(dff[:, a] - np.diag(dQ))
        g[a] = np.sum(B * dC)
    out.kgrad = g
    return out


def _over(err, scale):
    return float(np.max(np.abs(err) / np.maximum(scale, np.finfo(float).tiny), initial=0.0))


def gaps(spec, x, yerr, u, jitter, method, r):
    """What the two float64 routes on the CPU differ by on these inputs, per compared quantity (and ``c``).  Returns
    ``(gaps, restatement, dense)``."""
    ref = reference(spec, x, yerr, u, jitter, method, r)
    d = dense_model(spec, x, yerr, u, jitter, method, r)
    g = dict(L=rel(ref.L, d.L), c=rel(ref.c, d.c), resid=rel(ref.resid, d.resid), var=rel(ref.var, d.var), lpd=rel(ref.lpd, d.lpd),
             v=rel(ref.v, d.v), diagB=rel(ref.diagB, d.diagB), kgrad=_over(ref.kgrad - d.kgrad, ref.S))
    return g, ref, d


def tolerances(spec, x, yerr, u, rel_jitter, method, r, label=""):
    """``(absolute jitter, bound per quantity)`` from the first ``GAP_MAX_N`` points of the test's own inputs"""
    x, u = _two_d(x), _two_d(u)
    jitter = rel_jitter * float(np.mean(solver_np.kernel_matrix(spec, u, diag=True)))
    k = min(len(x), GAP_MAX_N)
    g = gaps(spec, x[:k], (np.zeros(len(x)) + yerr)[:k], u, jitter, method, np.asarray(r, dtype=np.float64)[:k])[0]
    print("gaps", label, len(x), len(u), method, {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return jitter, {key: 1000.0 * max(v, 4 * EPS) for key, v in g.items()}


def check(what, got, want, tol):
    """the seven outputs ``got`` of ``loo_lowrank`` against the restatement ``want``, each printed before it is asserted; without
    a gradient in ``got`` only the values"""
    from inducing_cases import _check
    L, resid, var, lpd, kgrad, v, diagB = got
    _check(what + ": L", L, want.L, tol["L"])
    for name, val in (("resid", resid), ("var", var), ("lpd", lpd)):
        _check(what + ": " + name, val, getattr(want, name), tol[name])
    if kgrad is None:
        assert v is None and diagB is None
        return
    if len(want.kgrad):
        _check(what + ": kgrad", kgrad, want.kgrad, tol["kgrad"], scale=want.S)
    _check(what + ": v", v, want.v, tol["v"])
    _check(what + ": diagB", diagB, want.diagB, tol["diagB"])
