"""NumPy restatement of what ``InducingSolver`` adds to DTC and FITC: the variational bound and the gradient with respect to the
inducing inputs (include/george_amd.h, "inducing-point solver"; george_amd/csrc/gh_inducing.hip).  Three objectives: ``"dtc"``,
``"fitc"`` and ``"vfe"`` (DTC's covariance under the bound).  On the factors of ``inducing_ref.reference``, with ``s_i = yerr_i^2``:

    resid_i = max(k(x_i, x_i) - q_i, 0),   tau = sum_i resid_i / s_i   (vfe; else 0),   F = log N(r | 0, C) - 1/2 tau
    omega_i = 0 (dtc), diagA_i (fitc), -1 / s_i (vfe),   diagA_i = alpha_i^2 - (C^-1)_ii  (+ resid_i / s_i^2 under vfe)
    Z = (P alpha) alpha^T - P C^-1 - P diag(omega),   W = -1/2 Z P^T
    kgrad[a]    = sum_ij Z_ji dk(x_i, u_j)/da + sum_jj' W_jj' dk(u_j, u_j')/da + 1/2 sum_i omega_i dk(x_i, x_i)/da
    ugrad[j, :] = sum_i Z_ji d2 k(x_i, u_j) + sum_b (W_jb + W_bj) d1 k(u_j, u_b)

``S`` and ``S_u`` are the same sums over absolute values: the scale an error is measured against.  ``tau`` is a sum of differences
``k(x_i, x_i) - q_i`` that cancel as the inducing inputs fill the domain; its scale is ``tau_scale = sum_i (k(x_i, x_i) + q_i) / s_i``.
``S_u_terms`` is ``S_u`` with the two parts of ``Z``, ``T`` and ``P diag(omega)``, taken by absolute value separately: the scale
where they cancel altogether (one data point under FITC, whose ``C = k(x, x) + s`` does not depend on ``u``).  Input gradients come from
``oracle.kernels_np.x1_gradient_general`` / ``x2_gradient_general``, parameter gradients from ``oracle.solver_np`` as in
tests/inducing_ref.py.  ``dense`` is the second route, from the explicit N x N matrix ``C`` by LAPACK: with
``M = alpha alpha^T - C^-1 - diag(omega)``

    ugrad[j, d] = sum_i d2k(x_i, u_j)_d (P M)_ji - sum_b d1k(u_j, u_b)_d (P M P^T)_jb
    kgrad[a]    = 1/2 sum_ij (alpha alpha^T - C^-1)_ij dQ_ij/da + 1/2 sum_i omega_i (dk(x_i, x_i)/da - dQ_ii/da)

``defect=`` runs a deliberately wrong result (``DEFECTS``; tests/test_inducing_vfe_host.py checks that the bound of the device
tests rejects each one).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

import inducing_ref
from inducing_ref import _two_d, rel
from oracle import kernels_np, solver_np

OBJECTIVES = ("dtc", "fitc", "vfe")
METHOD = {"dtc": "dtc", "fitc": "fitc", "vfe": "dtc"}        # the solver's method; "vfe" is dtc with variational=True
ROW_TILE = 128           # rows of a tile of the device reduction (gh_predgrad.hip PG_ROWS)
STRIP = 256              # data points per strip in the device tests

DEFECTS = ("kuu_dropped",            # ugrad without its K_uu term
           "kuu_w_once",             # .. with W in place of W + W^T
           "d1_for_d2",              # the rectangular term of ugrad with d1 k(x_i, u_j) for d2
           "drop_last_row_tile",     # .. without the last tile of 128 rows
           "drop_last_strip",        # .. without the last strip of 256 data points
           "omega_dropped",          # Z (and W with it) without its omega part: nothing under dtc
           "tau_diaga_dropped")      # diagA without tau's part: nothing but under vfe


class Result(object):
    """``F``, ``tau``, ``tau_scale``, ``logdet`` (log|C|), ``alpha``, ``diagA``, ``kgrad``, ``S``, ``ugrad``, ``S_u``, ``S_u_terms``"""


def _omega(objective, diagA, s):
    return {"dtc": np.zeros_like(s), "fitc": diagA, "vfe": -1.0 / s}[objective]


def model(spec, x, yerr, u, jitter, objective, r, defect=None):
    if objective not in OBJECTIVES or (defect is not None and defect not in DEFECTS):
        raise ValueError((objective, defect))
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    r = np.asarray(r, dtype=np.float64)
    ref = inducing_ref.reference(spec, x, yerr, u, jitter, METHOD[objective], r=r)
    s = (np.zeros(n) + yerr) ** 2
    Kfu = solver_np.kernel_matrix(spec, x, u)
    V = solve_triangular(ref.Lu, Kfu.T, lower=True)
    kd, q = solver_np.kernel_matrix(spec, x, diag=True), np.sum(V * V, axis=0)
    resid = np.maximum(kd - q, 0.0)
    out = Result()
    out.ref = ref
    out.tau_scale = float(np.sum((np.abs(kd) + q) / s))
    out.tau = float(np.sum(resid / s)) if objective == "vfe" else 0.0
    out.logdet = ref.logdet
    out.F = ref.log_likelihood() - 0.5 * out.tau
    out.alpha = ref.alpha
    out.diagA = ref.alpha ** 2 - (1.0 / ref.lam - np.sum(ref.H * ref.H, axis=0) / ref.lam ** 2)
    if objective == "vfe" and defect != "tau_diaga_dropped":
        out.diagA = out.diagA + resid / s ** 2
    omega = _omega(objective, out.diagA, s)
    P = cho_solve((ref.Lu, True), Kfu.T)                                        # (m, n)
    Z = np.outer(np.dot(P, ref.alpha), ref.alpha) - ref.solve(P.T).T
    Zabs = np.abs(Z) + np.abs(P * omega[None, :])
    if defect != "omega_dropped":
        Z = Z - P * omega[None, :]
    W = -0.5 * np.dot(Z, P.T)
    dK = solver_np.kernel_gradient(spec, np.vstack([x, u]))                     # ((n + m), (n + m), P): x first, u behind
    dfu, duu, dff = dK[:n, n:], dK[n:, n:], dK[np.arange(n), np.arange(n)]
    out.kgrad = np.einsum("ji,ijp->p", Z, dfu) + np.einsum("jk,jkp->p", W, duu) + 0.5 * np.einsum("i,ip->p", omega, dff)
    out.S = (np.einsum("ji,ijp->p", np.abs(Z), np.abs(dfu)) + np.einsum("jk,jkp->p", np.abs(W), np.abs(duu)) +
             0.5 * np.einsum("i,ip->p", np.abs(omega), np.abs(dff)))
    d2fu = kernels_np.x2_gradient_general(spec, x, u)                           # (n, m, ndim)
    d1uu = kernels_np.x1_gradient_general(spec, u, u)                           # (m, m, ndim)
    Ws = W + W.T
    out.S_u = np.einsum("ji,ijd->jd", np.abs(Z), np.abs(d2fu)) + np.einsum("jb,jbd->jd", np.abs(Ws), np.abs(d1uu))
    Wabs = 0.5 * np.dot(Zabs, np.abs(P.T))
    out.S_u_terms = np.einsum("ji,ijd->jd", Zabs, np.abs(d2fu)) + np.einsum("jb,jbd->jd", Wabs + Wabs.T, np.abs(d1uu))
    Zr = Z.copy()
    if defect == "drop_last_row_tile":
        Zr[:, ROW_TILE * ((n - 1) // ROW_TILE):] = 0.0
    if defect == "drop_last_strip":
        Zr[:, STRIP * ((n - 1) // STRIP):] = 0.0
    if defect == "d1_for_d2":
        d2fu = kernels_np.x1_gradient_general(spec, x, u)
    if defect == "kuu_dropped":
        Ws = np.zeros_like(Ws)
    if defect == "kuu_w_once":
        Ws = W
    out.ugrad = np.einsum("ji,ijd->jd", Zr, d2fu) + np.einsum("jb,jbd->jd", Ws, d1uu)
    return out


def dense(spec, x, yerr, u, jitter, objective, r):
    """The same quantities from the explicit C by LAPACK (no ``S``, ``S_u``)."""
    x, u = _two_d(x), _two_d(u)
    n, m = len(x), len(u)
    r = np.asarray(r, dtype=np.float64)
    s = (np.zeros(n) + yerr) ** 2
    Kuu = solver_np.kernel_matrix(spec, u) + jitter * np.eye(m)
    Kfu = solver_np.kernel_matrix(spec, x, u)
    P = cho_solve(cho_factor(Kuu, lower=True), Kfu.T)
    Q = np.dot(Kfu, P)
    resid = np.maximum(solver_np.kernel_matrix(spec, x, diag=True) - np.diag(Q), 0.0)
    lam = s + (resid if objective == "fitc" else 0.0)
    cf = cho_factor(Q + np.diag(lam), lower=True)
    Cinv = cho_solve(cf, np.eye(n))
    out = Result()
    out.alpha = cho_solve(cf, r)
    out.tau = float(np.sum(resid / s)) if objective == "vfe" else 0.0
    out.logdet = 2.0 * np.sum(np.log(np.diag(cf[0])))
    out.F = -0.5 * (np.dot(r, out.alpha) + out.logdet + n * np.log(2.0 * np.pi)) - 0.5 * out.tau
    Am = np.outer(out.alpha, out.alpha) - Cinv
    out.diagA = np.diag(Am) + (resid / s ** 2 if objective == "vfe" else 0.0)
    omega = _omega(objective, out.diagA, s)
    dK = solver_np.kernel_gradient(spec, np.vstack([x, u]))
    dfu, duu, dff = dK[:n, n:], dK[n:, n:], dK[np.arange(n), np.arange(n)]
    out.kgrad = np.empty(dK.shape[2])
    for a in range(dK.shape[2]):
        dQ = np.dot(dfu[:, :, a], P)
        dQ = dQ + dQ.T - np.dot(P.T, np.dot(duu[:, :, a], P))
        out.kgrad[a] = 0.5 * np.sum(Am * dQ) + 0.5 * np.sum(omega * (dff[:, a] - np.diag(dQ)))
    PM = np.dot(P, Am - np.diag(omega))
    out.ugrad = (np.einsum("ijd,ji->jd", kernels_np.x2_gradient_general(spec, x, u), PM) -
                 np.einsum("jbd,jb->jd", kernels_np.x1_gradient_general(spec, u, u), np.dot(PM, P.T)))
    return out


def over(err, scale):
    """largest |err| over ``scale``, element by element; entries whose scale is 0 must be exactly 0"""
    err, scale = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(scale, dtype=np.float64)
    assert np.all(err[scale == 0.0] == 0.0)
    return float(np.max(err[scale > 0.0] / scale[scale > 0.0], initial=0.0))


def gaps(spec, x, yerr, u, jitter, objective, r):
    """What the two routes differ by on the same inputs, per compared quantity: ``(gaps, model)``.  ``ll`` is ``F``; ``logdet``
    is ``log|C| + tau``, what the solver's ``log_determinant`` returns; ``tau`` over ``tau_scale``."""
    a, d = model(spec, x, yerr, u, jitter, objective, r), dense(spec, x, yerr, u, jitter, objective, r)
    g = dict(ll=rel(a.F, d.F), logdet=rel(a.logdet + a.tau, d.logdet + d.tau), tau=abs(a.tau - d.tau) / a.tau_scale,
             alpha=rel(a.alpha, d.alpha), diagA=rel(a.diagA, d.diagA), kgrad=over(a.kgrad - d.kgrad, a.S), ugrad=over(a.ugrad - d.ugrad, a.S_u))
    return g, a
