"""CPU reference for leave-group-out cross-validation of a GP, the groupings and the test problems that pin it.

With ``K = k(x, x) + diag(yerr^2)``, ``C = K^-1``, ``alpha = C r`` and groups ``I_1 .. I_G`` that partition the points
(group g has ``m_g`` of them, ``C_gg`` is the block of ``C`` on it):

    resid_g = C_gg^-1 alpha_g = y_g - mu_g,      cov_g = C_gg^-1 (``var`` its diagonal),
    lpd_g   = 1/2 log|C_gg| - 1/2 alpha_g^T C_gg^-1 alpha_g - m_g/2 log 2 pi,      L = sum_g lpd_g,

and with ``u = resid``, ``v = C u``, ``W = blockdiag_g 1/2 (C_gg^-1 + u_g u_g^T)``, ``B = 1/2 (v alpha^T + alpha v^T) - C W C``:

    dL/dtheta_p = sum_ij B_ij dK_ij/dtheta_p,      dL/dK_ii = B_ii (``diagB``),      dL/dmean_i = v_i.

Groups of one point each give tests/loo_ref.py.  The grouping is passed as the C ABI takes it: ``order`` lists the point
indices sorted by group, ``start`` the G + 1 offsets of the groups in it.

``reference()`` evaluates these independently of every HIP path, with the ingredients of ``loo_ref.reference``: ``K`` from
``oracle.solver_np.kernel_matrix``, ``dK`` from ``oracle.kernels_np``, factors / solves / inverses from SciPy
``cho_factor`` / ``cho_solve``, the contraction over the lower triangle in blocks of ``BLOCK`` rows summed in
``np.longdouble``.  ``brute_force()`` does the G explicit refits on the kept points.

Tolerance: the project's one rule (tests/grad_ref.py), ``|x - x_ref| <= C_TOL * U * kappa(K) * S`` with the scales

    resid: max|alpha| max(var)        var, cov: max(var)
    lpd: max_g (1/2 sum_{i in g} |log R_ii^2| + 1/2 |alpha_g|^T |C_gg^-1| |alpha_g|),  R = chol(C_gg);   L: the sum over g
    v: max|v|        diagB: max(|v_i alpha_i| + (|C| W_abs |C|)_ii),      W_abs = blockdiag_g 1/2 (|C_gg^-1| + |u_g| |u_g|^T)
    gradient: S_p = sum_ij (|v_i alpha_j| + (|C| W_abs |C|)_ij) D_ij,p     (D as in grad_ref.py).

The first power of ``kappa`` throughout, as ``loo_ref`` argues for these test problems.

``defect=`` runs a deliberately wrong version (tests/test_lgo_reference.py checks that the rule rejects each).
Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from grad_ref import U, C_TOL, BLOCK, Ref, leaf_blocks, _as_2d
from loo_ref import HALF_LOG_2PI, PAD, KERNELS, problem, _refined_solve       # noqa: F401  (the problems are loo_ref's)
from oracle import kernels_np, solver_np

SLOT = 128               # the device form packs whole consecutive groups into slots of this many positions
MAX_GROUP = 128          # ... and takes groups up to this size

DEFECTS = ("cross_group_entries_kept", "u_outer_dropped", "logdet_sign", "order_not_undone", "last_group_dropped",
           "padded_rows_in_L")
GROUPINGS = ("singletons", "blk7", "blk64", "blk128", "one", "random", "ragged", "labels")


class LgoRef(object):
    """What ``reference()`` returns: ``L``, ``lpd`` (G,), ``resid``, ``var``, ``v``, ``diagB`` (N,), ``cov`` (list of G
    blocks), ``g``, ``S`` (P,), ``alpha``, ``Kinv``, ``kappa`` and the scales ``S_resid``, ``S_var``, ``S_cov``, ``S_lpd``,
    ``S_L``, ``S_v``, ``S_diagB`` (the largest entry of ``mag_diagB``, the per-point magnitude)."""

    def tol(self, what):
        return C_TOL * U * self.kappa * getattr(self, "S" if what == "g" else "S_" + what)

    def ratio(self, what, value):
        """largest |error| / tolerance of quantity ``what`` (<= 1 passes); ``cov``: over all blocks"""
        if what == "cov":
            assert len(value) == len(self.cov)
            return max([Ref._ratio(np.asarray(a, dtype=np.float64) - b, self.tol("cov")) for a, b in zip(value, self.cov)] + [0.0])
        return Ref._ratio(np.asarray(value, dtype=np.float64) - getattr(self, what), self.tol(what))


# ------------------------------------------------------------------------------------ groupings
def order_start(labels):
    """``(order, start)`` of an (n,) array of integer labels: groups numbered by sorted unique label, the points of a group
    in the order they appear in the data."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    _, counts = np.unique(labels, return_counts=True)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def grouping(name, n, seed=0):
    """The (n,) label array of the grouping ``name``, or None where it does not apply (``one`` beyond 128 points)."""
    if name == "singletons":
        return np.arange(n)
    if name in ("blk7", "blk64", "blk128"):
        return np.arange(n) // int(name[3:])
    if name == "one":
        return np.zeros(n, dtype=np.int64) if n <= MAX_GROUP else None
    if name == "random":
        while True:
            labels = np.random.RandomState(seed).randint(0, max(2, n // 40), n)
            if np.max(np.bincount(labels)) <= MAX_GROUP:
                return labels
            seed += 1
    if name == "ragged":
        rng = np.random.RandomState(1000 + n + seed)
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.choice([1, 2, 5, 31, 64, 100, 128])))
        return np.repeat(np.arange(len(sizes)), sizes)[:n]
    if name == "labels":
        blocks = np.arange(n) // 7
        nb = int(blocks[-1]) + 1
        perm = np.random.RandomState(2000 + n + seed).permutation(nb)
        return (3 * perm - nb)[blocks]                    # negative ones, gaps of 3, not monotone in position
    raise ValueError(name)


def slots(start):
    """the device form's packing: lists of consecutive groups whose sizes sum to at most SLOT"""
    out, used = [], SLOT
    for g in range(len(start) - 1):
        m = int(start[g + 1] - start[g])
        if used + m > SLOT:
            out.append([])
            used = 0
        out[-1].append(g)
        used += m
    return out


# ------------------------------------------------------------------------------------ the reference
def reference(kernel, x, yerr, r, order, start, defect=None, block=BLOCK):
    """The leave-group-out reference (module docstring) for ``kernel`` at inputs ``x`` with per-point standard deviations
    ``yerr`` (white noise included), residual ``r = y - mean`` and the groups ``(order, start)``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    order, start = np.asarray(order, dtype=np.int64), np.asarray(start, dtype=np.int64)
    G = len(start) - 1
    P = kernels_np.full_size(kernel)
    groups = [order[start[g]:start[g + 1]] for g in range(G)]
    # the blocks the quantities are formed on: the groups, or (defect) the groups of a slot taken as one
    merged = groups
    if defect == "cross_group_entries_kept":
        merged = [np.concatenate([groups[g] for g in members]) for members in slots(start)]

    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    cf = cho_factor(K, lower=True)
    alpha = _refined_solve(cf, K, r)
    Kinv = cho_solve(cf, np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    absK = np.abs(Kinv)

    resid, var = np.empty(n), np.empty(n)
    Wfull, Wabs = np.zeros((n, n)), np.zeros((n, n))
    cov_at, lpd_at, each_at = {}, np.zeros(len(merged)), np.zeros(len(merged))
    for b, I in enumerate(merged):
        cg = cho_factor(Kinv[np.ix_(I, I)], lower=True)
        cov = cho_solve(cg, np.eye(len(I)))
        cov = 0.5 * (cov + cov.T)
        u = cho_solve(cg, alpha[I])
        resid[I], var[I] = u, np.diag(cov)
        half_logdet = float(np.sum(np.log(np.diag(cg[0]))))
        if defect == "logdet_sign":
            half_logdet = -half_logdet
        lpd_at[b] = half_logdet - 0.5 * float(np.dot(alpha[I], u)) - len(I) * HALF_LOG_2PI
        each_at[b] = float(np.sum(np.abs(np.log(np.diag(cg[0]))))) + 0.5 * float(np.abs(alpha[I]) @ np.abs(cov) @ np.abs(alpha[I]))
        cov_at[b] = cov
        if not (defect == "last_group_dropped" and b == len(merged) - 1):
            Wfull[np.ix_(I, I)] = 0.5 * (cov + (0.0 if defect == "u_outer_dropped" else np.outer(u, u)))
        Wabs[np.ix_(I, I)] = 0.5 * (np.abs(cov) + np.outer(np.abs(u), np.abs(u)))
    if merged is groups:
        lpd, each, covs = lpd_at, each_at, [cov_at[g] for g in range(G)]
    else:
        # the merged block's density booked on its first group, its covariance cut into the groups' diagonal blocks
        lpd, each, covs = np.zeros(G), np.zeros(G), []
        for b, members in enumerate(slots(start)):
            lpd[members[0]], each[members[0]] = lpd_at[b], each_at[b]
            at = 0
            for g in members:
                m = len(groups[g])
                covs.append(cov_at[b][at:at + m, at:at + m])
                at += m
    if defect == "last_group_dropped":
        lpd = lpd.copy()
        lpd[-1] = 0.0
    L = float(np.sum(lpd.astype(np.longdouble)))
    if defect == "padded_rows_in_L":
        L += (-(-n // PAD) * PAD - n) * (-HALF_LOG_2PI)      # identity padding: C = 1, alpha = 0
    v = _refined_solve(cf, K, resid)
    M = np.dot(np.dot(Kinv, Wfull), Kinv)
    M = 0.5 * (M + M.T)
    absM = np.dot(np.dot(absK, Wabs), absK)
    diagB = v * alpha - np.diag(M)

    g = np.zeros(P, dtype=np.longdouble)
    S = np.zeros(P, dtype=np.longdouble)
    blocks = [(a, b) for a, b in leaf_blocks(kernel) if b > 0]
    for s in range(0, n, block):
        e = min(n, s + block)
        Gd = kernels_np.gradient_general(kernel, x[s:e], x[:e])       # rows s..e-1 against columns 0..e-1
        Bm = 0.5 * (np.outer(v[s:e], alpha[:e]) + np.outer(alpha[s:e], v[:e])) - M[s:e, :e]
        Mag = 0.5 * (np.abs(np.outer(v[s:e], alpha[:e])) + np.abs(np.outer(alpha[s:e], v[:e]))) + absM[s:e, :e]
        rows = np.arange(s, e)[:, None]
        cols = np.arange(e)[None, :]
        wt = np.where(cols < rows, 2.0, np.where(cols == rows, 1.0, 0.0))
        if P:
            g += np.sum((Bm * wt)[:, :, None] * Gd, axis=(0, 1), dtype=np.longdouble)
            D = np.abs(Gd)
            for a, b in blocks:
                D[:, :, a:a + b] = np.max(D[:, :, a:a + b], axis=2, keepdims=True)
            S += np.sum((Mag * wt)[:, :, None] * D, axis=(0, 1), dtype=np.longdouble)

    out = LgoRef()
    if defect == "order_not_undone":
        resid, var = resid[order], var[order]
    out.L, out.lpd, out.resid, out.var, out.cov, out.v, out.diagB = L, lpd, resid, var, covs, v, diagB
    out.g = g.astype(np.float64)
    out.S = S.astype(np.float64)
    out.alpha, out.Kinv = alpha, Kinv
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(Kinv, 1))
    out.S_var = out.S_cov = float(np.max(var))
    out.S_resid = float(np.max(np.abs(alpha)) * np.max(var))
    out.S_lpd = float(np.max(each))
    out.S_L = float(np.sum(each))
    out.S_v = float(np.max(np.abs(v)))
    out.mag_diagB = np.abs(v * alpha) + np.diag(absM)
    out.S_diagB = float(np.max(out.mag_diagB))
    return out


def brute_force(kernel, x, yerr, r, order, start):
    """``(L, lpd, resid, var, covs)`` from G explicit refits: ``K`` on the points outside the group factorised afresh, the
    joint prediction of the group's ``r`` from them (noise of the group's points included) and its multivariate-normal log
    density."""
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    G = len(start) - 1
    resid, var, lpd, covs = np.empty(n), np.empty(n), np.empty(G), []
    for g in range(G):
        I = np.asarray(order[start[g]:start[g + 1]])
        keep = np.ones(n, dtype=bool)
        keep[I] = False
        cov, mu = K[np.ix_(I, I)].copy(), np.zeros(len(I))
        if np.any(keep):
            cf = cho_factor(K[np.ix_(keep, keep)], lower=True)
            Ks = K[np.ix_(I, keep)]
            mu = np.dot(Ks, cho_solve(cf, r[keep]))
            cov = cov - np.dot(Ks, cho_solve(cf, Ks.T))
            cov = 0.5 * (cov + cov.T)
        d = r[I] - mu
        cc = cho_factor(cov, lower=True)
        resid[I], var[I] = d, np.diag(cov)
        lpd[g] = -float(np.sum(np.log(np.diag(cc[0])))) - 0.5 * float(np.dot(d, cho_solve(cc, d))) - len(I) * HALF_LOG_2PI
        covs.append(cov)
    return float(np.sum(lpd.astype(np.longdouble))), lpd, resid, var, covs
