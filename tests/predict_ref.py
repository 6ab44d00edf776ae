"""CPU reference for batched posterior predictions (GP.predict_batch), and the tolerance rule that pins them.

For member b, with K = K_b(x, x) + diag(sigma_b^2), K* = K_b(xs, x), K** = K_b(xs, xs) (no white noise, as
``predict``), the prediction of reference ``gp.py:482-545`` is

    mu  = K* K^-1 r + mean(xs),       cov = K** - K* K^-1 K*^T,       var = diag(cov).

``reference()`` evaluates one member independently of every HIP path: K, K* and K** come from
``oracle.solver_np.kernel_matrix`` (the compiled reference evaluator where ``oracle/_ref`` was built, the NumPy port
otherwise), the linear algebra from fp64 LAPACK (SciPy ``cho_factor`` / ``cho_solve``), with alpha = K^-1 r refined once
on a residual formed in extended precision.

One tolerance rule covers every comparison: ``|x - x_ref| <= C_TOL * U * kappa(K) * S`` with ``kappa`` the 1-norm
condition number of K and ``S`` an operand-magnitude scale:

    S_mu_c   = sum_i |K*_ci| |alpha_i| + |mean_c|,
    S_cov_cd = |K**_cd| + sum_i |V_ic| |V_id|,          V = L^-1 K*^T    (S_var_c = S_cov_cc).

Both results are differences (mean of a cancelling sum, K** minus a Gram matrix), so their error follows the operands,
not the result.  ``defect=`` runs a deliberately wrong version (tests/test_predict_reference.py checks that the rule
rejects each one).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from oracle import solver_np

U = 2.0 ** -53           # unit round-off of fp64
C_TOL = 32               # the one constant of the tolerance rule
DEFECTS = ("drop_yerr", "white_noise_in_kss", "drop_last_test_row", "swap_members", "mean_at_x")


class PRef(object):
    """One member's reference: ``mu`` (M,), ``cov`` (M, M), ``var`` (M,), their scales ``S_mu``, ``S_cov`` and
    ``kappa``."""

    def tol_mu(self):
        return C_TOL * U * self.kappa * self.S_mu

    def tol_cov(self):
        return C_TOL * U * self.kappa * self.S_cov

    def tol_var(self):
        return C_TOL * U * self.kappa * np.diag(self.S_cov)

    # largest |error| / tolerance (<= 1 passes; a zero scale asks for an exact match)
    @staticmethod
    def _ratio(err, tol):
        err = np.abs(np.asarray(err, dtype=np.float64))
        tol = np.asarray(tol, dtype=np.float64) + np.zeros(np.shape(err))
        if err.size == 0:
            return 0.0
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        return float(np.max(q))

    def ratio_mu(self, mu):
        return self._ratio(np.asarray(mu) - self.mu, self.tol_mu())

    def ratio_var(self, var):
        return self._ratio(np.asarray(var) - self.var, self.tol_var())

    def ratio_cov(self, cov):
        return self._ratio(np.asarray(cov) - self.cov, self.tol_cov())


def _as_2d(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def reference(kernel, x, sigma, r, xs, mean_t=0.0, white_noise=None, defect=None):
    """One member (see the module docstring): ``kernel`` at its current parameters, points ``x`` with standard deviations
    ``sigma`` (white noise included), residual ``r``, test points ``xs`` and the mean model there, ``mean_t``.
    ``white_noise`` (the member's white-noise variance) is only used by the defect ``white_noise_in_kss``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x, xs = _as_2d(x), _as_2d(xs)
    n, m = len(x), len(xs)
    sigma = np.zeros(n) + np.asarray(sigma, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    mean_t = np.zeros(m) + np.asarray(mean_t, dtype=np.float64)

    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    if defect != "drop_yerr":
        K[np.diag_indices(n)] += sigma ** 2
    Ks = np.array(solver_np.kernel_matrix(kernel, xs, x), dtype=np.float64).reshape(m, n)
    if defect == "drop_last_test_row":
        Ks[-1] = 0.0
    Kss = np.array(solver_np.kernel_matrix(kernel, xs), dtype=np.float64).reshape(m, m)
    if defect == "white_noise_in_kss":
        Kss[np.diag_indices(m)] += white_noise
    cf = cho_factor(K, lower=True)
    alpha = cho_solve(cf, r)
    res = r.astype(np.longdouble) - np.dot(K.astype(np.longdouble), alpha.astype(np.longdouble))
    alpha = alpha + cho_solve(cf, res.astype(np.float64))
    L = np.tril(cf[0])
    V = solve_triangular(L, Ks.T, lower=True)
    Kinv = cho_solve(cf, np.eye(n))

    out = PRef()
    out.mu = Ks @ alpha + mean_t
    out.cov = Kss - V.T @ V
    out.cov = 0.5 * (out.cov + out.cov.T)
    out.var = np.diag(out.cov).copy()
    out.S_mu = np.abs(Ks) @ np.abs(alpha) + np.abs(mean_t)
    out.S_cov = np.abs(Kss) + np.abs(V).T @ np.abs(V)
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(Kinv, 1))
    return out


def member_inputs(gp, vectors, y, xs):
    """Per member, by the one-vector path (``set_parameter_vector`` and the GP's own model calls; the GP is restored):
    (full kernel parameter vector, sigma (N,), residual (N,), mean at xs (M,), mean at x (N,), white-noise variance)."""
    v0 = gp.get_parameter_vector()
    out = []
    try:
        for v in vectors:
            gp.set_parameter_vector(v)
            wn = np.exp(gp._call_white_noise(gp._x))
            out.append((gp.kernel.get_parameter_vector(include_frozen=True), np.sqrt(gp._yerr2 + wn),
                        np.asarray(y, dtype=np.float64) - gp._call_mean(gp._x), gp._call_mean(xs), gp._call_mean(gp._x),
                        float(wn[0])))
    finally:
        gp.set_parameter_vector(v0)
    return out


def batch_reference(gp, vectors, y, xs, members=None, defect=None):
    """``{b: PRef}`` for the members ``members`` (all by default) of ``gp.predict_batch(vectors, y, xs)``."""
    xs = _as_2d(xs)
    inputs = member_inputs(gp, vectors, y, xs)
    if defect == "swap_members":
        inputs[0], inputs[1] = inputs[1], inputs[0]
    k = gp.kernel
    saved = k.get_parameter_vector(include_frozen=True)
    out = {}
    try:
        for b in (range(len(vectors)) if members is None else members):
            kp, sigma, r, mean_t, mean_x, wn = inputs[b]
            if defect == "mean_at_x":
                assert len(mean_x) == len(mean_t)
                mean_t = mean_x
            k.set_parameter_vector(kp, include_frozen=True)
            out[b] = reference(k, gp._x, sigma, r, xs, mean_t, white_noise=wn,
                               defect=None if defect in ("swap_members", "mean_at_x") else defect)
    finally:
        k.set_parameter_vector(saved, include_frozen=True)
    return out
