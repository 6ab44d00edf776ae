"""CPU reference for the input derivatives of the prediction (GP.predict_gradient), and the tolerance rule that pins them.

With K = K(x, x) + diag(sigma^2), alpha = K^-1 r, k_c = K(x, t_c), w_c = K^-1 k_c, G_cid = d k(t_c, x_i) / d t_cd (the
x1-gradient) and D_cd = [x1-gradient + x2-gradient]_d of k at (t_c, t_c):

    dmu_cd  = sum_i G_cid alpha_i + d mean / d t_cd,          dvar_cd = D_cd - 2 sum_i G_cid w_ic.

``reference()`` evaluates this independently of every HIP path, on the linear algebra of ``predict_ref.reference``: K from
``oracle.solver_np.kernel_matrix``, SciPy ``cho_factor`` / ``cho_solve``, alpha (and the columns w_c) refined once on a residual
formed in extended precision, ``kappa`` the 1-norm condition number of K.  G and D come from
``oracle.kernels_np.x1_gradient_general`` / ``x2_gradient_general``.  ``mu`` and ``var`` (with their own scales) are those of
``predict_ref.reference``, in ``.pred``.

The project's one tolerance rule, ``|x - x_ref| <= C_TOL * U * kappa * S``, with the scales in norm form, because the solver's
error in alpha and w_c is norm-wise (||d alpha|| <= c u kappa ||alpha||, spread over the entries in no particular way):

    S_dmu_cd  = ||G_c.d||_2 ||alpha||_2 + |dmean_cd|,         S_dvar_cd = |D_cd| + 2 ||G_c.d||_2 ||w_c||_2.

``defect=`` runs a deliberately wrong version (tests/test_predict_gradient_reference.py checks that the rule rejects each one
wherever it changes the result).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

import predict_ref
from predict_ref import C_TOL, U
from oracle import kernels_np, solver_np

DEFECTS = ("drop_factor_2", "drop_diag_term", "x2_for_x1", "drop_last_train_row", "drop_last_test_row", "swap_dims")


class GRef(object):
    """``dmu``, ``dvar`` (M, ndim), their scales ``S_dmu``, ``S_dvar``, ``kappa``; the pieces ``G`` (M, N, ndim), ``D`` (M, ndim),
    ``alpha`` (N,), ``W`` (N, M); ``pred``: the ``predict_ref.PRef`` of the same problem (mu, var)."""

    _ratio = staticmethod(predict_ref.PRef._ratio)

    def tol_dmu(self):
        return C_TOL * U * self.kappa * self.S_dmu

    def tol_dvar(self):
        return C_TOL * U * self.kappa * self.S_dvar

    # largest |error| / tolerance (<= 1 passes)
    def ratio_dmu(self, dmu):
        return self._ratio(np.asarray(dmu) - self.dmu, self.tol_dmu())

    def ratio_dvar(self, dvar):
        return self._ratio(np.asarray(dvar) - self.dvar, self.tol_dvar())


def _refined_solve(cf, K, b):
    s = cho_solve(cf, b)
    res = b.astype(np.longdouble) - np.dot(K.astype(np.longdouble), s.astype(np.longdouble))
    return s + cho_solve(cf, res.astype(np.float64))


def gradients(kernel, xs, x):
    """(G (M, N, ndim), D (M, ndim)) from the oracle's evaluator"""
    G = kernels_np.x1_gradient_general(kernel, xs, x)
    idx = np.arange(len(xs))
    D = kernels_np.x1_gradient_general(kernel, xs, xs)[idx, idx] + kernels_np.x2_gradient_general(kernel, xs, xs)[idx, idx]
    return G, D


def reference(kernel, x, sigma, r, xs, mean_t=0.0, dmean_t=0.0, defect=None):
    """``kernel`` at its current parameters, points ``x`` with standard deviations ``sigma`` (white noise included), residual
    ``r``, test points ``xs``, the mean model there (``mean_t``) and its input derivative (``dmean_t``, (M, ndim) or a scalar)."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x, xs = predict_ref._as_2d(x), predict_ref._as_2d(xs)
    n, m, nd = len(x), len(xs), x.shape[1]
    sigma = np.zeros(n) + np.asarray(sigma, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    dmean_t = np.zeros((m, nd)) + np.asarray(dmean_t, dtype=np.float64)

    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += sigma ** 2
    Ks = np.array(solver_np.kernel_matrix(kernel, xs, x), dtype=np.float64).reshape(m, n)
    cf = cho_factor(K, lower=True)
    alpha = _refined_solve(cf, K, r)
    W = _refined_solve(cf, K, np.ascontiguousarray(Ks.T))
    Kinv = cho_solve(cf, np.eye(n))

    G, D = gradients(kernel, xs, x)
    if defect == "x2_for_x1":
        G = kernels_np.x2_gradient_general(kernel, xs, x)
    if defect == "drop_last_train_row":
        G = G.copy()
        G[:, -1, :] = 0.0
    if defect == "drop_last_test_row":
        G, D = G.copy(), D.copy()
        G[-1], D[-1] = 0.0, 0.0
    if defect == "swap_dims":
        G, D = np.ascontiguousarray(G[:, :, ::-1]), np.ascontiguousarray(D[:, ::-1])
    if defect == "drop_diag_term":
        D = np.zeros_like(D)

    out = GRef()
    out.G, out.D, out.alpha, out.W = G, D, alpha, W
    out.dmu = np.einsum("cid,i->cd", G, alpha) + dmean_t
    out.dvar = D - (1.0 if defect == "drop_factor_2" else 2.0) * np.einsum("cid,ic->cd", G, W)
    gn = np.sqrt(np.sum(G * G, axis=1))                                      # ||G_c.d||_2, (M, ndim)
    out.S_dmu = gn * np.linalg.norm(alpha) + np.abs(dmean_t)
    out.S_dvar = np.abs(D) + 2.0 * gn * np.linalg.norm(W, axis=0)[:, None]
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(Kinv, 1))
    out.pred = predict_ref.reference(kernel, x, sigma, r, xs, mean_t)
    return out
