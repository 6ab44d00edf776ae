"""CPU reference for the gradient of the GP log-likelihood, and the test problems that pin it.

The kernel part of ``GP.grad_log_likelihood`` (reference ``gp.py:429-466``) is

    g_p = 1/2 sum_ij A_ij dK_ij/dtheta_p,      A = alpha alpha^T - K^-1,  alpha = K^-1 r.

``reference()`` evaluates it independently of every HIP path: ``K`` comes from
``oracle.solver_np.kernel_matrix`` (the compiled reference evaluator where ``oracle/_ref`` was
built, the NumPy port otherwise), ``dK`` from ``oracle.kernels_np``, the factor, ``alpha`` and
``K^-1`` from fp64 LAPACK (SciPy ``cho_factor`` / ``cho_solve``).  The contraction runs over the
lower triangle in blocks of at most ``BLOCK`` rows -- the (N, N, P) tensor is never formed -- with
the same weights as the device reduction (off-diagonal 1, diagonal 1/2), summed in
``np.longdouble``.

One tolerance rule covers every comparison: ``|x - x_ref| <= C_TOL * U * kappa(K) * S`` where
``kappa`` is the 1-norm condition number ``||K||_1 ||K^-1||_1`` and ``S`` is the matching absolute
scale: ``max|alpha|`` for alpha, ``max(alpha_i^2 + |K^-1_ii|)`` for diag(A), and for the gradient

    S_p = 1/2 sum_ij (|alpha_i alpha_j| + |K^-1_ij|) D_ij,p,    D_ij,p = max_{q in leaf(p)} |dK_ij/dtheta_q|.

Both magnitudes are those of the operands rather than of the result.  ``A_ij`` is a difference, and
a correct fp64 evaluation of it carries an error of about ``u (|alpha_i alpha_j| + |K^-1_ij|)``
however small ``A_ij`` is.  The derivatives of one leaf share intermediates (the back-substituted
difference vector of a general metric, for one), so each is off by about ``u`` times the largest of
them, however small it is itself.  At N = 2 a single term makes up each ``g_p``, and both effects
showed on the device at a few times the ``|A_ij| |dK_ij|`` scale.

``defect=`` runs a deliberately wrong version of the reference (tests/test_grad_reference.py
checks that the tolerance rejects each one).  Test helper only: not a conftest.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import kernels_np, solver_np

U = 2.0 ** -53           # unit round-off of fp64
C_TOL = 32               # the one constant of the tolerance rule
BLOCK = 256              # rows per block of the contraction
TILE = 64                # edge of a tile of the device reduction (gh_kmat.hip KT)

DEFECTS = ("diag_weight_one", "drop_offdiag_tile", "drop_last_row", "swap_first_pair", "swap_last_pair",
           "product_wrong_operand")


class Ref(object):
    """What ``reference()`` returns: ``g``, ``S`` (P,), ``alpha``, ``diagA`` (N,), ``Kinv`` (N, N), ``logdet``,
    ``quad``, ``kappa`` and the scales of the scalar results ``S_logdet``, ``S_quad``."""

    def tol_grad(self):
        return C_TOL * U * self.kappa * self.S

    def tol_alpha(self):
        return C_TOL * U * self.kappa * np.max(np.abs(self.alpha))

    def tol_diagA(self):
        return C_TOL * U * self.kappa * np.max(self.alpha ** 2 + np.abs(np.diag(self.Kinv)))

    def tol_logdet(self):
        return C_TOL * U * self.kappa * self.S_logdet

    def tol_quad(self):
        return C_TOL * U * self.kappa * self.S_quad

    # largest |error| / tolerance of each quantity (<= 1 passes; a zero scale asks for an exact match)
    @staticmethod
    def _ratio(err, tol):
        err, tol = np.abs(np.asarray(err, dtype=np.float64)), np.asarray(tol, dtype=np.float64) + np.zeros(np.shape(err))
        if err.size == 0:
            return 0.0
        q = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err == 0, 0.0, np.inf))
        return float(np.max(q))

    def ratio_grad(self, g):
        return self._ratio(np.asarray(g) - self.g, self.tol_grad())

    def ratio_alpha(self, alpha):
        return self._ratio(np.asarray(alpha) - self.alpha, self.tol_alpha())

    def ratio_diagA(self, diagA):
        return self._ratio(np.asarray(diagA) - self.diagA, self.tol_diagA())

    def ratio_logdet(self, logdet):
        return self._ratio(logdet - self.logdet, self.tol_logdet())

    def ratio_quad(self, quad):
        return self._ratio(quad - self.quad, self.tol_quad())


def _as_2d(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return x[:, None] if x.ndim == 1 else x


def _grad_wrong_product(spec, x1, x2):
    """(value, grad (n1, n2, P)) with the product rule applied to the WRONG operand's value
    (d(ab) = a'a + b'b): the defect ``product_wrong_operand``."""
    if bool(spec.is_kernel):
        return kernels_np.value_general(spec, x1, x2), kernels_np.gradient_general(spec, x1, x2)
    va, ga = _grad_wrong_product(spec.k1, x1, x2)
    vb, gb = _grad_wrong_product(spec.k2, x1, x2)
    if int(spec.operator_type) == 0:
        return va + vb, np.concatenate([ga, gb], axis=2)
    return va * vb, np.concatenate([ga * va[:, :, None], gb * vb[:, :, None]], axis=2)


def leaf_blocks(spec):
    """(start, size) of each leaf's parameters in the full vector, in order."""
    if bool(spec.is_kernel):
        return [(0, kernels_np.full_size(spec))]
    left = leaf_blocks(spec.k1)
    off = kernels_np.full_size(spec.k1)
    return left + [(off + a, b) for a, b in leaf_blocks(spec.k2)]


def reference(kernel, x, yerr, r, defect=None, block=BLOCK):
    """The gradient reference (see the module docstring) for ``kernel`` at inputs ``x`` with per-point standard
    deviations ``yerr`` (white noise included) and residual ``r``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    x = _as_2d(x)
    n = len(x)
    yerr = np.zeros(n) + np.asarray(yerr, dtype=np.float64)
    r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
    P = kernels_np.full_size(kernel)

    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(n)] += yerr ** 2
    cf = cho_factor(K, lower=True)
    alpha = cho_solve(cf, r)
    # one step of refinement on a residual formed in extended precision (K itself is taken as exact)
    res = r.astype(np.longdouble) - np.dot(K.astype(np.longdouble), alpha.astype(np.longdouble))
    alpha = (alpha + cho_solve(cf, res.astype(np.float64)))
    Kinv = cho_solve(cf, np.eye(n))

    g = np.zeros(P, dtype=np.longdouble)
    S = np.zeros(P, dtype=np.longdouble)
    diagA = alpha * alpha - np.diag(Kinv)
    blocks = [(a, b) for a, b in leaf_blocks(kernel) if b > 0]
    for s in range(0, n, block):
        e = min(n, s + block)
        # rows s..e-1 against columns 0..e-1: the lower triangle of the block row
        if defect == "product_wrong_operand":
            G = _grad_wrong_product(kernel, x[s:e], x[:e])[1]
        else:
            G = kernels_np.gradient_general(kernel, x[s:e], x[:e])
        W = np.outer(alpha[s:e], alpha[:e]) - Kinv[s:e, :e]
        M = np.abs(np.outer(alpha[s:e], alpha[:e])) + np.abs(Kinv[s:e, :e])
        rows = np.arange(s, e)[:, None]
        cols = np.arange(e)[None, :]
        W = np.where(cols < rows, W, 0.0)
        M = np.where(cols < rows, M, 0.0)
        W[np.arange(e - s), np.arange(s, e)] = diagA[s:e] * (1.0 if defect == "diag_weight_one" else 0.5)
        M[np.arange(e - s), np.arange(s, e)] = 0.5 * (alpha[s:e] ** 2 + np.abs(np.diag(Kinv)[s:e]))
        if defect == "drop_offdiag_tile":
            W = np.where((rows >= TILE) & (rows < 2 * TILE) & (cols < TILE), 0.0, W)
        if defect == "drop_last_row":
            W = np.where(rows == n - 1, 0.0, W)
        if P:
            g += np.sum(W[:, :, None] * G, axis=(0, 1), dtype=np.longdouble)
            D = np.abs(G)
            for a, b in blocks:
                D[:, :, a:a + b] = np.max(D[:, :, a:a + b], axis=2, keepdims=True)
            S += np.sum(M[:, :, None] * D, axis=(0, 1), dtype=np.longdouble)
    g = g.astype(np.float64)
    if defect == "swap_first_pair" and P >= 2:
        g[[0, 1]] = g[[1, 0]]
    if defect == "swap_last_pair" and P >= 2:
        g[[P - 2, P - 1]] = g[[P - 1, P - 2]]

    out = Ref()
    out.g = g
    out.S = S.astype(np.float64)
    out.alpha = alpha
    out.diagA = diagA
    out.logdet = float(2.0 * np.sum(np.log(np.diag(cf[0]))))
    out.quad = float(np.dot(r, alpha))
    out.kappa = float(np.linalg.norm(K, 1) * np.linalg.norm(Kinv, 1))
    out.S_logdet = float(np.sum(np.abs(Kinv) * np.abs(K)))
    aa = np.abs(alpha)
    out.S_quad = float(aa @ (np.abs(K) @ aa) + np.abs(r) @ aa)
    out.Kinv = Kinv
    return out


# ------------------------------------------------------------------------------------ test problems
# Kernels of the parameter-count matrix: P -> (builder(K), input dimension).  The device reduction has three
# instances, chosen by P: kgrad_reduce_kernel<4> (P <= 4), <16> (5..16) and <64> (17..64).
def _spd(n, seed, scale):
    rng = np.random.RandomState(seed)
    L = rng.randn(n, n) * 0.3
    L[np.diag_indices(n)] = 1.0 + 0.2 * rng.rand(n)
    L = np.tril(L)
    return scale * np.dot(L, L.T)


def kernel_p1(K):
    return K.PolynomialKernel(order=2, log_sigma2=-0.5)


def kernel_p4(K):
    return K.ConstantKernel(log_constant=np.log(0.8), ndim=3) * K.Matern32Kernel([0.6, 1.4, 2.5], ndim=3)


def kernel_p5(K):
    # a product of sums
    return ((K.ConstantKernel(log_constant=np.log(0.3), ndim=2) + K.ExpSquaredKernel([0.8, 1.7], ndim=2))
            * K.RationalQuadraticKernel(log_alpha=np.log(1.5), metric=0.9, ndim=2, axes=1))


def kernel_p16(K):
    return (K.ConstantKernel(log_constant=np.log(0.9), ndim=4) * K.ExpSquaredKernel(_spd(4, 11, 1.5), ndim=4)
            * (K.ConstantKernel(log_constant=np.log(0.4), ndim=4) + K.Matern52Kernel([1.0, 2.0, 0.7, 3.0], ndim=4)))


def kernel_p17(K):
    return kernel_p16(K) + K.CosineKernel(log_period=1.3, ndim=4, axes=2)


def _amp(K, value):
    # a plain ``value * k`` over 16 dimensions would build a 16-axis ConstantKernel (more than 8 active axes)
    return K.ConstantKernel(log_constant=np.log(value), ndim=16, axes=0)


def kernel_p37(K):
    return _amp(K, 0.7) * K.ExpSquaredKernel(_spd(8, 21, 2.0), ndim=16, axes=list(range(8)))


def kernel_p64(K):
    return (kernel_p37(K)
            + _amp(K, 0.3) * K.Matern32Kernel(_spd(5, 23, 1.2), ndim=16, axes=list(range(8, 13)))
            + _amp(K, 0.2) * K.Matern52Kernel([0.5, 0.8, 1.1, 1.4, 1.7, 2.0, 2.3, 2.6], ndim=16, axes=list(range(8, 16)))
            + K.ExpKernel(1.5, ndim=16, axes=3)
            + K.ExpKernel(0.6, ndim=16, axes=12))


PCASES = {1: (kernel_p1, 1), 4: (kernel_p4, 3), 5: (kernel_p5, 2), 16: (kernel_p16, 4), 17: (kernel_p17, 4),
          37: (kernel_p37, 16), 64: (kernel_p64, 16)}


def instance(P):
    """The ``PMAX`` of the device reduction a kernel with ``P`` parameters runs on (gh_launch_kgrad_reduce)."""
    return 4 if P <= 4 else 16 if P <= 16 else 64


def problem(P, n, seed=0):
    """(kernel, x, yerr, r) of the matrix cell (P, n).  The noise grows with n so that kappa(K) <= 1e6 up to n = 4097."""
    build, ndim = PCASES[P]
    kernel = build(_kernels())
    rng = np.random.RandomState(1000 * P + n + seed)
    if ndim == 1:
        x = np.sort(rng.uniform(-1.0, 1.0, n))[:, None]
    else:
        x = rng.uniform(0.0, 2.0, (n, ndim))
        x = x[np.argsort(x[:, 0])]
    yerr = (0.1 + 0.05 * rng.rand(n)) * max(1.0, np.sqrt(n / 300.0))
    r = np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n)
    return kernel, x, yerr, r


def _kernels():
    from george_amd import kernels
    return kernels


def deep_kernel(K, depth):
    """A right-nested expression over 16 dimensions whose postfix program holds ``depth`` operands at once:
    k1 op (k2 op (... (k_{depth-1} op k_depth))), alternating products and sums."""
    leaves = [
        lambda: K.ExpSquaredKernel([0.9, 1.6], ndim=16, axes=[0, 5]),
        lambda: K.ConstantKernel(log_constant=np.log(0.6), ndim=16, axes=15),
        lambda: K.Matern32Kernel(_spd(3, 31, 1.3), ndim=16, axes=[1, 9, 14]),
        lambda: K.CosineKernel(log_period=0.8, ndim=16, axes=7),
        lambda: K.RationalQuadraticKernel(log_alpha=np.log(0.7), metric=1.1, ndim=16, axes=[2, 3, 11]),
        lambda: K.ExpSine2Kernel(gamma=0.5, log_period=0.4, ndim=16, axes=13),
        lambda: K.Matern52Kernel([0.8, 1.2, 2.1, 0.5], ndim=16, axes=[4, 6, 8, 10]),
        lambda: K.LocalGaussianKernel(location=0.9, log_width=0.3, ndim=16, axes=12),
        lambda: K.ExpKernel(2.2, ndim=16, axes=[0, 1]),
    ]
    k = leaves[depth - 1]()
    for i in range(depth - 2, -1, -1):
        a = leaves[i]()
        k = a * k if i % 2 == 0 else a + k
    return k
