"""The prediction reference of tests/predict_ref.py, checked on the CPU: its accuracy against a 50-digit evaluation and
the power of its tolerance rule to reject a wrong prediction.  (No GPU needed.)"""
import functools

import mpmath
import numpy as np
import pytest

import predict_ref as R
from george_amd import GP, kernels as K
from george_amd.modeling import Model
from oracle import solver_np


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


# ------------------------------------------------------------------ accuracy against mpmath
def _mp_predict(kernel, x, sigma, r, xs, mean_t):
    """mu and cov from the same fp64 K, K*, K** with the Cholesky factor and both solves in 50-digit arithmetic"""
    mp = mpmath.mp
    n, m = len(x), len(xs)
    Kf = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    Kf[np.diag_indices(n)] += sigma ** 2
    Ks = np.array(solver_np.kernel_matrix(kernel, xs, x), dtype=np.float64).reshape(m, n)
    Kss = np.array(solver_np.kernel_matrix(kernel, xs), dtype=np.float64).reshape(m, m)
    with mpmath.workdps(50):
        Km = [[mp.mpf(float(Kf[i, j])) for j in range(n)] for i in range(n)]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            L[j][j] = mp.sqrt(Km[j][j] - mp.fsum(L[j][k] ** 2 for k in range(j)))
            for i in range(j + 1, n):
                L[i][j] = (Km[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]

        def fwd(b):
            z = []
            for i in range(n):
                z.append((b[i] - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i])
            return z

        z = fwd([mp.mpf(float(v)) for v in r])
        V = [fwd([mp.mpf(float(Ks[c, i])) for i in range(n)]) for c in range(m)]
        mu = [mp.fsum(V[c][i] * z[i] for i in range(n)) + mp.mpf(float(mean_t[c])) for c in range(m)]
        cov = [[mp.mpf(float(Kss[c, d])) - mp.fsum(V[c][i] * V[d][i] for i in range(n)) for d in range(m)]
               for c in range(m)]
        return np.array([float(v) for v in mu]), np.array([[float(v) for v in row] for row in cov])


MP_CASES = {
    "stationary_1d": (lambda: K.ConstantKernel(log_constant=0.2) * K.ExpSquaredKernel(0.7), 1),
    "sum_1d": (lambda: K.Matern32Kernel(0.5) + 0.3 * K.ExpSine2Kernel(gamma=1.0, log_period=0.2), 1),
    "axis_aligned_3d": (lambda: 1.5 * K.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + K.ConstantKernel(0.1, ndim=3), 3),
}


@pytest.mark.parametrize("n", [1, 17, 40])
@pytest.mark.parametrize("name", sorted(MP_CASES))
def test_reference_matches_50_digit_evaluation(name, n):
    make, ndim = MP_CASES[name]
    kernel = make()
    rng = np.random.RandomState(n + ndim)
    x = rng.uniform(0.0, 2.0, (n, ndim))
    xs = rng.uniform(-0.2, 2.2, (9, ndim))
    sigma = 0.1 + 0.05 * rng.rand(n)
    r = rng.randn(n)
    mean_t = 0.3 * rng.randn(9)
    ref = R.reference(kernel, x, sigma, r, xs, mean_t)
    mu, cov = _mp_predict(kernel, x, sigma, r, xs, mean_t)
    assert ref.kappa <= 1e6
    assert np.all(ref.S_mu > 0) and np.all(ref.S_cov >= np.abs(ref.cov))
    assert ref.ratio_mu(mu) < 0.1, (ref.mu, mu)              # the reference uses at most a tenth of the allowance
    assert ref.ratio_cov(cov) < 0.1
    assert ref.ratio_var(np.diag(cov)) < 0.1


# ------------------------------------------------------------------ the tolerance tells right from wrong
@functools.lru_cache(maxsize=None)
def _disc_problem():
    """A GP with a linear mean, fitted white noise and a Matern32 kernel (positive definite without its error bars
    too), at 60 points and 60 test points, and three parameter vectors."""
    rng = np.random.RandomState(4)
    x = np.sort(rng.uniform(0, 10, 60))
    gp = GP(1.3 * K.Matern32Kernel(0.8), mean=LinearMean(m=0.4, b=-1.0), white_noise=np.log(0.02),
            fit_white_noise=True)
    gp._x = np.ascontiguousarray(gp.parse_samples(x), dtype=np.float64)
    gp._yerr2 = np.full(60, 0.1 ** 2)
    y = np.sin(x) + 0.1 * rng.randn(60)
    xs = np.ascontiguousarray(gp.parse_samples(np.linspace(-1.0, 11.0, 60)), dtype=np.float64)
    p0 = gp.get_parameter_vector()
    vec = p0 + 0.05 * rng.randn(3, len(p0))
    return gp, y, xs, vec, R.batch_reference(gp, vec, y, xs)


def _worst(ref, bad, members):
    return min(max(ref[b].ratio_mu(bad[b].mu), ref[b].ratio_cov(bad[b].cov)) for b in members)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_tolerance_rejects_each_defect_by_a_wide_margin(defect):
    gp, y, xs, vec, ref = _disc_problem()
    bad = R.batch_reference(gp, vec, y, xs, defect=defect)
    members = [0, 1] if defect == "swap_members" else [0, 1, 2]
    assert _worst(ref, bad, members) > 1e4, defect
    assert _worst(ref, ref, members) == 0.0


def test_unknown_defect_is_refused():
    gp, y, xs, vec, _ = _disc_problem()
    with pytest.raises(ValueError):
        R.batch_reference(gp, vec, y, xs, defect="nonsense")
