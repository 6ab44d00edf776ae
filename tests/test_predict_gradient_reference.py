"""The reference of tests/predgrad_ref.py, checked on the CPU: the power of its tolerance rule to reject a wrong derivative,
and its agreement with central differences of the prediction reference itself.  (No GPU needed.)"""
import functools

import numpy as np
import pytest

import predgrad_ref as R
import predict_ref
from george_amd import kernels as K

# one stationary kernel and one with a non-zero diagonal term D, in one and three dimensions
DISC_KERNELS = {
    "stationary_1d": (lambda: 1.3 * K.ExpSquaredKernel(0.8), 1),
    "stationary_3d": (lambda: 1.3 * K.ExpSquaredKernel([0.8, 1.5, 0.6], ndim=3), 3),
    "polynomial_1d": (lambda: 0.5 * K.ExpSquaredKernel(0.8) + 0.2 * K.PolynomialKernel(log_sigma2=0.1, order=2), 1),
    "polynomial_3d": (lambda: 0.5 * K.ExpSquaredKernel([0.8, 1.5, 0.6], ndim=3)
                      + 0.2 * K.PolynomialKernel(log_sigma2=0.1, order=2, ndim=3), 3),
}


@functools.lru_cache(maxsize=None)
def _disc_problem(name):
    make, nd = DISC_KERNELS[name]
    rng = np.random.RandomState(11 + nd)
    n, m = 40, 12
    x = rng.uniform(0.0, 3.0, (n, nd))
    xs = rng.uniform(0.2, 2.8, (m, nd))
    sigma = 0.2 + 0.05 * rng.rand(n)
    r = np.sin(x.sum(axis=1)) + 0.1 * rng.randn(n)
    return make(), x, sigma, r, xs


def _is_a_defect(defect, name):
    """where the defect changes the result at all: D is identically zero for a stationary kernel, and one dimension
    cannot be swapped"""
    if defect == "drop_diag_term":
        return name.startswith("polynomial")
    if defect == "swap_dims":
        return name.endswith("3d")
    return True


@pytest.mark.parametrize("name", sorted(DISC_KERNELS))
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_tolerance_rejects_each_defect_by_a_wide_margin(defect, name):
    kernel, x, sigma, r, xs = _disc_problem(name)
    ref = R.reference(kernel, x, sigma, r, xs)
    bad = R.reference(kernel, x, sigma, r, xs, defect=defect)
    rm, rv = ref.ratio_dmu(bad.dmu), ref.ratio_dvar(bad.dvar)
    print("%s %s: kappa %.3g, error / tolerance dmu %.3g dvar %.3g" % (name, defect, ref.kappa, rm, rv))
    assert ref.kappa <= 1e6
    assert ref.ratio_dmu(ref.dmu) == 0.0 and ref.ratio_dvar(ref.dvar) == 0.0
    if not _is_a_defect(defect, name):
        assert rm == 0.0 and rv == 0.0
        return
    if defect in ("drop_factor_2", "drop_diag_term"):                  # these touch the variance only
        assert rm == 0.0 and rv > 1e4
    else:
        assert rm > 1e4 and rv > 1e4


def test_x2_for_x1_flips_the_sign_on_a_stationary_kernel():
    kernel, x, sigma, r, xs = _disc_problem("stationary_3d")
    ref = R.reference(kernel, x, sigma, r, xs)
    bad = R.reference(kernel, x, sigma, r, xs, defect="x2_for_x1")
    assert np.array_equal(bad.dmu, -ref.dmu) and np.array_equal(bad.dvar, -ref.dvar) and np.all(ref.D == 0.0)


def test_unknown_defect_is_refused():
    kernel, x, sigma, r, xs = _disc_problem("stationary_1d")
    with pytest.raises(ValueError):
        R.reference(kernel, x, sigma, r, xs, defect="nonsense")


# ------------------------------------------------------------------ central differences of the prediction reference
FD_KERNELS = {
    "expsquared_1d": (lambda: 1.2 * K.ExpSquaredKernel(0.7), 1),
    "matern52_3d": (lambda: 0.9 * K.Matern52Kernel([1.0, 2.0, 0.5], ndim=3), 3),
    "ratquad_2d": (lambda: K.RationalQuadraticKernel(log_alpha=0.3, metric=1.1, ndim=2) + K.ConstantKernel(-1.0, ndim=2), 2),
    "expsine2_1d": (lambda: 0.8 * K.ExpSine2Kernel(gamma=0.9, log_period=0.6), 1),
    "polynomial_2d": (lambda: 0.6 * K.ExpSquaredKernel(1.0, ndim=2) + 0.1 * K.PolynomialKernel(log_sigma2=0.2, order=3, ndim=2), 2),
}
EPS = 1.32e-6                    # the step and allclose settings of Kernel._fd_x: atol = 0.5 * eps, on values scaled by S


@pytest.mark.parametrize("name", sorted(FD_KERNELS))
def test_reference_agrees_with_central_differences_of_the_prediction(name):
    make, nd = FD_KERNELS[name]
    kernel = make()
    rng = np.random.RandomState(3 + nd)
    n, m = 25, 6
    x = rng.uniform(0.0, 2.0, (n, nd))
    xs = rng.uniform(0.1, 1.9, (m, nd))
    sigma = 0.25 + 0.05 * rng.rand(n)
    r = rng.randn(n)
    ref = R.reference(kernel, x, sigma, r, xs)
    print("%s: kappa %.3g" % (name, ref.kappa))
    assert ref.kappa <= 1e5
    fd_mu, fd_var = np.empty((m, nd)), np.empty((m, nd))
    for d in range(nd):
        tp, tm = xs.copy(), xs.copy()
        tp[:, d] += EPS
        tm[:, d] -= EPS
        p, q = predict_ref.reference(kernel, x, sigma, r, tp), predict_ref.reference(kernel, x, sigma, r, tm)
        fd_mu[:, d] = 0.5 * (p.mu - q.mu) / EPS
        fd_var[:, d] = 0.5 * (p.var - q.var) / EPS
    assert np.all(ref.S_dmu > 0) and np.all(ref.S_dvar > 0)
    assert np.allclose(ref.dmu / ref.S_dmu, fd_mu / ref.S_dmu, atol=0.5 * EPS)
    assert np.allclose(ref.dvar / ref.S_dvar, fd_var / ref.S_dvar, atol=0.5 * EPS)
    # signs, the factor 2 and the D term are not within that allowance of one another
    for defect in ("drop_factor_2", "x2_for_x1") + (("drop_diag_term",) if name.startswith("polynomial") else ()):
        bad = R.reference(kernel, x, sigma, r, xs, defect=defect)
        assert not np.allclose(bad.dvar / ref.S_dvar, fd_var / ref.S_dvar, atol=0.5 * EPS), defect
