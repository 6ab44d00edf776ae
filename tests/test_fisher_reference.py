"""The information reference of tests/fisher_ref.py pinned on the CPU: its tolerance rejects every planted defect, its matrix
means what it should (minus the derivative of the expected score), and it is symmetric positive definite."""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

import fisher_ref as R
from oracle import kernels_np, solver_np

_PIECES = {}


def _pieces(name, n):
    if (name, n) not in _PIECES:
        kernel, x, yerr, _ = R.problem(name, n)
        rows = R.diag_rows_for(x, yerr)
        _PIECES[(name, n)] = (kernel, x, yerr, rows, R.planes(kernel, x, yerr, rows))
    return _PIECES[(name, n)]


@pytest.mark.parametrize("name,n", [("hyper", 129), ("hyper", 300), ("2d", 129), ("2d", 300)])
def test_the_rule_rejects_every_defect(name, n):
    kernel, x, yerr, rows, pieces = _pieces(name, n)
    ref = R.reference(kernel, x, yerr, rows, pieces=pieces)
    assert ref.ratio(ref.F) == 0.0
    for defect in R.DEFECTS:
        bad = R.reference(kernel, x, yerr, rows, defect=defect, pieces=pieces)
        ratio = ref.ratio(bad.F)
        print("%s N=%d %-20s error / tolerance %.3g (kappa %.3g)" % (name, n, defect, ratio, ref.kappa))
        assert ratio > 1.0, defect


@pytest.mark.parametrize("name,n", [("hyper", 129), ("hyper", 300), ("2d", 129), ("2d", 300), ("expsq", 65)])
def test_symmetric_and_positive_definite(name, n):
    kernel, x, yerr, rows, pieces = _pieces(name, n)
    ref = R.reference(kernel, x, yerr, rows, pieces=pieces)
    assert np.array_equal(ref.F, ref.F.T)
    lam = np.linalg.eigvalsh(ref.F / ref.S)
    print("%s N=%d smallest eigenvalue of F / S: %.3g" % (name, n, lam[0]))
    assert lam[0] > 0.0


def _expected_score(kernel, x, yerr, K_true, theta):
    """1/2 tr((K'^-1 K K'^-1 - K'^-1) dK'/dtheta_a) at the kernel parameters ``theta`` (all of them), under y ~ N(0, K)"""
    saved = kernel.get_parameter_vector(include_frozen=True)
    kernel.set_parameter_vector(theta, include_frozen=True)
    try:
        Kp = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
        Kp[np.diag_indices(len(x))] += yerr ** 2
        G = np.asarray(kernels_np.gradient_general(kernel, x, x), dtype=np.float64)
    finally:
        kernel.set_parameter_vector(saved, include_frozen=True)
    cf = cho_factor(Kp, lower=True)
    Ki = cho_solve(cf, np.eye(len(x)))
    A = cho_solve(cf, cho_solve(cf, K_true).T) - Ki
    return 0.5 * np.einsum("ij,jip->p", A, G)


@pytest.mark.parametrize("name", ["expsq", "2d"])
def test_minus_the_derivative_of_the_expected_score(name):
    # Independent of the formula: under y ~ N(0, K(theta)) the score at theta' has the expectation above, which vanishes at
    # theta' = theta and whose derivative there is -F.  Central differences with step H in the (logarithmic) parameters.
    # Observed error relative to S_ab, both problems alike: 5.3e-7 at H = 1e-3, 8.5e-8 at 4e-4, 2.1e-8 at 2e-4, 5.9e-9 (expsq)
    # and 5.3e-9 (2d) at 1e-4, 1.3e-9 at 5e-5, 1.0e-9 at 2.5e-5: truncation 0.55 H^2 (a factor 4 per doubling) down to a
    # rounding floor of about 1e-9.  H = 1e-4 keeps the truncation well above that floor; the bound is five times the
    # truncation error there.  A dropped factor, a missing transpose or a wrong sign is off by order 1.
    H, BOUND = 1e-4, 3e-8
    kernel, x, yerr, _ = R.problem(name, 40)
    ref = R.reference(kernel, x, yerr)
    K = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    K[np.diag_indices(len(x))] += yerr ** 2
    theta = np.array(kernel.get_parameter_vector(include_frozen=True), dtype=np.float64)
    P = len(theta)
    assert ref.F.shape == (P, P)
    s0 = _expected_score(kernel, x, yerr, K, theta)
    assert np.max(np.abs(s0) / np.sqrt(np.diag(ref.F))) < 1e-9          # the expected score vanishes at the truth
    J = np.empty((P, P))
    for b in range(P):
        e = np.zeros(P)
        e[b] = H
        J[:, b] = (_expected_score(kernel, x, yerr, K, theta + e) - _expected_score(kernel, x, yerr, K, theta - e)) / (2 * H)
    err = np.max(np.abs(J + ref.F) / ref.S)
    print("%s: central differences of the expected score vs -F: %.3g relative to S" % (name, err))
    assert err <= BOUND
