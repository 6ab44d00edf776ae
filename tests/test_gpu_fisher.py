"""The expected information of the hyper-parameters on the device (``-m gpu``): gh_chol_fisher, BasicSolver.fisher and the GP
methods against the CPU reference of tests/fisher_ref.py under its one tolerance rule
(``|F_ab - ref| <= 32 * 2^-53 * kappa * sqrt(F_aa F_bb)``), and against themselves (mask / no mask, blocked / resident,
call / call again).

The sizes are where the 64-wide evaluation tile, the 128-wide tile of the products and the contraction, and the padding can
go wrong."""
import numpy as np
import pytest

import fisher_ref as R
from george_amd import GP, BasicSolver, HODLRSolver
from george_amd import _native as N
from george_amd.modeling import Model

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 300]
CASES = [(k, n) for k in ("expsq", "hyper") for n in SIZES] + [("2d", 129), ("2d", 300), ("p13", 200), ("p17", 129)]


def _computed(name, n):
    kernel, x, yerr, rows, ref = R.cached(name, n)
    s = BasicSolver(kernel)
    s.compute(x, yerr)
    return s, rows, ref


# ------------------------------------------------------------------ 1. parity with the CPU reference
@pytest.mark.parametrize("name,n", CASES)
def test_matches_the_reference_with_and_without_diagonal_parameters(name, n):
    s, rows, ref = _computed(name, n)
    P = s._dk.size
    F = s.fisher(diag_rows=rows)
    assert F.shape == (2 + P, 2 + P)
    ratio = ref.ratio(F)
    F0 = s.fisher()
    assert F0.shape == (P, P)
    ratio0 = ref.ratio(F0, 2 + np.arange(P))
    print("%s N=%d: kappa %.3g, error / tolerance %.3g with two diagonal parameters, %.3g without" % (name, n, ref.kappa, ratio, ratio0))
    assert ratio <= 1.0 and ratio0 <= 1.0
    assert np.array_equal(F, F.T) and np.array_equal(F0, F0.T)
    assert np.array_equal(F[2:, 2:], F0)                          # a pair's sum does not depend on the other planes


# ------------------------------------------------------------------ 2. masks, symmetry, repeatability
def test_partial_mask_zeroes_rows_and_columns_and_keeps_the_other_bits():
    s, rows, ref = _computed("hyper", 300)
    P = s._dk.size
    full = s.fisher(diag_rows=rows)
    which = np.arange(P) % 2 == 0
    part = s.fisher(which=which, diag_rows=rows)
    keep = np.concatenate([[0, 1], 2 + np.flatnonzero(which)])
    gone = 2 + np.flatnonzero(~which)
    assert np.all(part[gone, :] == 0.0) and np.all(part[:, gone] == 0.0)
    assert np.array_equal(part[np.ix_(keep, keep)], full[np.ix_(keep, keep)])
    none = s.fisher(which=np.zeros(P, dtype=bool))
    assert none.shape == (P, P) and np.all(none == 0.0)


def test_symmetric_bit_for_bit_and_two_calls_give_the_same_bits():
    s, rows, _ = _computed("p13", 200)
    a = s.fisher(diag_rows=rows)
    b = s.fisher(diag_rows=rows)
    assert np.array_equal(a, a.T) and np.array_equal(a, b)


# ------------------------------------------------------------------ 3. the memory rule
def test_blocked_calls_give_the_bits_of_the_resident_call_and_too_little_memory_raises():
    n = 300
    s, rows, _ = _computed("hyper", n)
    P = s._dk.size
    assert 2 + P >= 8                                             # two planes resident: one per block, at least eight blocks
    r = np.sin(np.arange(n))
    before = s.dot_solve(r)
    resident = s.fisher(diag_rows=rows)
    for planes in (2, 3):                                         # blocks of 1 and of 2 planes beside the scratch plane
        blocked = s.fisher(diag_rows=rows, max_bytes=BasicSolver.fisher_bytes(n, planes))
        assert np.array_equal(blocked, resident), planes
    exact = s.fisher(diag_rows=rows, max_bytes=BasicSolver.fisher_bytes(n, 2 + P))
    assert np.array_equal(exact, resident)
    with pytest.raises(MemoryError):
        s.fisher(diag_rows=rows, max_bytes=BasicSolver.fisher_bytes(n, 1))
    assert s.computed and s.dot_solve(r) == before


def test_factor_untouched_and_trim_gives_the_memory_back():
    n = 300
    BasicSolver.release_pool()                                    # a handle of its own: nothing grown by an earlier test
    s, rows, _ = _computed("hyper", n)
    r = np.cos(np.arange(n))
    before, logdet = s.dot_solve(r), s.log_determinant
    h = s._handle
    N.lib.gh_chol_trim(h)
    base = int(N.lib.gh_chol_device_bytes(h))
    s.fisher(diag_rows=rows)
    grown = int(N.lib.gh_chol_device_bytes(h))
    np_ = -(-n // 128) * 128
    print("fisher: %d bytes above the factor (%d planes of %d)" % (grown - base, 2 + s._dk.size, 8 * np_ * np_))
    assert grown - base >= BasicSolver.fisher_bytes(n, 2 + s._dk.size)
    assert s.dot_solve(r) == before and s.log_determinant == logdet
    N.lib.gh_chol_trim(h)
    assert int(N.lib.gh_chol_device_bytes(h)) == base
    assert s.dot_solve(r) == before


# ------------------------------------------------------------------ 4. the GP surface
class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b

    def compute_gradient(self, t):
        return np.stack([t, np.ones_like(t)])


class NoiseRamp(Model):
    parameter_names = ("a", "c")

    def get_value(self, t):
        return self.a + self.c * t

    def compute_gradient(self, t):
        return np.stack([np.ones_like(t), t])


def test_gp_on_the_device_agrees_with_hodlr_through_the_numpy_branch():
    n = 300
    kernel, x, yerr, _ = R.problem("hyper", n)
    kernel.freeze_parameter("k1:k1:k1:k2:metric:log_M_0_0")
    t = x[:, 0]
    a, c = np.log(0.5 * np.min(yerr ** 2)), 0.1
    wn = np.exp(a + c * t)

    def gp_on(solver, **kw):
        gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=a, c=c), fit_white_noise=True, solver=solver, **kw)
        gp.compute(t, yerr)
        return gp

    dense, hod = gp_on(BasicSolver), gp_on(HODLRSolver, tol=1e-14)
    assert callable(dense.solver.fisher) and not callable(getattr(hod.solver, "fisher", None))
    Fd, Fh = dense.fisher_information(), hod.fisher_information()
    P = len(dense)
    assert Fd.shape == Fh.shape == (P, P) and P == 2 + 2 + 10
    assert np.all(Fd[:2, 2:] == 0.0) and np.all(Fd[2:, :2] == 0.0) and np.array_equal(Fd, Fd.T)
    ref = R.reference(kernel, x, np.sqrt(yerr ** 2 + wn), np.stack([wn, wn * t]))
    keep = np.concatenate([[0, 1], 2 + np.flatnonzero(kernel.unfrozen_mask)])
    rd, rh = ref.ratio(Fd[2:, 2:], keep), ref.ratio(Fh[2:, 2:], keep)
    tol = ref.tol()[np.ix_(keep, keep)]
    between = R.Ref._ratio(Fd[2:, 2:] - Fh[2:, 2:], tol)
    dm = np.sqrt(np.diag(Fd[:2, :2]))
    mean_between = R.Ref._ratio(Fd[:2, :2] - Fh[:2, :2], R.C_TOL * R.U * ref.kappa * np.outer(dm, dm))
    print("kappa %.3g, error / tolerance: device %.3g, HODLR %.3g, device against HODLR %.3g (mean block %.3g)"
          % (ref.kappa, rd, rh, between, mean_between))
    assert rd <= 1.0 and between <= 1.0 and mean_between <= 1.0
    # the Cramer-Rao covariance on the device path
    C = dense.parameter_covariance()
    kappa_F = np.linalg.cond(Fd)
    resid = np.max(np.abs(np.dot(C, Fd) - np.eye(P)))
    print("kappa(F) %.3g, |C F - I| %.3g" % (kappa_F, resid))
    assert C.shape == (P, P) and np.array_equal(C, C.T) and resid <= kappa_F * 1e-12
    assert np.all(np.diag(C) > 0.0)


# ------------------------------------------------------------------ 5. bad arguments
def test_bad_arguments():
    s, rows, _ = _computed("hyper", 65)
    P = s._dk.size
    with pytest.raises(ValueError):
        s.fisher(which=np.ones(P + 1, dtype=bool))
    with pytest.raises(ValueError):
        s.fisher(diag_rows=rows[:, :-1])
    with pytest.raises(ValueError):
        s.fisher(diag_rows=rows[0])
    fresh = BasicSolver(R.problem("hyper", 65)[0])
    with pytest.raises(RuntimeError, match="compute"):
        fresh.fisher()
