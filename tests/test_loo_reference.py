"""The leave-one-out reference of tests/loo_ref.py, checked on the CPU: its closed forms against N explicit refits, its
gradient (kernel, mean and white-noise parameters) against central differences of the refit objective, and the power of
its tolerance rule to reject a wrong implementation.  (No GPU needed.)"""
import functools

import numpy as np
import pytest

import loo_ref as R
from george_amd import kernels as K

KERNELS = ("expsq", "matern3d", "hyper")


@functools.lru_cache(maxsize=None)
def _reference(name, n):
    return R.reference(*R.problem(name, n))


# ------------------------------------------------------------------ closed form against N refits
@pytest.mark.parametrize("n", [1, 2, 37, 129])
@pytest.mark.parametrize("name", KERNELS)
def test_closed_form_matches_explicit_refits(name, n):
    ref = _reference(name, n)
    L, lpd, resid, var = R.brute_force(*R.problem(name, n))
    ratios = dict(L=ref.ratio("L", L), lpd=ref.ratio("lpd", lpd), resid=ref.ratio("resid", resid), var=ref.ratio("var", var))
    print("%s N=%d: kappa %.3g, largest error / tolerance %.3g  %s" % (name, n, ref.kappa, max(ratios.values()), ratios))
    assert ref.kappa <= 1e6
    assert max(ratios.values()) <= 1.0
    assert np.all(ref.var > 0) and np.all(ref.c > 0)


# ------------------------------------------------------------------ gradient against central differences of the refits
def _mean(theta, t):
    return theta[0] * t + theta[1]                       # the LinearMean of tests/test_append_host.py


def _log_noise(theta, t):
    return theta[0] + theta[1] * t                       # ... and its NoiseRamp


def _matern3d_axis_aligned():
    build, ndim, amp = R.KERNELS["matern3d"]
    _, x, yerr, r = R.problem("matern3d", 37)
    return 0.9 * K.Matern32Kernel([1.2, 0.8, 1.5], ndim=3), x, yerr, r


# The general metric is left out of THIS check only: the reference evaluator's gradient entries for a general metric are not the
# derivatives with respect to its parameter vector (the diagonal entries differ by a factor, two off-diagonal ones change
# places; central differences of the kernel VALUE show it), and oracle/kernels_np.py and the device evaluator reproduce the
# reference entry for entry.  The contraction sum_ij B_ij dK_ij is checked for that kernel by the refit comparison above and by
# the defect test below; here the 3-D Matern-3/2 takes an axis-aligned metric.
#
# Which parameters the check can reach, from the arithmetic of central differences: their round-off term is the round-off of L
# over h, and L feels every entry of K -- the hyper.rst composite's are evaluated to a few ulp of 66^2 ~ 4e3 -- so that term is
# about U * max_p S_p / h = 1e-10 max_p S_p for EVERY parameter, not U * S_p / h.  It fits into the tolerance 1e-6 * S_p only
# while S_p >= 1e-4 max_p S_p: parameters below that floor are printed and not asserted.  ExpSquared and the Matern have none
# (their S_p lie within two decades); the composite's S_p span 0.3 .. 4.4e5, and its seven parameters with S_p < 44 show the
# same absolute difference of 1e-6 .. 3e-6 as the eight above the floor -- up to 6 tolerances for them, 0.003 at most for
# those.  The composite's whole gradient is held to loo_ref's rule on the device (tests/test_gpu_loo.py) and by the defect
# test below.
FLOOR = 1e-4


@pytest.mark.parametrize("name", ["expsq", "matern3d_axis", "hyper"])
def test_gradient_matches_central_differences_of_the_refit_objective(name):
    n, h = 37, 1e-6
    kernel, x, yerr, r = _matern3d_axis_aligned() if name == "matern3d_axis" else R.problem(name, n)
    name = "matern3d" if name == "matern3d_axis" else name
    t = x[:, 0]
    y = r + _mean([0.2, -1.0], t)
    amp2 = R.KERNELS[name][2] ** 2
    mean0, noise0 = np.array([0.2, -1.0]), np.array([np.log(0.02 * amp2), 0.03])
    theta0 = np.array(kernel.get_parameter_vector(include_frozen=True))

    def pieces(theta, mean_p, noise_p):
        kernel.set_parameter_vector(theta, include_frozen=True)
        return kernel, x, np.sqrt(yerr ** 2 + np.exp(_log_noise(noise_p, t))), y - _mean(mean_p, t)

    def objective(theta, mean_p, noise_p):
        return R.brute_force(*pieces(theta, mean_p, noise_p))[0]

    ref = R.reference(*pieces(theta0, mean0, noise0))
    wn = np.exp(_log_noise(noise0, t))
    mg = np.stack([t, np.ones(n)])                       # d mean / d (m, b); the residual falls as the mean rises: d r = -d mean
    ng = np.stack([np.ones(n), t])                       # d log-noise / d (a, c)
    # d L / d r_i = -v_i, so d L / d mean parameter = + mg @ v;   d L / d K_ii = diagB_i, d K_ii = exp(wn_i) d wn_i
    grads = np.concatenate([ref.g, mg @ ref.v, (ng * (wn * ref.diagB)[None, :]).sum(axis=1)])
    scales = np.concatenate([ref.S, np.abs(mg) @ np.abs(ref.v), (np.abs(ng) * (wn * ref.mag_diagB)[None, :]).sum(axis=1)])
    P = len(theta0)
    worst, checked = 0.0, 0
    for p in range(P + 4):
        args = [theta0.copy(), mean0.copy(), noise0.copy()]
        which, at = (0, p) if p < P else (1, p - P) if p < P + 2 else (2, p - P - 2)
        args[which][at] += h
        up = objective(*args)
        args[which][at] -= 2 * h
        down = objective(*args)
        fd = (up - down) / (2 * h)
        ratio = abs(fd - grads[p]) / (1e-6 * scales[p])
        reach = scales[p] >= FLOOR * np.max(scales)
        if reach:
            worst, checked = max(worst, ratio), checked + 1
        print("%s parameter %d: closed form %.12g, central difference %.12g, scale %.3g, error / (1e-6 S) %.3g%s"
              % (name, p, grads[p], fd, scales[p], ratio, "" if reach else "  (below the round-off floor: not asserted)"))
    kernel.set_parameter_vector(theta0, include_frozen=True)
    assert worst <= 1.0
    assert checked == (8 if name == "hyper" else P + 4)


# ------------------------------------------------------------------ the tolerance tells right from wrong
WHERE = {"diag_weight_half": ("g",), "outer_half_kept": ("g",), "w_without_alpha_term": ("g", "diagB"), "v_is_u": ("g", "v", "diagB"),
         "drop_last_row": ("g",), "padded_rows_in_L": ("L",)}


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("name", KERNELS)
def test_tolerance_rejects_every_defect(name, defect):
    n = 129                                              # three 64-row tiles, the last one a single row; 127 padded rows
    ref = _reference(name, n)
    for q in ("L", "lpd", "resid", "var", "v", "diagB", "g"):
        assert ref.ratio(q, getattr(ref, q)) == 0.0
    bad = R.reference(*R.problem(name, n), defect=defect)
    for q in WHERE[defect]:
        ratio = ref.ratio(q, getattr(bad, q))
        print("%s, %s: %s off by %.3g tolerances" % (name, defect, q, ratio))
        assert ratio >= 10.0, (name, defect, q, ratio)


def test_defects_are_the_six_of_the_issue_and_sizes_are_what_they_claim():
    assert sorted(WHERE) == sorted(R.DEFECTS) and len(R.DEFECTS) == 6
    from oracle import kernels_np
    sizes = {name: kernels_np.full_size(R.KERNELS[name][0]()) for name in R.KERNELS}
    assert sizes == {"expsq": 2, "matern3d": 7, "hyper": 11, "2d": 5, "p13": 13, "p17": 17}
    for name, (build, ndim, amp) in R.KERNELS.items():
        kernel, x, yerr, r = R.problem(name, 65)
        assert x.shape == (65, ndim) and kernel.ndim == ndim
        assert np.all(yerr >= 0.1 * amp)
    assert isinstance(R.KERNELS["hyper"][0](), K.Sum)
