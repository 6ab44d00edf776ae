"""The leave-group-out reference of tests/lgo_ref.py, checked on the CPU: its closed forms against G explicit refits, its
gradient (kernel, mean and white-noise parameters) against central differences of the refit objective, its one-point-group
case against tests/loo_ref.py, and the power of its tolerance rule to reject a wrong implementation.  (No GPU needed.)"""
import functools

import numpy as np
import pytest

import lgo_ref as R
import loo_ref
from george_amd import kernels as K


@functools.lru_cache(maxsize=None)
def _case(name, n, grouping):
    labels = R.grouping(grouping, n)
    if labels is None:
        return None
    order, start = R.order_start(labels)
    return R.problem(name, n) + (order, start)


@functools.lru_cache(maxsize=None)
def _reference(name, n, grouping):
    return R.reference(*_case(name, n, grouping))


# ------------------------------------------------------------------ closed form against G refits
@pytest.mark.parametrize("n", [1, 2, 37, 129])
@pytest.mark.parametrize("name", sorted(R.KERNELS))
def test_closed_form_matches_explicit_refits(name, n):
    seen = 0
    for grouping in R.GROUPINGS:
        case = _case(name, n, grouping)
        if case is None:
            assert grouping == "one" and n > 128
            continue
        seen += 1
        ref = _reference(name, n, grouping)
        L, lpd, resid, var, covs = R.brute_force(*case)
        ratios = dict(L=ref.ratio("L", L), lpd=ref.ratio("lpd", lpd), resid=ref.ratio("resid", resid), var=ref.ratio("var", var),
                      cov=ref.ratio("cov", covs))
        print("%s N=%d %s: %d groups, kappa %.3g, largest error / tolerance %.3g  %s"
              % (name, n, grouping, len(lpd), ref.kappa, max(ratios.values()), ratios))
        assert ref.kappa <= 1e6
        assert max(ratios.values()) <= 1.0, (grouping, ratios)
        assert np.all(ref.var > 0) and lpd.shape == ref.lpd.shape == (len(case[5]) - 1,)
    assert seen == (8 if n <= 128 else 7)


def test_groupings_are_what_they_claim():
    for n in (1, 2, 37, 129, 300, 1000):
        for grouping in R.GROUPINGS:
            labels = R.grouping(grouping, n)
            if labels is None:
                continue
            order, start = R.order_start(labels)
            sizes = np.diff(start)
            assert sorted(order) == list(range(n)) and start[0] == 0 and start[-1] == n
            assert np.all(sizes >= 1) and np.all(sizes <= 128)
            for g in range(len(sizes)):                      # one label per group, points in data order
                I = order[start[g]:start[g + 1]]
                assert len(set(labels[I])) == 1 and np.all(np.diff(I) > 0)
    assert np.array_equal(np.diff(R.order_start(R.grouping("blk128", 129))[1]), [128, 1])
    assert np.array_equal(np.diff(R.order_start(R.grouping("blk7", 129))[1]), [7] * 18 + [3])
    lab = R.grouping("labels", 129)
    assert lab.min() < 0 and np.any(np.diff(lab) < 0) and np.any(np.diff(lab) > 0) and set(np.diff(np.unique(lab))) == {3}
    assert not np.array_equal(R.order_start(lab)[0], np.arange(129))
    rnd = R.grouping("random", 300)
    assert np.any(np.diff(R.order_start(rnd)[0]) < 0)        # scattered: not contiguous
    rag = np.diff(R.order_start(R.grouping("ragged", 1000))[1])
    assert set(rag[:-1]) <= {1, 2, 5, 31, 64, 100, 128} and 128 in rag and len(R.slots(R.order_start(R.grouping("ragged", 1000))[1])) < len(rag)


# ------------------------------------------------------------------ one-point groups are leave-one-out
@pytest.mark.parametrize("name", ["expsq", "matern3d", "hyper"])
def test_singletons_reproduce_the_leave_one_out_reference(name):
    n = 129
    ref = _reference(name, n, "singletons")
    loo = loo_ref.reference(*R.problem(name, n))
    ratios = {q: loo.ratio(q, getattr(ref, q)) for q in ("L", "lpd", "resid", "var", "v", "diagB", "g")}
    print("%s: singletons against loo_ref, error / tolerance %s" % (name, ratios))
    assert max(ratios.values()) <= 1.0
    for q in ("resid", "var", "lpd", "L", "v", "diagB"):      # the scales agree too
        assert np.isclose(getattr(ref, "S_" + q), getattr(loo, "S_" + q), rtol=1e-9)
    assert np.allclose(ref.S, loo.S, rtol=1e-9)


# ------------------------------------------------------------------ gradient against central differences of the refits
def _mean(theta, t):
    return theta[0] * t + theta[1]


def _log_noise(theta, t):
    return theta[0] + theta[1] * t


def _matern3d_axis_aligned():
    _, x, yerr, r = R.problem("matern3d", 37)
    return 0.9 * K.Matern32Kernel([1.2, 0.8, 1.5], ndim=3), x, yerr, r


# As in tests/test_loo_reference.py: the general metric is left out of this check only (the reference evaluator's gradient
# entries for it are not the derivatives with respect to its parameter vector), and a parameter whose scale lies below
# FLOOR of the largest is printed, not asserted: the round-off of the central difference, U max_p S_p / h, exceeds its
# tolerance 1e-6 S_p.
FLOOR = 1e-4


@pytest.mark.parametrize("grouping", ["blk7", "random"])
@pytest.mark.parametrize("name", ["expsq", "matern3d_axis", "hyper"])
def test_gradient_matches_central_differences_of_the_refit_objective(name, grouping):
    n, h = 37, 1e-6
    kernel, x, yerr, r = _matern3d_axis_aligned() if name == "matern3d_axis" else R.problem(name, n)
    name = "matern3d" if name == "matern3d_axis" else name
    order, start = R.order_start(R.grouping(grouping, n))
    t = x[:, 0]
    y = r + _mean([0.2, -1.0], t)
    amp2 = R.KERNELS[name][2] ** 2
    mean0, noise0 = np.array([0.2, -1.0]), np.array([np.log(0.02 * amp2), 0.03])
    theta0 = np.array(kernel.get_parameter_vector(include_frozen=True))

    def pieces(theta, mean_p, noise_p):
        kernel.set_parameter_vector(theta, include_frozen=True)
        return kernel, x, np.sqrt(yerr ** 2 + np.exp(_log_noise(noise_p, t))), y - _mean(mean_p, t), order, start

    def objective(theta, mean_p, noise_p):
        return R.brute_force(*pieces(theta, mean_p, noise_p))[0]

    ref = R.reference(*pieces(theta0, mean0, noise0))
    wn = np.exp(_log_noise(noise0, t))
    mg = np.stack([t, np.ones(n)])                       # d mean / d (m, b); d r = -d mean and d L / d r_i = -v_i
    ng = np.stack([np.ones(n), t])                       # d log-noise / d (a, c); d K_ii = exp(wn_i) d wn_i
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
        print("%s %s parameter %d: closed form %.12g, central difference %.12g, scale %.3g, error / (1e-6 S) %.3g%s"
              % (name, grouping, p, grads[p], fd, scales[p], ratio, "" if reach else "  (below the round-off floor: not asserted)"))
    kernel.set_parameter_vector(theta0, include_frozen=True)
    assert worst <= 1.0
    assert checked >= (7 if name == "hyper" else P + 4)      # (the composite: the four mean and noise parameters, three of the kernel's at least)


# ------------------------------------------------------------------ the tolerance tells right from wrong
WHERE = {"cross_group_entries_kept": ("resid", "var", "L", "g"), "u_outer_dropped": ("g", "diagB"), "logdet_sign": ("lpd", "L"),
         "order_not_undone": ("resid", "var"), "last_group_dropped": ("lpd", "L", "g"), "padded_rows_in_L": ("L",)}


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("name", sorted(R.KERNELS))
def test_tolerance_rejects_every_defect(name, defect):
    # windows of 7 under shuffled labels at n = 129: 18 groups to a slot, a permutation to undo, 127 padded rows
    n, grouping = 129, "labels"
    ref = _reference(name, n, grouping)
    for q in ("L", "lpd", "resid", "var", "cov", "v", "diagB", "g"):
        assert ref.ratio(q, getattr(ref, q)) == 0.0
    bad = R.reference(*_case(name, n, grouping), defect=defect)
    for q in WHERE[defect]:
        ratio = ref.ratio(q, getattr(bad, q))
        print("%s, %s: %s off by %.3g tolerances" % (name, defect, q, ratio))
        assert ratio >= 10.0, (name, defect, q, ratio)


def test_defects_are_the_six_of_the_issue():
    assert sorted(WHERE) == sorted(R.DEFECTS) and len(R.DEFECTS) == 6
    assert R.GROUPINGS == ("singletons", "blk7", "blk64", "blk128", "one", "random", "ragged", "labels")
