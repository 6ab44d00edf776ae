"""The host side of tests/test_gpu_vecchia_fisher.py: the restatement of the Vecchia information (tests/vecchia_fisher_ref.py)
against the dense long-double reference of tests/fisher_ref.py at full conditioning, the bound of the device tests against
deliberately wrong versions on those very problems, and the restatement of ``vecchia_fisher_kernel``'s LDS size against the
constants of the sources.  No device is touched.

Observed on the CPU (every test prints its figures): the two routes differ by 7e-16 .. 2e-14 of ``S_ab`` on the first 150 points
(bounds 8.9e-13 .. 2.1e-11); the weakest defect is ``drop_last_slot`` at P = 62, 0.78 of ``S_ab``.
"""
import os
import re

import numpy as np
import pytest

import fisher_ref
import vecchia_cases as VC
import vecchia_fisher_ref as VF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (parameters, dimension, LDS bytes of the information kernel with two diagonal rows at m = 64, at m = 7)
TABLE = {1: (1, 1, 31352, 11088), 5: (5, 2, 36176, 13664), 16: (16, 4, 50224, 21872), 17: (17, 4, 50896, 22096),
         37: (37, 16, 82496, 39264), 62: (62, 16, 119208, 64776)}


# ------------------------------------------------------------------ full conditioning: the dense information
@pytest.mark.parametrize("name,n", [("expsq", 65), ("hyper", 65), ("2d", 129), ("p17", 129)])
def test_full_conditioning_is_the_dense_information(name, n):
    """with every predecessor in the set the block formula is 1/2 tr(K^-1 D_a K^-1 D_b): within fisher_ref's own rule"""
    kernel, x, yerr, rows, dense = fisher_ref.cached(name, n)
    ref = VF.reference(kernel, x, yerr, VF.full_table(n), rows)
    ratio = dense.ratio(ref.F)
    print("%s N=%d: kappa %.3g, error / tolerance %.3g" % (name, n, dense.kappa, ratio))
    assert ref.F.shape == dense.F.shape and ratio <= 1.0
    assert VC._over(ref.S - dense.S, dense.S) <= 1e-10
    # and with fewer neighbours it is another quantity: far outside that rule
    near = VF.reference(kernel, x, yerr, VF.vecchia_neighbors(x, 4), rows)
    assert dense.ratio(near.F) > 1e3


def test_masks_and_no_diagonal_rows():
    kernel, x, yerr, rows = VF.problem(5, 40)
    nbr = VF.vecchia_neighbors(x, 7)
    full = VF.reference(kernel, x, yerr, nbr, rows)
    which = np.array([1, 0, 1, 1, 0], dtype=bool)
    part = VF.reference(kernel, x, yerr, nbr, rows, which=which)
    keep = np.concatenate([[0, 1], 2 + np.flatnonzero(which)])
    gone = 2 + np.flatnonzero(~which)
    assert np.all(part.F[gone] == 0.0) and np.all(part.F[:, gone] == 0.0) and np.all(part.S[gone] == 0.0)
    assert np.array_equal(part.F[np.ix_(keep, keep)], full.F[np.ix_(keep, keep)])
    bare = VF.reference(kernel, x, yerr, nbr)
    assert bare.F.shape == (5, 5) and VC._over(bare.F - full.F[2:, 2:], full.S[2:, 2:]) <= 64 * VF.EPS    # (NumPy's products: not bits)
    with pytest.raises(ValueError):
        VF.reference(kernel, x, yerr, nbr, rows[:, :-1])
    with pytest.raises(ValueError):
        VF.reference(kernel, x, yerr, nbr, defect="diag_unpermuted")
    with pytest.raises(ValueError):
        VF.reference(kernel, x, yerr, nbr, rows, defect="none")


# ------------------------------------------------------------------ the problems and their bounds
@pytest.mark.parametrize("case,n", [(c, 300) for c in VF.CASES] + [(62, 1), (62, 2), (62, 64), (62, 65), (1, 1)])
def test_the_two_cpu_routes_stay_inside_the_cap(case, n):
    g, bound = VF.gap(case, n), VF.bound(case, n)
    assert g <= VF.GAP_CAP and g <= bound <= max(1000.0 * g, 4000.0 * VF.EPS)


@pytest.mark.parametrize("n", [4099, 8200])
def test_the_two_cpu_routes_stay_inside_the_cap_at_the_grid_stride_sizes(n):
    assert VF.gap(5, n) <= VF.GAP_CAP


@pytest.mark.parametrize("m", [7, 64])
@pytest.mark.parametrize("case", VF.CASES)
def test_the_bound_of_the_device_tests_rejects_every_defect(case, m):
    kernel, x, yerr, rows = VF.problem(case)
    ref, nbr = VF.cached(case, 300, m)
    bound = VF.bound(case)
    assert np.all(ref.S > 0.0) and np.array_equal(ref.F, ref.F.T) and (nbr[-1] >= 0).sum() == m
    assert ref.F.shape == (2 + len(kernel), 2 + len(kernel))
    for defect in VF.DEFECTS:
        bad = VF.reference(kernel, x, yerr, nbr, rows, defect=defect)
        assert np.array_equal(bad.S, ref.S)
        err = VC._over(bad.F - ref.F, ref.S)
        print("P=%d m=%d %-15s error over S %.3g  bound %.3g" % (case, m, defect, err, bound))
        assert err > bound, (defect, err, bound)


# ------------------------------------------------------------------ the LDS size
def test_lds_bytes_of_the_table():
    assert set(TABLE) == set(VF.CASES)
    for case, (P, ndim, big, small) in TABLE.items():
        kernel, x, yerr, rows = VF.problem(case)
        assert len(kernel) == P and x.shape == (300, ndim) and rows.shape == (2, 300)
        assert VF.fisher_lds_bytes(64, ndim, P, P + 2) == big and VF.fisher_lds_bytes(7, ndim, P, P + 2) == small, case
    # the switch of the device tests: 62 parameters in 16-D with two diagonal rows, m = 8 the largest at or below 64 KB, m = 9 the
    # smallest above; everything inside the raised limit, the full 64 parameters in 64 planes included
    assert VF.fisher_lds_bytes(8, 16, 62, 64) == 65000 <= 65536 < VF.fisher_lds_bytes(9, 16, 62, 64) == 66264
    sizes = [VF.fisher_lds_bytes(m, 16, 62, 64) for m in range(1, 65)]
    assert sizes == sorted(sizes) and sizes[-1] == 119208
    assert VF.fisher_lds_bytes(64, 16, 64, 64) == 120232 <= VF.V_FISHER_LDS <= 160 * 1024


def test_the_restatement_reads_the_constants_of_the_sources():
    with open(os.path.join(ROOT, "george_amd", "csrc", "gh_vecchia.hip")) as f:
        hip = f.read()
    assert re.search(r"#define V_FISHER_LDS \((\d+) \* 1024\)", hip).group(1) == str(VF.V_FISHER_LDS // 1024)
    assert int(re.search(r"#define V_FISHER_PLANES (\d+)\b", hip).group(1)) == VF.V_FISHER_PLANES == VC.VM_MAX
    squeezed = re.sub(r"\s+", " ", hip)
    assert "static inline int v_fisher_pitch(int m) { return (m + 1) | 1; }" in squeezed
    assert ("return v_lds_doubles(m, nd, gp) + (size_t)Q * v_fisher_pitch(m) + VM_MAX + (size_t)Q * (Q + 1) / 2;" in squeezed)
    assert "const size_t lds = v_fisher_lds_doubles(m, h->ndim, gp, Q) * sizeof(double);" in squeezed
    assert "const int gp = (P + GH_EVAL_WS) | 1, npair = Q * (Q + 1) / 2;" in squeezed
    assert squeezed.count("if (lds > 64 * 1024) {") == 2 and "if (lds > V_FISHER_LDS) {" in squeezed
