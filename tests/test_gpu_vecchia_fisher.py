"""``VecchiaSolver.fisher_blocks`` on the device (gh_vecchia_fisher, ``vecchia_fisher_kernel`` of george_amd/csrc/gh_vecchia.hip) against
the NumPy restatement of tests/vecchia_fisher_ref.py, and ``GP.fisher_information`` / ``GP.parameter_covariance`` through it.

The kernel sizes its dynamic LDS as ``v_fisher_lds_doubles``: what the gradient kernel takes, ``Q`` plane rows of the odd pitch
``(m + 1) | 1``, 64 values ``df_a`` and ``Q (Q + 1) / 2`` packed pairs, ``Q`` = diagonal rows + unmasked kernel parameters <= 64.
Above 64 KB the host raises the kernel's limit first.  ``vecchia_fisher_ref.fisher_lds_bytes`` restates the size;
tests/test_vecchia_fisher_host.py holds it to this table (two diagonal rows) and to the constants of the sources.

=========  ====  =================  ================
kernel     ndim  LDS bytes, m = 64  LDS bytes, m = 7
=========  ====  =================  ================
P = 1      1     31 352             11 088
P = 5      2     36 176             13 664
P = 16     4     50 224             21 872
P = 17     4     50 896             22 096
P = 37     16    82 496 (raised)    39 264
P = 62     16    119 208 (raised)   64 776
=========  ====  =================  ================

=====  =================================================================================================================
group  what
=====  =================================================================================================================
a      every kernel of the table at N = 300 with m = 7 and m = 64 and the two diagonal rows of ``fisher_ref.diag_rows_for``
       (P = 62 with them: the 64-plane cap) against the restatement
b      full conditioning, N = 65 and m = 64: against ``fisher_ref.reference`` (dense, long double) and ``BasicSolver.fisher``
c      the 64 KB switch with P = 62 in 16-D: m = 8 (65 000 bytes, the largest below), m = 9 (66 264, the smallest above); then
       m = 64, m = 7, m = 64 again: the two m = 64 results agree bit for bit
d      masks at P = 5 / 17 / 62: masked rows and columns exactly 0, kept entries the bits of the all-ones call; no diagonal
       rows; diagonal rows only; 65 planes raise ``ValueError`` and 64 of a 64-parameter kernel do not
e      more points than workgroups (4096), P = 5 in 2-D, m = 7: N = 4099 and N = 8200
f      N = 1 / 2 / 64 / 65 with P = 62, m = 64, and N = 1 with P = 1
g      two calls give the same bits, and ``F`` equals ``F.T``
h      ``order=perm`` on ``(x, yerr, rows)`` against ``order=None`` on the permuted inputs, and ``order="coordinate"``: bits
i      ``GP`` with a fitted mean, fitted white noise and a partly frozen kernel: layout mean | white noise | kernel, the kernel
       block the restatement's, the mean block ``mg Q mg^T`` of ``vecchia_ref``, cross blocks 0; ``parameter_covariance``
       inverts it.  Without ``VecchiaSolver.fisher_blocks`` ``GP`` falls back to NumPy on ``get_inverse()`` -- N x N, and
       ``1/2 tr(Q D_a Q D_b)``, which is not this quantity -- and the test fails.
j      the C entry with ``diag_rows`` and ``out`` in device memory: the bits of the host-pointer call
=====  =================================================================================================================

Tolerances: the rule of tests/vecchia_cases.py as ``vecchia_fisher_ref.bound`` applies it -- ``1000 x`` the gap, over
``S_ab = sqrt(F_aa F_bb)``, of the two CPU routes (the restatement with every predecessor in the set, and the dense long-double
reference) on the first 150 points of the test's own inputs, at least ``4 eps``, the gap asserted below 1e-9 -- and an entry whose
scale is zero must be exactly zero.  tests/test_vecchia_fisher_host.py shows that the bound rejects a missing mean term, a missing
1/2, a dropped last slot and unpermuted diagonal rows on these problems.  The module prints its largest error / bound per group
at the end (``-s``).  Seen on one MI355X: a 0.0043 (P = 1, m = 64), b 0.0056 (against ``BasicSolver.fisher``, P = 17), c 0.0016,
d 0.0026, e 0.0037 (N = 4099: 7.1e-15 of 1.9e-12), f 0.0017, h 0.0007, i 0.0014 (1.8e-14 of 1.3e-11); g, j and the rest of c, d
and h compare bits.  No case came near its bound.  33 tests in 5 s, none above 0.8 s, the CPU restatement included.
"""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

from george_amd import GP, BasicSolver, VecchiaSolver
from george_amd import _native as N
from george_amd.solvers.vecchia import vecchia_neighbors

import fisher_ref
import vecchia_cases as VC
import vecchia_fisher_ref as VF
import vecchia_ref
from test_gpu_fisher import LinearMean, NoiseRamp
from test_gpu_grad_reference import _masks
from vecchia_cases import LOG, _check

pytestmark = pytest.mark.gpu

MARGINS = {}             # group -> (largest error / bound seen, the quantity, the test)
M = pytest.mark.parametrize("m", [7, 64])


@pytest.fixture(autouse=True)
def _note_margins(request):
    start = len(LOG)
    yield
    group = request.node.name[len("test_")]
    MARGINS[group] = max([MARGINS.get(group, (0.0, "", ""))] + [(ratio, what.strip(), request.node.name) for what, ratio in LOG[start:]])


@pytest.fixture(scope="module", autouse=True)
def _report_margins_and_clear():
    yield
    for group in sorted(MARGINS):
        print("group %s: largest error / bound %.3g  (%s of %s)" % ((group,) + MARGINS[group]))
    VF.clear()
    VC.clear()
    VecchiaSolver.release_pool()
    BasicSolver.release_pool()


def _solver(case, n, m):
    kernel, x, yerr, rows = VF.problem(case, n)
    ref, nbr = VF.cached(case, n, m)
    s = VecchiaSolver(kernel, m=m, neighbors=nbr)
    s.compute(x, yerr)
    return s, rows, ref


def _fisher(s, rows, ref, bound, what="fisher"):
    F = s.fisher_blocks(diag_rows=rows)
    _check(what, F, ref.F, bound, scale=ref.S)
    assert np.array_equal(F, F.T)
    return F


# ------------------------------------------------------------------ a. the kernel table
@M
@pytest.mark.parametrize("case", VF.CASES)
def test_a_kernel_table(case, m):
    kernel, x, yerr, rows = VF.problem(case)
    print("LDS of the information kernel: %d bytes" % VF.fisher_lds_bytes(m, x.shape[1], len(kernel), 2 + len(kernel)))
    s, rows, ref = _solver(case, 300, m)
    F = _fisher(s, rows, ref, VF.bound(case))
    assert F.shape == (2 + len(kernel), 2 + len(kernel)) and np.all(np.diag(F) > 0.0)


# ------------------------------------------------------------------ b. full conditioning
@pytest.mark.parametrize("case", [5, 17, 62])
def test_b_full_conditioning_is_the_dense_information(case):
    n = 65
    kernel, x, yerr, rows = VF.problem(case, n)
    bound = VF.bound(case, n)
    dense = fisher_ref.reference(kernel, x, yerr, rows)
    s = VecchiaSolver(kernel, m=64)
    s.compute(x, yerr)
    assert np.array_equal(s._default_table(x)[n - 1], np.arange(64))
    F = s.fisher_blocks(diag_rows=rows)
    _check("against the dense reference", F, dense.F, bound, scale=dense.S)
    b = BasicSolver(kernel)
    b.compute(x, yerr)
    _check("against BasicSolver.fisher", F, b.fisher(diag_rows=rows), bound, scale=dense.S)


# ------------------------------------------------------------------ c. the 64 KB switch
@pytest.mark.parametrize("m", [8, 9])
def test_c_both_sides_of_the_lds_switch(m):
    lds = VF.fisher_lds_bytes(m, 16, 62, 64)
    assert (lds <= 64 * 1024) == (m == 8) and lds <= VF.V_FISHER_LDS
    s, rows, ref = _solver(62, 300, m)
    _fisher(s, rows, ref, VF.bound(62))


def test_c_the_raised_limit_and_back_gives_the_same_bits():
    runs = []
    for m in (64, 7, 64):
        s, rows, ref = _solver(62, 300, m)
        runs.append(_fisher(s, rows, ref, VF.bound(62)))
        del s
    assert np.all(np.isfinite(runs[0])) and np.array_equal(runs[0], runs[2])
    assert not np.array_equal(runs[0], runs[1])


# ------------------------------------------------------------------ d. masks and plane counts
@pytest.mark.parametrize("P", [5, 17, 62])
def test_d_masks_zero_rows_and_columns_and_leave_the_rest_bitwise(P):
    s, rows, ref = _solver(P, 300, 7)
    full = _fisher(s, rows, ref, VF.bound(P))
    for name, mask in _masks(P).items():
        F = s.fisher_blocks(which=mask.astype(np.uint32), diag_rows=rows)
        keep = np.concatenate([[0, 1], 2 + np.flatnonzero(mask)])
        gone = 2 + np.flatnonzero(~mask)
        assert np.all(F[gone, :] == 0.0) and np.all(F[:, gone] == 0.0), name
        assert np.array_equal(F[np.ix_(keep, keep)], full[np.ix_(keep, keep)]), name
    # no diagonal rows: the kernel block alone; diagonal rows alone (every kernel parameter masked)
    bare = s.fisher_blocks()
    assert bare.shape == (P, P) and np.array_equal(bare, full[2:, 2:])
    only = s.fisher_blocks(which=np.zeros(P, dtype=bool), diag_rows=rows)
    assert np.array_equal(only[:2, :2], full[:2, :2]) and np.all(only[2:] == 0.0) and np.all(only[:, 2:] == 0.0)
    none = s.fisher_blocks(which=np.zeros(P, dtype=bool))
    assert none.shape == (P, P) and np.all(none == 0.0)


def test_d_sixty_four_planes_at_most():
    kernel, x, yerr, r, xs = VC.pcase(64)
    rows = fisher_ref.diag_rows_for(x, yerr)
    s = VecchiaSolver(kernel, m=7)
    s.compute(x, yerr)
    with pytest.raises(ValueError, match="64 planes"):
        s.fisher_blocks(diag_rows=rows)                                           # 66
    one_off = np.ones(64, dtype=bool)
    one_off[3] = False
    with pytest.raises(ValueError, match="64 planes"):
        s.fisher_blocks(which=one_off, diag_rows=rows)                            # 65
    F = s.fisher_blocks(diag_rows=rows[:1], which=one_off)                        # 64: one row and 63 parameters
    assert F.shape == (65, 65) and np.array_equal(F, F.T) and np.all(np.isfinite(F))
    assert np.all(F[1 + 3] == 0.0) and np.all(np.diag(F)[np.arange(65) != 4] > 0.0)
    all64 = s.fisher_blocks()                                                     # 64: every parameter, no row
    keep = np.flatnonzero(one_off)
    assert np.array_equal(all64[np.ix_(keep, keep)], F[1:, 1:][np.ix_(keep, keep)])
    # the contract of BasicSolver.fisher on shapes
    with pytest.raises(ValueError):
        s.fisher_blocks(which=np.ones(65, dtype=bool))
    with pytest.raises(ValueError):
        s.fisher_blocks(diag_rows=rows[:, :-1])
    with pytest.raises(ValueError):
        s.fisher_blocks(diag_rows=rows[0])
    with pytest.raises(RuntimeError, match="compute"):
        VecchiaSolver(kernel, m=7).fisher_blocks()


# ------------------------------------------------------------------ e. more points than workgroups
@pytest.mark.parametrize("n", [4099, 8200])
def test_e_more_points_than_workgroups(n):
    """4096 workgroups: beyond that a workgroup walks several points and its pair sums carry across them"""
    s, rows, ref = _solver(5, n, 7)
    _fisher(s, rows, ref, VF.bound(5, n))


# ------------------------------------------------------------------ f. the smallest N
@pytest.mark.parametrize("case,n", [(62, 1), (62, 2), (62, 64), (62, 65), (1, 1)])
def test_f_smallest_n(case, n):
    """m = 64.  N = 1: one block of one entry, no neighbour, no substitution; zero where the scale is (a metric's derivative at
    distance 0)"""
    kernel, x, yerr, rows = VF.problem(case, n)
    s, rows, ref = _solver(case, n, 64)
    if (case, n) == (62, 1):
        assert np.sum(np.diag(ref.S) == 0.0) >= 50
    F = _fisher(s, rows, ref, VF.bound(case, n))
    assert F.shape == (2 + len(kernel), 2 + len(kernel))


# ------------------------------------------------------------------ g. determinism
def test_g_two_calls_give_the_same_bits():
    s, rows, ref = _solver(17, 300, 64)
    a = s.fisher_blocks(diag_rows=rows)
    b = s.fisher_blocks(diag_rows=rows)
    assert np.array_equal(a, b) and np.array_equal(a, a.T) and np.all(np.isfinite(a))
    s2, _, _ = _solver(17, 300, 64)                                        # another solver, another handle
    assert np.array_equal(s2.fisher_blocks(diag_rows=rows), a)


# ------------------------------------------------------------------ h. ordering
def test_h_order_permutes_the_diagonal_rows_with_the_points():
    kernel, x, yerr, rows = VF.problem(5)
    n = len(x)
    plain = VecchiaSolver(kernel, m=7)
    plain.compute(x, yerr)
    want = plain.fisher_blocks(diag_rows=rows)
    assert np.ptp(rows[1]) > 0.0                                           # (a row that varies: its order matters)
    perm = np.random.RandomState(3).permutation(n)
    inv = np.argsort(perm)
    # the caller holds the points shuffled (position perm[k] of the caller's arrays is solver position k)
    xc, yc, rc = x[inv], yerr[inv], rows[:, inv]
    assert np.array_equal(xc[perm], x)
    s = VecchiaSolver(kernel, m=7, order=perm)
    s.compute(xc, yc)
    assert np.array_equal(s.fisher_blocks(diag_rows=rc), want)
    assert not np.array_equal(s.fisher_blocks(diag_rows=rows), want)
    # order="coordinate": a stable argsort of the first column brings the shuffled points back (the column has no ties)
    assert len(np.unique(x[:, 0])) == n
    s = VecchiaSolver(kernel, m=7, order="coordinate")
    s.compute(xc, yc)
    assert np.array_equal(s.fisher_blocks(diag_rows=rc), want)
    ref, _ = VF.cached(5, 300, 7)
    _check("order=perm", s.fisher_blocks(diag_rows=rc), ref.F, VF.bound(5), scale=ref.S)


# ------------------------------------------------------------------ i. through GP
def _mean_block_gap(kernel, x, yerr, mg):
    """the two CPU routes for ``mg K^-1 mg^T`` on these inputs: the restatement with every predecessor, and LAPACK"""
    n = len(x)
    K = np.array(VF.solver_np.kernel_matrix(kernel, x))
    K[np.diag_indices(n)] += yerr ** 2
    dense = np.dot(mg, cho_solve(cho_factor(K, lower=True), mg.T))
    full = vecchia_ref.reference(kernel, x, yerr, VF.full_table(n))
    d = np.sqrt(np.diag(dense))
    return VC._over(np.dot(mg, full.apply_q(mg.T)) - dense, np.outer(d, d))


def test_i_through_gp():
    n, m = 300, 32
    kernel, x, yerr, _ = fisher_ref.problem("hyper", n)
    kernel.freeze_parameter("k1:k1:k1:k2:metric:log_M_0_0")
    t = x[:, 0]
    a, c = np.log(0.5 * np.min(yerr ** 2)), 0.1
    wn = np.exp(a + c * t)
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=a, c=c), fit_white_noise=True, solver=VecchiaSolver, m=m)
    gp.compute(t, yerr)
    assert callable(gp.solver.fisher_blocks) and not callable(getattr(gp.solver, "fisher", None))
    F = gp.fisher_information()
    P = len(gp)
    assert F.shape == (P, P) and P == 2 + 2 + 10 and np.array_equal(F, F.T)
    assert np.all(F[:2, 2:] == 0.0) and np.all(F[2:, :2] == 0.0)
    # the kernel block (white noise | kernel) is the restatement's on the effective error bars
    ye, rows = np.sqrt(yerr ** 2 + wn), np.stack([wn, wn * t])
    nbr = vecchia_neighbors(x, m)
    k = VC.GAP_N
    gap = VC._over(VF.reference(kernel, x[:k], ye[:k], VF.full_table(k), rows[:, :k]).F
                   - fisher_ref.reference(kernel, x[:k], ye[:k], rows[:, :k]).F, fisher_ref.reference(kernel, x[:k], ye[:k], rows[:, :k]).S)
    print("gap of the two CPU routes: %.1e" % gap)
    assert gap <= VF.GAP_CAP
    ref = VF.reference(kernel, x, ye, nbr, rows, which=kernel.unfrozen_mask)
    keep = np.concatenate([[0, 1], 2 + np.flatnonzero(kernel.unfrozen_mask)])
    _check("GP: white noise | kernel", F[2:, 2:], ref.F[np.ix_(keep, keep)], 1000.0 * max(gap, 4 * VF.EPS), scale=ref.S[np.ix_(keep, keep)])
    # the mean block is mg Q mg^T
    mg = np.stack([t, np.ones_like(t)])
    mgap = _mean_block_gap(kernel, x[:k], ye[:k], mg[:, :k])
    print("gap of the two CPU routes, mean block: %.1e" % mgap)
    assert mgap <= VF.GAP_CAP
    want = np.dot(mg, vecchia_ref.reference(kernel, x, ye, nbr).apply_q(mg.T))
    d = np.sqrt(np.diag(want))
    _check("GP: mean block", F[:2, :2], 0.5 * (want + want.T), 1000.0 * max(mgap, 4 * VF.EPS), scale=np.outer(d, d))
    # the Cramer-Rao covariance
    C = gp.parameter_covariance()
    kappa_F = np.linalg.cond(F)
    resid = np.max(np.abs(np.dot(C, F) - np.eye(P)))
    print("kappa(F) %.3g, |C F - I| %.3g" % (kappa_F, resid))
    assert C.shape == (P, P) and np.array_equal(C, C.T) and resid <= kappa_F * 1e-12 and np.all(np.diag(C) > 0.0)


# ------------------------------------------------------------------ j. device pointers
def test_j_device_pointers_give_the_bits_of_host_pointers():
    import torch
    s, rows, ref = _solver(5, 300, 7)
    want = s.fisher_blocks(diag_rows=rows)
    P = len(want)
    which = np.ones(5, dtype=np.uint32)
    d_rows = torch.from_numpy(rows).to("cuda")
    d_out = torch.full((P, P), float("nan"), dtype=torch.float64, device="cuda")
    N.check(N.lib.gh_vecchia_fisher(s._handle, s._dk.handle, N.ptr(which), d_rows.data_ptr(), 2, d_out.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(d_rows.cpu().numpy(), rows)
    mixed = np.full((P, P), np.nan)
    N.check(N.lib.gh_vecchia_fisher(s._handle, s._dk.handle, N.ptr(which), d_rows.data_ptr(), 2, N.ptr(mixed)))
    assert np.array_equal(mixed, want)
    # the native argument checks: rows announced but not given, a negative count
    with pytest.raises(ValueError):
        N.check(N.lib.gh_vecchia_fisher(s._handle, s._dk.handle, N.ptr(which), None, 2, N.ptr(mixed)))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_vecchia_fisher(s._handle, s._dk.handle, N.ptr(which), None, -1, N.ptr(mixed)))
