"""``VecchiaSolver`` on the device (george_amd/csrc/gh_vecchia.hip) against the NumPy restatements (tests/vecchia_ref.py,
tests/vecchia_local_ref.py) at the parameter counts, dimensions, LDS sizes and edges that tests/test_gpu_vecchia.py,
test_gpu_vecchia_local.py and test_gpu_vecchia_search.py do not reach: those run four kernels, at most 3-D and 11 parameters.

``vecchia_grad_kernel`` sizes its dynamic LDS as ``v_lds_doubles(m, ndim, gp)`` with ``gp = (P + 16) | 1`` doubles a lane -- the
gradient row and the evaluator's work space, whose runtime-indexed temporaries live there and not in registers.  Above 64 KB the
host raises the kernel's limit first.  ``vecchia_cases.grad_lds_bytes`` restates the size; tests/test_vecchia_grad_host.py
holds it to this table and to the constants of the sources.

=====================  ====  =================  ================
kernel                 ndim  LDS bytes, m = 64  LDS bytes, m = 7
=====================  ====  =================  ================
P = 1                  1     29 232             10 312
P = 4                  3     32 320             12 488
P = 5                  2     31 800             12 424
P = 16                 4     38 984             18 696
P = 17 (same pitch)    4     38 984             18 696
P = 20, stack depth 8  16    47 272             21 512
P = 37                 16    55 464             29 704
P = 64 (all 64 lanes)  16    69 800 (raised)    44 040
=====================  ====  =================  ================

=====  =================================================================================================================
group  what
=====  =================================================================================================================
a      every kernel of the table at N = 300 with m = 7 and m = 64: log-determinant, ``dot_solve``, ``apply_inverse`` (1 and 5
       columns, in place and not), ``grad`` (kernel part over ``S``, ``alpha``, ``diagA``), ``predict`` (mean, variance,
       covariance at 7 points)
b      the 64 KB switch with P = 64 in 16-D: m = 57 (65 240 bytes, the largest below), m = 58 (65 864, the smallest above),
       m = 64; then m = 64, m = 7, m = 64 again: the two m = 64 gradients agree bit for bit
c      masks at P = 5 / 17 / 64, m = 7: masked slots exactly 0, kept slots the bits of the all-ones call
d      more points than workgroups, P = 5 in 2-D, m = 7: N = 4099 (three workgroups walk two points) and N = 8200 (every
       workgroup walks two, eight walk three)
e      N = 1 / 2 / 64 / 65 with P = 64, m = 64, and N = 1 with P = 1: no neighbour at all, an empty transposed index, a
       triangle of one entry; where ``S`` is zero the gradient is exactly zero
f      ``predict_local`` beyond 3-D: P = 16 (4-D), P = 20 / 37 / 64 (16-D) with mq = 1 / 7 / 64, host and device search
=====  =================================================================================================================

Tolerances: the rule of tests/test_gpu_vecchia.py as ``vecchia_cases.tolerances`` applies it -- ``1000 x`` the gap of the two
CPU routes on the first 150 points of the test's own inputs, at least ``4 eps``, capped -- and for (f) the rule of
tests/test_gpu_vecchia_local.py on the first 64 points.  tests/test_vecchia_grad_host.py shows that the gradient's bound
rejects a dropped pair, a short last chunk, a shifted slot and a wrong weight on these problems.  (b) and (c) also compare bits.
The largest error / bound seen on one MI355X, per group (the module prints its own at the end with ``-s``):

=====  =============  =================================================================================================
group  error / bound  the quantity
=====  =============  =================================================================================================
a      0.031          the covariance at P = 16, m = 64: 2.5e-13 of 8.2e-12; the kernel gradient at most 2.8e-16 of ``S``
                      against 8.9e-13 (0.00031)
b      0.00057        ``dot_solve`` at m = 64, 1.9e-15 of 3.3e-12; then bits
c      bits           --
d      0.00099        the kernel gradient at N = 8200, 8.8e-16 of ``S`` against 8.9e-13
e      0.0025         the variance at N = 65, 3.0e-15 of 1.2e-12; the kernel gradient at most 1.3e-15 of ``S`` (N = 1, P = 1)
f      0.033          the variance at P = 16, mq = 64: 2.9e-14 of 8.9e-13; tables and bits equal on both searches
=====  =============  =================================================================================================

No case came near its bound, and none showed a defect of the device code.  Running time on one MI355X, the CPU restatement
included: 42 tests in 3.9 s, none above 0.7 s.
"""
import functools

import numpy as np
import pytest

from george_amd import VecchiaSolver
from george_amd.solvers.vecchia import vecchia_query_neighbors

import test_gpu_vecchia_local as TL
import vecchia_cases as VC
import vecchia_local_ref
from test_gpu_grad_reference import _masks
from vecchia_cases import LOG, _check, check_grad, check_predict, check_solves

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
    VC.clear()
    _local_tol.cache_clear()
    VecchiaSolver.release_pool()


def _solver(case, n, m):
    kernel, x, yerr, r, xs = VC.pcase(case, n)
    ref, nbr = VC.reference(case, n, m)
    s = VecchiaSolver(kernel, m=m, neighbors=nbr)
    s.compute(x, yerr)
    return s, ref


# ------------------------------------------------------------------ a. parameter count x dimension
@M
@pytest.mark.parametrize("case", VC.PCASE_NAMES)
def test_a_parameter_count_and_dimension(case, m):
    kernel, x, yerr, r, xs = VC.pcase(case)
    tol = VC.tolerances(case)
    print("LDS of the gradient kernel: %d bytes" % VC.grad_lds_bytes(m, x.shape[1], len(kernel)))
    s, ref = _solver(case, 300, m)
    check_solves(s, r, ref, tol)
    check_grad(s, r, ref, tol)
    check_predict(s, kernel, r, xs, ref, tol)


# ------------------------------------------------------------------ b. the 64 KB switch
@pytest.mark.parametrize("m", [57, 58, 64])
def test_b_both_sides_of_the_lds_switch(m):
    kernel, x, yerr, r, xs = VC.pcase(64)
    lds = VC.grad_lds_bytes(m, 16, 64)
    assert (lds <= 64 * 1024) == (m == 57) and lds <= VC.V_GRAD_LDS
    tol = VC.tolerances(64)
    s, ref = _solver(64, 300, m)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    check_grad(s, r, ref, tol)


def test_b_the_raised_limit_and_back_gives_the_same_bits():
    """m = 64 (raised limit), m = 7, m = 64 again: the header of gh_vecchia.hip promises "two calls give the same bits" """
    kernel, x, yerr, r, xs = VC.pcase(64)
    tol = VC.tolerances(64)
    runs = []
    for m in (64, 7, 64):
        s, ref = _solver(64, 300, m)
        runs.append(check_grad(s, r, ref, tol))
        del s
    for a, b in zip(runs[0], runs[2]):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert not np.array_equal(runs[0][0], runs[1][0])


# ------------------------------------------------------------------ c. masks
@pytest.mark.parametrize("P", [5, 17, 64])
def test_c_masks_zero_frozen_entries_and_leave_the_rest_bitwise(P):
    kernel, x, yerr, r, xs = VC.pcase(P)
    s, ref = _solver(P, 300, 7)
    g_all, a_all, d_all = s.grad(r, np.ones(P, dtype=np.uint32))
    assert np.any(g_all != 0.0)
    for name, mask in _masks(P).items():
        g, a, d = s.grad(r, mask.astype(np.uint32))
        assert np.all(g[~mask] == 0.0), name
        assert np.array_equal(g[mask], g_all[mask]), name
        assert np.array_equal(a, a_all) and np.array_equal(d, d_all), name


# ------------------------------------------------------------------ d. more points than workgroups
@pytest.mark.parametrize("n", [4099, 8200])
def test_d_more_points_than_workgroups(n):
    """V_GRAD_WGS = 4096 workgroups: beyond that a workgroup walks several points and its sums carry across them"""
    kernel, x, yerr, r, xs = VC.pcase(5, n)
    tol = VC.tolerances(5, n)
    s, ref = _solver(5, n, 7)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    check_grad(s, r, ref, tol)


# ------------------------------------------------------------------ e. the smallest N
@pytest.mark.parametrize("case,n", [(64, 1), (64, 2), (64, 64), (64, 65), (1, 1)])
def test_e_smallest_n(case, n):
    """m = 64.  N = 1: no neighbour, an empty transposed index, a triangle of one entry -- ``alpha`` and ``diagA`` of one
    element, and a gradient that is exactly zero where ``S`` is (61 of the 64 slots of the P = 64 kernel)"""
    kernel, x, yerr, r, xs = VC.pcase(case, n)
    tol = VC.tolerances(case, n)
    s, ref = _solver(case, n, 64)
    if (case, n) == (64, 1):
        assert np.sum(ref.S == 0.0) == 61
    check_solves(s, r, ref, tol)
    g, alpha, diagA = check_grad(s, r, ref, tol)
    assert g.shape == (len(kernel),) and alpha.shape == diagA.shape == (n,)
    check_predict(s, kernel, r, xs, ref, tol, cov=False)


# ------------------------------------------------------------------ f. local prediction beyond 3-D
@functools.lru_cache(maxsize=None)
def _local_tol(case):
    """the rule of tests/test_gpu_vecchia_local.py (its ``_tol``) on these inputs: the first ``GAP_N`` = 64 data points"""
    kernel, x, yerr, r, xs = VC.pcase(case)
    k = TL.GAP_N
    g = vecchia_local_ref.gaps(kernel, x[:k], yerr[:k], r[:k], xs)[0]
    print("gaps", case, g)
    assert max(g.values()) <= VC.GAP_CAP
    return {key: min(1000.0 * max(v, 4 * TL.EPS), TL.CAP) for key, v in g.items()}


@pytest.mark.parametrize("mq", [1, 7, 64])
@pytest.mark.parametrize("case", [16, "deep8", 37, 64])
def test_f_local_prediction_beyond_three_dimensions(case, mq):
    kernel, x, yerr, r, xs = VC.pcase(case)
    tol = _local_tol(case)
    s, _ = _solver(case, 300, 7)
    tab = vecchia_local_ref.query_neighbors(x, xs, mq)
    host = vecchia_query_neighbors(x, xs, mq)
    dev = vecchia_query_neighbors(x, xs, mq, device=0)
    assert np.array_equal(host, tab) and np.array_equal(dev, tab)
    mu0, var0 = vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs, tab)
    mu, var = s.predict_local(kernel, r, xs, return_var=True, m=mq, search="host")
    _check("mq=%d: mean" % mq, mu, mu0, tol["mu"])
    _check("  .. variance", var, var0, tol["var"])
    mu_d, var_d = s.predict_local(kernel, r, xs, return_var=True, m=mq, search="device")
    assert np.array_equal(mu_d, mu) and np.array_equal(var_d, var)
    mu_t, var_t = s.predict_local(kernel, r, xs, return_var=True, m=mq, neighbors=dev)
    assert np.array_equal(mu_t, mu) and np.array_equal(var_t, var)
