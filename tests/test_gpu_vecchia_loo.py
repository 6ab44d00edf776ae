"""``VecchiaSolver.loo_blocks`` on the device (gh_vecchia_loo: ``vecchia_qdiag_kernel``, ``vecchia_loo_point_kernel`` and
``vecchia_loo_grad_kernel`` of george_amd/csrc/gh_vecchia.hip) against the NumPy restatement of tests/vecchia_loo_ref.py, and
``GP.loo_predict`` / ``loo_log_likelihood`` / ``grad_loo_log_likelihood`` / ``loo_nll_and_grad`` through it.

=====  =================================================================================================================
group  what
=====  =================================================================================================================
a      full conditioning, N = 65 and m = 64: against ``BasicSolver.loo`` on the same device and the dense reference
b      the restatement at N = 777 (no multiple of any launch size; the first m rows have short lists) for m = 1 / 7 / 32 / 64
       in 1-D and 3-D; an irregular table in which point 0 is a neighbour of every row and a third of the points nobody's
       (the longest and the empty gather columns); the interpreter path with the eleven-parameter composite
c      P = 64 in 16-D on both sides of the 64 KB switch of the gradient kernels' LDS: m = 57, 58, 64
d      masks: masked slots exactly 0, the others the bits of the unmasked call; ``which=None``: no gradient parts, the bits of
       the gradient path's values
e      N = 1, 2 and 4099 (more points than the 4096 workgroups of the gradient kernel)
f      ``order=`` a permutation and ``"coordinate"``: the bits of the unpermuted call, in the caller's order
g      two calls, a second solver, and a solver that picks up the handle the pool kept: the same bits
h      another kernel than ``compute``'s under which some blocks do not factor: they add nothing
i      through ``GP`` with a fitted linear mean and a fitted white-noise model, against the restatement assembled by
       ``GP._assemble_grad``.  Without ``VecchiaSolver.loo_blocks`` ``GP`` asks ``get_inverse()`` for an N x N array.
j      one call at N = 20 011, m = 32 (the generic branch would start from a 3.2 GB identity): the values
=====  =================================================================================================================

Tolerances: the rule of tests/vecchia_cases.py as ``vecchia_loo_ref.tolerances`` applies it -- per quantity ``1000 x`` the gap of
the two CPU routes (the restatement with every predecessor in the set, and the dense leave-one-out by LAPACK) on the first 150
points of the test's own inputs, at least ``4 eps``, no bound above 1e-9, the gap asserted below 1e-9; vectors over their largest
entry, the gradient over ``S``.  tests/test_vecchia_loo_host.py holds the restatement to central differences and to the dense
reference, and these problems to the cap.  Every comparison prints its error and bound (``-s``).  Seen on one MI355X: the largest
error / bound is 0.0076 (``L`` at full conditioning, N = 65: 2.2e-14 of 2.9e-12), the kernel gradient at most 3.2e-15 of ``S``
against 2.3e-12 (the composite kernel); d, f, g and parts of c and j compare bits.  30 tests in 4.9 s, none above 1.1 s, the CPU
restatement included.
"""
import functools

import numpy as np
import pytest

from george_amd import GP, BasicSolver, VecchiaSolver, kernels
from george_amd import _native as N
from george_amd.solvers.protocol import DeviceKernel
from george_amd.solvers.vecchia import vecchia_neighbors

import loo_ref
import vecchia_cases as VC
import vecchia_loo_ref as VL
from test_gpu_fisher import LinearMean, NoiseRamp
from test_gpu_grad_reference import _masks
from test_gpu_vecchia import _problem
from vecchia_cases import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _clear():
    yield
    for f in (_tol, _ref):
        f.cache_clear()
    VC.clear()
    VecchiaSolver.release_pool()
    BasicSolver.release_pool()


def _inputs(name, n):
    """(kernel, x, yerr, r): the problems of tests/test_gpu_vecchia.py, or -- an integer name -- of tests/vecchia_cases.py"""
    if isinstance(name, int):
        return VC.pcase(name, n)[:4]
    return _problem(name, n, 250.0 if n > 10000 else 10.0)[:4]


@functools.lru_cache(maxsize=None)
def _tol(name, n):
    return VL.tolerances(*_inputs(name, n))


@functools.lru_cache(maxsize=None)
def _ref(name, n, m, table="default", want_grad=True):
    kernel, x, yerr, r = _inputs(name, n)
    nbr = vecchia_neighbors(x, m) if table == "default" else VL.irregular_table(n, m)
    return VL.reference(kernel, x, yerr, nbr, r, want_grad=want_grad), nbr


def _solver(name, n, m, table="default", **kw):
    kernel, x, yerr, r = _inputs(name, n)
    s = VecchiaSolver(kernel, m=m, neighbors=None if table == "default" else VL.irregular_table(n, m), **kw)
    s.compute(x, yerr)
    return s, r, np.ones(len(kernel), dtype=np.uint32)


def _same(a, b):
    assert len(a) == len(b) == 7
    for p, q in zip(a, b):
        assert np.all(np.isfinite(p)) and np.array_equal(p, q)


# ------------------------------------------------------------------ a. full conditioning
@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_a_full_conditioning_is_the_dense_leave_one_out(name):
    n = 65
    kernel, x, yerr, r = _inputs(name, n)
    tol = _tol(name, n)
    s, r, ones = _solver(name, n, 64)
    assert np.array_equal(s._default_table(x)[n - 1], np.arange(64))
    got = s.loo_blocks(r, ones)
    b = BasicSolver(kernel)
    b.compute(x, yerr)
    L, resid, var, lpd, g, v, diagB = b.loo(r, ones)
    full = VL.reference(kernel, x, yerr, VL.full_table(n), r)
    _check("BasicSolver.loo: L", got[0], L, tol["L"])
    for what, val, want in (("resid", got[1], resid), ("var", got[2], var), ("lpd", got[3], lpd), ("v", got[5], v), ("diagB", got[6], diagB)):
        _check("BasicSolver.loo: " + what, val, want, tol[what])
    _check("BasicSolver.loo: kgrad", got[4], g, tol["kgrad"], scale=full.S)
    dense = loo_ref.reference(kernel, x, yerr, r)
    _check("dense reference: kgrad", got[4], dense.g, tol["kgrad"], scale=full.S)
    _check("dense reference: diagB", got[6], dense.diagB, tol["diagB"])
    VL.check("restatement", got, full, tol)


# ------------------------------------------------------------------ b. the restatement
@pytest.mark.parametrize("m", [1, 7, 32, 64])
@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_b_parity_with_the_restatement(name, m):
    s, r, ones = _solver(name, 777, m)
    ref, nbr = _ref(name, 777, m)
    VL.check("m=%d" % m, s.loo_blocks(r, ones), ref, _tol(name, 777))


@pytest.mark.parametrize("name", ["m32_1d", "expsq_3d"])
def test_b_irregular_table_longest_and_empty_columns(name):
    n, m = 777, 24
    ref, nbr = _ref(name, n, m, table="irregular")
    cols = np.bincount(nbr[nbr >= 0], minlength=n)
    assert cols[0] == n - 1 and np.all(cols[2::3] == 0)
    s, r, ones = _solver(name, n, m, table="irregular")
    got = s.loo_blocks(r, ones)
    VL.check("irregular", got, ref, _tol(name, n))
    _check("empty columns: var = f", got[2][2::3], ref.base.f[2::3], _tol(name, n)["var"])


def test_b_interpreter_path():
    """the 17-node composite of docs/tutorials/hyper.rst: no fast form, eleven gradient slots"""
    s, r, ones = _solver("hyper", 300, 16)
    assert len(ones) == 11
    ref, nbr = _ref("hyper", 300, 16)
    VL.check("hyper", s.loo_blocks(r, ones), ref, _tol("hyper", 300))


# ------------------------------------------------------------------ c. the 64 KB switch
@pytest.mark.parametrize("m", [57, 58, 64])
def test_c_both_sides_of_the_lds_switch(m):
    lds = VC.grad_lds_bytes(m, 16, 64)
    assert (lds <= 64 * 1024) == (m == 57) and lds <= VC.V_GRAD_LDS
    s, r, ones = _solver(64, 300, m)
    ref, nbr = _ref(64, 300, m)
    VL.check("P=64 m=%d" % m, s.loo_blocks(r, ones), ref, _tol(64, 300))


def test_c_the_raised_limit_and_back_gives_the_same_bits():
    runs = []
    for m in (64, 7, 64):
        s, r, ones = _solver(64, 300, m)
        runs.append(s.loo_blocks(r, ones))
        del s
    _same(runs[0], runs[2])
    assert not np.array_equal(runs[0][4], runs[1][4])


# ------------------------------------------------------------------ d. masks and values only
@pytest.mark.parametrize("P", [5, 17, 64])
def test_d_masks_zero_frozen_entries_and_leave_the_rest_bitwise(P):
    s, r, ones = _solver(P, 300, 7)
    full = s.loo_blocks(r, ones)
    assert np.any(full[4] != 0.0)
    for name, mask in _masks(P).items():
        got = s.loo_blocks(r, mask.astype(np.uint32))
        assert np.all(got[4][~mask] == 0.0), name
        assert np.array_equal(got[4][mask], full[4][mask]), name
        for k in (0, 1, 2, 3, 5, 6):
            assert np.array_equal(got[k], full[k]), (name, k)


def test_d_values_only():
    s, r, ones = _solver("expsq_3d", 777, 32)
    full = s.loo_blocks(r, ones)
    vals = s.loo_blocks(r)
    assert vals[4] is None and vals[5] is None and vals[6] is None
    for k in range(4):
        assert np.array_equal(vals[k], full[k])
    assert isinstance(vals[0], float) and vals[1].shape == vals[2].shape == vals[3].shape == (777,)
    VL.check("values only", vals, _ref("expsq_3d", 777, 32)[0], _tol("expsq_3d", 777))
    with pytest.raises(ValueError):
        s.loo_blocks(r, np.ones(len(ones) + 1))
    with pytest.raises(ValueError):
        s.loo_blocks(r[:-1])
    # the native argument checks: gradient outputs without a mask, a mask without the gradient, no residual
    import ctypes
    total, buf = ctypes.c_double(0.0), np.empty(777)
    args = (s._handle, s._dk.handle)
    for which, rr, grad, v in ((None, r, np.empty(4), None), (None, r, None, buf), (ones, r, None, None), (ones, None, np.empty(4), None)):
        with pytest.raises(ValueError):
            N.check(N.lib.gh_vecchia_loo(*args, N.ptr(which), N.ptr(rr), ctypes.byref(total), N.ptr(buf), N.ptr(buf), None, N.ptr(grad),
                                         N.ptr(v), None))


# ------------------------------------------------------------------ e. the smallest N, and more points than workgroups
@pytest.mark.parametrize("name,n,m", [("expsq_3d", 1, 64), ("expsq_3d", 2, 64), ("m32_1d", 1, 1), ("m32_1d", 4099, 7)])
def test_e_smallest_n_and_more_points_than_workgroups(name, n, m):
    s, r, ones = _solver(name, n, m)
    ref, nbr = _ref(name, n, m)
    got = s.loo_blocks(r, ones)
    assert got[1].shape == got[5].shape == got[6].shape == (n,) and got[4].shape == (len(ones),)
    VL.check("N=%d" % n, got, ref, _tol(name, n))


# ------------------------------------------------------------------ f. ordering
def test_f_order_returns_the_callers_order():
    kernel, x, yerr, r = _inputs("expsq_3d", 777)
    s, r, ones = _solver("expsq_3d", 777, 7)
    want = s.loo_blocks(r, ones)
    n = len(x)
    perm = np.random.RandomState(3).permutation(n)
    inv = np.argsort(perm)
    xc, yc, rc = x[inv], yerr[inv], r[inv]                                 # the caller holds the points shuffled
    assert np.array_equal(xc[perm], x)
    s2 = VecchiaSolver(kernel, m=7, order=perm)
    s2.compute(xc, yc)
    assert len(np.unique(x[:, 0])) == n
    s3 = VecchiaSolver(kernel, m=7, order="coordinate")
    s3.compute(xc, yc)
    for sol in (s2, s3):
        got = sol.loo_blocks(rc, ones)
        assert got[0] == want[0] and np.array_equal(got[4], want[4])
        for k in (1, 2, 3, 5, 6):
            assert np.array_equal(got[k], want[k][inv]) and not np.array_equal(got[k], want[k])
        vals = sol.loo_blocks(rc)
        for k in (1, 2, 3):
            assert np.array_equal(vals[k], want[k][inv])


# ------------------------------------------------------------------ g. determinism
def test_g_same_bits_again_on_a_second_solver_and_on_a_handle_from_the_pool():
    s, r, ones = _solver("hyper", 300, 16)
    a = s.loo_blocks(r, ones)
    _same(a, s.loo_blocks(r, ones))
    s2, _, _ = _solver("hyper", 300, 16)                                  # another solver, another handle, both alive
    assert s2._handle != s._handle
    _same(a, s2.loo_blocks(r, ones))
    del s, s2
    s3, _, _ = _solver("hyper", 300, 16)                                  # picks up a handle the pool kept
    _same(a, s3.loo_blocks(r, ones))
    vals = s3.loo_blocks(r)
    assert vals[0] == a[0] and np.array_equal(vals[3], a[3])


# ------------------------------------------------------------------ h. a block that does not factor
def test_h_a_block_that_fails_under_another_kernel_adds_nothing():
    """``compute`` with a Matern kernel and NO error bar at five points; then the C entry with a narrow ``LocalGaussianKernel``,
    ``phi(x) phi(y)``: away from its location ``phi`` underflows to an exact 0, so a block that holds one of the five points has
    an exact zero pivot -- those blocks add nothing and write zeros -- while the blocks near the location factor and count."""
    import ctypes
    n, m = 300, 7
    kernel, x, yerr, r = _inputs("m32_1d", n)
    yerr = yerr.copy()
    bare = np.array([3, 40, 41, 150, 299])
    yerr[bare] = 0.0
    other = kernels.LocalGaussianKernel(location=float(x[100, 0]), log_width=np.log(1e-3))
    assert np.all(np.abs(x[bare, 0] - x[100, 0]) > 1.3)
    nbr = vecchia_neighbors(x, m)
    ref = VL.reference(kernel, x, yerr, nbr, r, block_spec=other)
    hit = np.array([i for i in range(n) if np.intersect1d(np.concatenate([nbr[i][nbr[i] >= 0], [i]]), bare).size])
    assert sorted(ref.failed) == sorted(hit) and 5 < len(hit) < 60 and np.all(ref.S > 0.0)
    s = VecchiaSolver(kernel, m=m)
    s.compute(x, yerr)
    dk = DeviceKernel(other)
    total, g = ctypes.c_double(0.0), np.full(2, np.nan)
    resid, var, lpd, v, diagB = (np.empty(n) for _ in range(5))
    ones = np.ones(2, dtype=np.uint32)
    N.check(N.lib.gh_vecchia_loo(s._handle, dk.handle, N.ptr(ones), N.ptr(r), ctypes.byref(total), N.ptr(resid), N.ptr(var), N.ptr(lpd),
                                 N.ptr(g), N.ptr(v), N.ptr(diagB)))
    tol = VL.tolerances(kernel, x, yerr, r)
    VL.check("another kernel", (total.value, resid, var, lpd, g, v, diagB), ref, tol)
    assert np.all(diagB[bare] == 0.0) and np.any(g != 0.0)
    # and the solver's own kernel afterwards: every block factors again
    VL.check("own kernel", s.loo_blocks(r, np.ones(len(kernel), dtype=np.uint32)), VL.reference(kernel, x, yerr, nbr, r), tol)


# ------------------------------------------------------------------ i. through GP
def test_i_through_gp():
    n, m = 300, 32
    _, x, yerr, y = _inputs("hyper", n)
    kernel = loo_ref.kernel_hyper()                                        # (a kernel of its own: one parameter is frozen below)
    kernel.freeze_parameter("k1:k1:k1:k2:metric:log_M_0_0")
    t = x[:, 0]
    a, c = np.log(0.5 * np.min(yerr ** 2)), 0.1
    wn = np.exp(a + c * t)
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=a, c=c), fit_white_noise=True, solver=VecchiaSolver, m=m)
    gp.compute(t, yerr)
    assert callable(gp.solver.loo_blocks) and not callable(getattr(gp.solver, "loo", None))
    ye = np.sqrt(yerr ** 2 + wn)
    r = y - (0.25 * t - 0.8)
    tol = VL.tolerances(kernel, x, ye, r)
    ref = VL.reference(kernel, x, ye, vecchia_neighbors(x, m), r)
    mu, var = gp.loo_predict(y)
    _check("GP: loo_predict mean (resid)", y - mu, ref.resid, tol["resid"])
    _check("GP: loo_predict var", var, ref.var, tol["var"])
    _check("GP: pointwise", gp.loo_log_likelihood(y, pointwise=True), ref.lpd, tol["lpd"])
    _check("GP: loo_log_likelihood", gp.loo_log_likelihood(y), ref.L, tol["L"])
    g = gp.grad_loo_log_likelihood(y)
    mask = kernel.unfrozen_mask
    want = gp._assemble_grad(ref.v, ref.diagB, ref.kgrad[mask], False, diag_weight=1.0)
    assert g.shape == want.shape == (2 + 2 + 10,)
    # a sum_j d_j z_j carries at most (the error of z over its largest entry) x max|z| sum_j |d_j|
    mg, wg = np.stack([t, np.ones(n)]), np.stack([wn, wn * t])
    _check("GP: gradient, mean", g[:2], want[:2], tol["v"], scale=np.max(np.abs(ref.v)) * np.sum(np.abs(mg), axis=1))
    _check("GP: gradient, white noise", g[2:4], want[2:4], tol["diagB"], scale=np.max(np.abs(ref.diagB)) * np.sum(np.abs(wg), axis=1))
    _check("GP: gradient, kernel", g[4:], want[4:], tol["kgrad"], scale=ref.S[mask])
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector(), y)
    _check("GP: loo_nll_and_grad value", val, -ref.L, tol["L"])
    assert np.array_equal(grad, -g)


# ------------------------------------------------------------------ j. where the generic branch cannot go
def test_j_twenty_thousand_points():
    """N = 20 011, 1-D, m = 32: ``apply_inverse(np.eye(N))`` would be 3.2 GB going in and 3.2 GB coming out"""
    n, m = 20011, 32
    s, r, ones = _solver("m32_1d", n, m)
    ref, nbr = _ref("m32_1d", n, m, want_grad=False)
    vals = s.loo_blocks(r)
    VL.check("N=20011", vals, ref, _tol("m32_1d", n))
    full = s.loo_blocks(r, ones)
    for k in range(4):
        assert np.array_equal(vals[k], full[k])
    assert np.all(np.isfinite(full[4])) and np.all(np.isfinite(full[5])) and np.all(np.isfinite(full[6]))
