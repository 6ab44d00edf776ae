"""``InducingSolver.loo_lowrank`` on the device (gh_inducing_loo: ``ind_loo_point_kernel``, ``ind_loo_diagb_kernel`` and
``ind_loo_zt_kernel`` of george_amd/csrc/gh_inducing.hip, and the gradient reduction it shares with ``gh_inducing_grad``) against
the NumPy restatement of tests/inducing_loo_ref.py, and ``GP.loo_predict`` / ``loo_log_likelihood`` / ``grad_loo_log_likelihood`` /
``loo_nll_and_grad`` through it.

=====  =================================================================================================================
group  what
=====  =================================================================================================================
a      ``u = x`` without jitter, N = m = 300, ``m32_3d``, DTC and FITC: against ``BasicSolver.loo`` on the same device and the
       dense reference
b      the restatement at N = 300, m = 65 for DTC and FITC: 1-D and 3-D, the six-parameter composite with a frozen parameter
       (interpreter path), ``expsq_1d`` under relative jitter 1e-8, and inducing inputs that are no data points
c      strip and tile edges: ``strip_points=128`` at N = 257 (three strips, the last of one point) and N = 256; m = 1, 64, 65,
       128, 129; N = 1; N = 4097 with m = 16 under FITC (a second workgroup of the diagonal term); strips of 128 / 256 / one
d      parameter count and dimension: P = 1 .. 64 in 1 .. 16 dimensions, both sides of the tile kernel's 64 KB LDS switch
e      masks: masked slots exactly 0, the others the bits of the unmasked call; ``which=None``: no gradient parts, the bits of
       the gradient path's values; ``variational=True``: the bits of a ``method="dtc"`` solver
f      two calls, a second solver, a solver that picks up the pooled handle: the same bits; ``gh_inducing_grad``'s three
       results before and after a ``loo_lowrank`` call on the same handle: the same bits
g      through ``GP`` with a fitted linear mean and a fitted white-noise model, against the restatement assembled by
       ``GP._assemble_grad``.  Without ``loo_lowrank`` ``GP`` contracts ``B`` with the derivative of ``K(x, x)``, which is not
       the derivative of the matrix this solver inverts: the kernel gradient is then off by orders of magnitude more than the bound
h      one value-only call at N = 20 011, m = 128 (the generic branch would start from a 3.2 GB identity)
=====  =================================================================================================================

Tolerances: the rule of tests/inducing_cases.py as ``inducing_loo_ref.tolerances`` applies it -- per quantity ``1000 x`` the gap
of the two CPU routes (the low-rank restatement, and the explicit N x N ``C`` by LAPACK) on the first 800 points of the test's own
inputs, at least ``4 eps``, the gap asserted below 1e-9; vectors over their largest entry, the gradient over ``S``.
tests/test_inducing_loo_host.py holds the restatement to central differences and to the dense reference, these problems to the
cap, and shows that the bound rejects every wrong gradient of ``inducing_loo_ref.DEFECTS``.  Every comparison prints its error and
bound (``-s``), and the module prints the largest error / bound per group at the end.  Seen on one MI355X, the largest error /
bound per group: a 0.034 (``var`` against ``BasicSolver.loo``, 9.4e-13 of 2.8e-11), b 0.017, c 0.021, d 0.017, e 0.0046, g 0.13
(``L`` through ``GP``, 1.2e-13 of 9.4e-13), h 0.0040; the kernel gradient at most 4.5e-15 of ``S`` against 8.9e-13 (P = 5); f and
parts of e compare bits.  No case came near its bound.  61 tests in 5.2 s, the CPU restatement included.
"""
import ctypes
import functools
import gc

import numpy as np
import pytest

from george_amd import GP, BasicSolver, InducingSolver
from george_amd import _native as N

import inducing_cases as IC
import inducing_loo_ref as IL
import loo_ref
from inducing_cases import LOG, _check
from test_gpu_fisher import LinearMean, NoiseRamp
from test_gpu_grad_reference import _masks
from test_inducing_loo_host import _case

pytestmark = pytest.mark.gpu

METHOD = pytest.mark.parametrize("method", ["dtc", "fitc"])
MARGINS = {}             # group -> largest error / bound seen


@pytest.fixture(autouse=True)
def _note_margins(request):
    start = len(LOG)
    yield
    group = request.node.name[len("test_")]
    MARGINS[group] = max([MARGINS.get(group, 0.0)] + [ratio for _, ratio in LOG[start:]])


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    for group in sorted(MARGINS):
        print("group %s: largest error / bound %.3g" % (group, MARGINS[group]))
    _bounds.cache_clear()
    InducingSolver.release_pool()
    BasicSolver.release_pool()


@functools.lru_cache(maxsize=None)
def _bounds(name, n, m, inducing, rel_jitter, method, want_grad=True):
    """(inputs, restatement, tolerances) of a named problem; past ``GAP_MAX_N`` points the block-wise route"""
    kernel, x, yerr, r, u = inputs = _pcase(name) if inducing == "pcase" else _case(name, n, m, inducing)
    jitter, tol = IL.tolerances(kernel, x, yerr, u, rel_jitter, method, r, label=str(name))
    ref = IL.reference(kernel, x, yerr, u, jitter, method, r, want_grad=want_grad, route="blocks" if n > IC.GAP_MAX_N else "stacked")
    return inputs, ref, tol


def _pcase(name):
    kernel, x, yerr, r, _, u = IC.pcase(name)
    return kernel, x, yerr, r, u


def _solver(kernel, x, yerr, u, method, rel_jitter=1e-10, strip=0, **kw):
    s = InducingSolver(kernel, inducing=u, method=method, jitter=rel_jitter, strip_points=strip, **kw)
    s.compute(x, yerr)
    return s


def _mask(kernel):
    return kernel.unfrozen_mask.astype(np.uint32)


def _check_loo(what, got, ref, tol, mask=None):
    """``IL.check`` with the frozen slots of the gradient held to exactly 0"""
    if got[4] is not None and mask is not None:
        keep = mask != 0
        assert len(got[4]) == len(keep) and np.all(got[4][~keep] == 0.0)
        want = IL.InducingLooRef()
        want.__dict__.update(ref.__dict__)
        want.kgrad, want.S = ref.kgrad[keep], ref.S[keep]
        got = got[:4] + (got[4][keep],) + got[5:]
        ref = want
    IL.check(what, got, ref, tol)


def _same(a, b):
    assert len(a) == len(b) == 7
    for p, q in zip(a, b):
        assert np.all(np.isfinite(p)) and np.array_equal(p, q)


# ------------------------------------------------------------------ a. u = x: the dense leave-one-out
@METHOD
def test_a_all_points_inducing_is_the_dense_leave_one_out(method):
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 300, 300, "all", 0.0, method)
    s = _solver(kernel, x, yerr, u, method, 0.0)
    ones = np.ones(len(kernel), dtype=np.uint32)
    got = s.loo_lowrank(r, ones)
    _check_loo("restatement", got, ref, tol)
    b = BasicSolver(kernel)
    b.compute(x, yerr)
    L, resid, var, lpd, g, v, diagB = b.loo(r, ones)
    _check("BasicSolver.loo: L", got[0], L, tol["L"])
    for what, val, want in (("resid", got[1], resid), ("var", got[2], var), ("lpd", got[3], lpd), ("v", got[5], v), ("diagB", got[6], diagB)):
        _check("BasicSolver.loo: " + what, val, want, tol[what])
    _check("BasicSolver.loo: kgrad", got[4], g, tol["kgrad"], scale=ref.S)
    dense = loo_ref.reference(kernel, x, yerr, r)
    _check("dense reference: kgrad", got[4], dense.g, tol["kgrad"], scale=ref.S)
    _check("dense reference: diagB", got[6], dense.diagB, tol["diagB"])
    _check("dense reference: resid", got[1], dense.resid, tol["resid"])


# ------------------------------------------------------------------ b. the restatement
@METHOD
@pytest.mark.parametrize("name,inducing,rel_jitter", [("m32_1d", "maxmin", 1e-10), ("m32_3d", "maxmin", 1e-10), ("comp_3d", "maxmin", 1e-10),
                                                      ("expsq_1d", "maxmin", 1e-8), ("m32_3d", "random", 1e-10)])
def test_b_parity_with_the_restatement(name, inducing, rel_jitter, method):
    (kernel, x, yerr, r, u), ref, tol = _bounds(name, 300, 65, inducing, rel_jitter, method)
    s = _solver(kernel, x, yerr, u, method, rel_jitter)
    if name == "comp_3d":
        assert len(kernel.unfrozen_mask) == 6 and not np.all(kernel.unfrozen_mask)
    _check_loo(name, s.loo_lowrank(r, _mask(kernel)), ref, tol, _mask(kernel))


# ------------------------------------------------------------------ c. strip and tile edges
@METHOD
@pytest.mark.parametrize("n", [257, 256])
def test_c_strips_of_128(n, method):
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", n, 65, "maxmin", 1e-10, method)
    runs = []
    for strip in (128, 256, 0):
        print("strip_points", strip)
        s = _solver(kernel, x, yerr, u, method, strip=strip)
        runs.append(s.loo_lowrank(r, _mask(kernel)))
        _check_loo("N=%d" % n, runs[-1], ref, tol)
        _check_loo("N=%d, values" % n, s.loo_lowrank(r), ref, tol)
    for other in runs[1:]:                                                    # the strip size changes rounding only
        _check_loo("strips against one another", other, _view(runs[0], ref.S), tol)


def _view(out, S):
    """the seven outputs of a call as a reference object"""
    v = IL.InducingLooRef()
    v.L, v.resid, v.var, v.lpd, v.kgrad, v.v, v.diagB = out
    v.S = S
    return v


@METHOD
@pytest.mark.parametrize("m", [1, 64, 65, 128, 129])
def test_c_inducing_counts_at_the_tile_edges(m, method):
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 300, m, "maxmin", 1e-10, method)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    _check_loo("m=%d" % m, s.loo_lowrank(r, _mask(kernel)), ref, tol)


@METHOD
def test_c_one_point(method):
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 1, 1, "maxmin", 1e-10, method)
    s = _solver(kernel, x, yerr, u, method)
    got = s.loo_lowrank(r, _mask(kernel))
    assert got[1].shape == got[5].shape == got[6].shape == (1,) and got[4].shape == (len(kernel),)
    _check_loo("N=1", got, ref, tol)


def test_c_a_second_workgroup_of_the_diagonal_term():
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 4097, 16, "maxmin", 1e-10, "fitc")
    s = _solver(kernel, x, yerr, u, "fitc")
    _check_loo("N=4097", s.loo_lowrank(r, _mask(kernel)), ref, tol)


# ------------------------------------------------------------------ d. parameter count and dimension
@METHOD
@pytest.mark.parametrize("case", IC.PCASE_NAMES)
def test_d_parameter_count_and_dimension(case, method):
    (kernel, x, yerr, r, u), ref, tol = _bounds(case, 300, 65, "pcase", 1e-10, method)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    _check_loo("P=%s" % case, s.loo_lowrank(r, _mask(kernel)), ref, tol, _mask(kernel))


# ------------------------------------------------------------------ e. masks, values only, the bound
@METHOD
@pytest.mark.parametrize("P", [5, 17, 64])
def test_e_masks_zero_frozen_entries_and_leave_the_rest_bitwise(P, method):
    kernel, x, yerr, r, u = _pcase(P)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    full = s.loo_lowrank(r, np.ones(P, dtype=np.uint32))
    assert np.any(full[4] != 0.0)
    for name, mask in _masks(P).items():
        got = s.loo_lowrank(r, mask.astype(np.uint32))
        assert np.all(got[4][~mask] == 0.0), name
        assert np.array_equal(got[4][mask], full[4][mask]), name
        for k in (0, 1, 2, 3, 5, 6):
            assert np.array_equal(got[k], full[k]), (name, k)


@METHOD
def test_e_values_only(method):
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 300, 65, "maxmin", 1e-10, method)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    ones = np.ones(len(kernel), dtype=np.uint32)
    full = s.loo_lowrank(r, ones)
    vals = s.loo_lowrank(r)
    assert vals[4] is None and vals[5] is None and vals[6] is None
    for k in range(4):
        assert np.array_equal(vals[k], full[k])
    assert isinstance(vals[0], float) and vals[1].shape == vals[2].shape == vals[3].shape == (300,)
    _check_loo("values only", vals, ref, tol)
    with pytest.raises(ValueError):
        s.loo_lowrank(r, np.ones(len(ones) + 1))
    with pytest.raises(ValueError):
        s.loo_lowrank(r[:-1])
    # the native argument checks: gradient outputs without a mask, a mask without the gradient, no residual
    total, buf = ctypes.c_double(0.0), np.empty(300)
    args = (s._handle, s._dk.handle)
    for which, rr, grad, v in ((None, r, np.empty(4), None), (None, r, None, buf), (ones, r, None, None), (ones, None, np.empty(4), None)):
        with pytest.raises(ValueError):
            N.check(N.lib.gh_inducing_loo(*args, N.ptr(which), N.ptr(rr), ctypes.byref(total), N.ptr(buf), N.ptr(buf), None, N.ptr(grad),
                                          N.ptr(v), None))


def test_e_the_variational_bound_gives_the_bits_of_dtc():
    kernel, x, yerr, r, u = _case("m32_3d", 300, 65)
    ones = np.ones(len(kernel), dtype=np.uint32)
    dtc = _solver(kernel, x, yerr, u, "dtc", strip=128)
    vfe = _solver(kernel, x, yerr, u, "dtc", strip=128, variational=True)
    assert vfe.trace_term > 0.0
    _same(dtc.loo_lowrank(r, ones), vfe.loo_lowrank(r, ones))
    a, b = dtc.loo_lowrank(r), vfe.loo_lowrank(r)
    for k in range(4):
        assert np.array_equal(a[k], b[k])


# ------------------------------------------------------------------ f. determinism
@METHOD
def test_f_same_bits_again_on_a_second_solver_and_on_a_handle_from_the_pool(method):
    kernel, x, yerr, r, u = _case("comp_3d", 300, 65)
    mask = _mask(kernel)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    a = s.loo_lowrank(r, mask)
    _same(a, s.loo_lowrank(r, mask))
    s2 = _solver(kernel, x, yerr, u, method, strip=128)                       # another solver, another handle, both alive
    assert s2._handle != s._handle
    _same(a, s2.loo_lowrank(r, mask))
    del s, s2
    gc.collect()
    s3 = _solver(kernel, x, yerr, u, method, strip=128)                       # picks up a handle the pool kept
    _same(a, s3.loo_lowrank(r, mask))
    vals = s3.loo_lowrank(r)
    assert vals[0] == a[0] and np.array_equal(vals[3], a[3])


@METHOD
def test_f_grad_keeps_its_bits_around_a_loo_call(method):
    kernel, x, yerr, r, u = _case("comp_3d", 300, 65)
    mask = _mask(kernel)
    s = _solver(kernel, x, yerr, u, method, strip=128)
    before = s.grad(r, mask)
    s.loo_lowrank(r, mask)
    after = s.grad(r, mask)
    for p, q in zip(before, after):
        assert np.all(np.isfinite(p)) and np.array_equal(p, q)
    assert np.array_equal(s.apply_inverse(r), before[1])


# ------------------------------------------------------------------ g. through GP
@METHOD
def test_g_through_gp(method):
    n, m = 300, 65
    kernel, x, yerr, y, u = _case("m32_1d", n, m)
    t = x[:, 0]
    a, c = np.log(0.5 * np.min(yerr ** 2)), 0.1
    wn = np.exp(a + c * t)
    gp = GP(kernel, mean=LinearMean(m=0.25, b=-0.8), white_noise=NoiseRamp(a=a, c=c), fit_white_noise=True, solver=InducingSolver,
            inducing=u, method=method)
    gp.compute(t, yerr)
    assert callable(gp.solver.loo_lowrank) and not callable(getattr(gp.solver, "loo", None))
    ye = np.sqrt(yerr ** 2 + wn)
    r = y - (0.25 * t - 0.8)
    jitter, tol = IL.tolerances(kernel, x, ye, u, 1e-10, method, r, label="GP")
    ref = IL.reference(kernel, x, ye, u, jitter, method, r)
    mu, var = gp.loo_predict(y)
    _check("GP: loo_predict mean (resid)", y - mu, ref.resid, tol["resid"])
    _check("GP: loo_predict var", var, ref.var, tol["var"])
    _check("GP: pointwise", gp.loo_log_likelihood(y, pointwise=True), ref.lpd, tol["lpd"])
    _check("GP: loo_log_likelihood", gp.loo_log_likelihood(y), ref.L, tol["L"])
    g = gp.grad_loo_log_likelihood(y)
    want = gp._assemble_grad(ref.v, ref.diagB, ref.kgrad, False, diag_weight=1.0)
    assert g.shape == want.shape == (2 + 2 + 2,)
    # a sum_j d_j z_j carries at most (the error of z over its largest entry) x max|z| sum_j |d_j|
    mg, wg = np.stack([t, np.ones(n)]), np.stack([wn, wn * t])
    _check("GP: gradient, mean", g[:2], want[:2], tol["v"], scale=np.max(np.abs(ref.v)) * np.sum(np.abs(mg), axis=1))
    _check("GP: gradient, white noise", g[2:4], want[2:4], tol["diagB"], scale=np.max(np.abs(ref.diagB)) * np.sum(np.abs(wg), axis=1))
    _check("GP: gradient, kernel", g[4:], want[4:], tol["kgrad"], scale=ref.S)
    val, grad = gp.loo_nll_and_grad(gp.get_parameter_vector(), y)
    _check("GP: loo_nll_and_grad value", val, -ref.L, tol["L"])
    assert np.array_equal(grad, -g)


# ------------------------------------------------------------------ h. where the generic branch cannot go
def test_h_twenty_thousand_points():
    """N = 20 011, m = 128: ``apply_inverse(np.eye(N))`` would be 3.2 GB going in and 3.2 GB coming out"""
    (kernel, x, yerr, r, u), ref, tol = _bounds("m32_3d", 20011, 128, "maxmin", 1e-10, "fitc", want_grad=False)
    s = _solver(kernel, x, yerr, u, "fitc")
    vals = s.loo_lowrank(r)
    _check_loo("N=20011", vals, ref, tol)
    assert vals[4] is None and vals[1].shape == (20011,)
