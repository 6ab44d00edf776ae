"""``InducingSolver``'s gradient reduction and strip driver (george_amd/csrc/gh_inducing.hip) against the NumPy restatement
(tests/inducing_ref.py) at the parameter counts, dimensions, sizes and edges tests/test_gpu_inducing.py does not reach.

``ind_grad_tile_kernel`` sizes its dynamic LDS from the parameter count P and the dimension: ``(2 P + 16) | 1`` doubles a lane
for 64 lanes and two tiles of 64 points.  Above 64 KB the host raises the kernel's limit first.

=====  ======================  ====  =========  ==========================================================================
group  kernel                  ndim  LDS bytes  shapes
=====  ======================  ====  =========  ==========================================================================
a      P = 1                   1     10 752     N = 300, m = 65 max-min points (data points: distance 0 off the diagonal),
a      P = 4                   3     15 872     strips of 128 + 128 + 44 and one automatic strip, 7 test points
a, b   P = 5                   2     15 872
a      P = 16                  4     29 184
a, b   P = 17                  4     30 208
a      P = 20, stack depth 8   16    45 568
a      P = 37                  16    62 976     the largest below the switch
a, b   P = 64 (all 64 lanes)   16    90 624     above the switch: the raised limit
c      m32_3d, P = 2           3     13 824     N = 4200, m = 65: one strip (66 tile rows, two workgroups of the FITC diagonal
                                                kernel), 4096 + 104, and strips of 256
d      m32_3d                  3     13 824     N = 64 / 65 / 128 / 129 / 256 / 257 / 512 x m = 63 / 64 / 65 inducing inputs that
                                                are no data points, strips of 256; M = 128 / 129 / 256 / 257 test points
e      m32_3d                  3     13 824     N = 300, m = 65, strips of 128: 129 and 300 right-hand sides (rp = 256 / 384)
f      DotProduct, P = 0       2     no launch  N = 300, m = 2
g      P = 4 <-> P = 64        3/16  as above   m = 300 in 3-D and m = 65 in 16-D on one native handle, both orders
=====  ======================  ====  =========  ==========================================================================

Tolerances: the rule of tests/test_gpu_inducing.py (``inducing_cases.bounds``), nothing else; tests/test_inducing_host.py shows
that the gradient's bound rejects each wrong gradient of ``inducing_ref.DEFECTS`` on these problems (the weakest, one missing
pair of 273 000, is 8e-7 of ``S`` against a bound of 9e-13).  (b) and (g) compare bits.  The largest error / bound seen on one
MI355X, per group (the module prints its own at the end with ``-s``):

=====  ===============  ===============================================================================================
group  error / bound    the quantity
=====  ===============  ===============================================================================================
a      0.052            ``dot_solve`` 8.3e-14 of 1.6e-12; the gradient at most 7.5e-15 of ``S`` against 8.9e-13 (0.0085)
b      bits             --
c      0.00098
d      0.024            the predictive mean, 7.3e-14 of 3.0e-12
e      0.0013
f      0.0058
g      bits             --
=====  ===============  ===============================================================================================

No case came near its bound, and none showed a defect of the device code.  Running time on one MI355X, the CPU restatement
included: 75 tests in 4.5 s, none above 0.3 s.
"""
import gc

import numpy as np
import pytest

from george_amd import InducingSolver
from george_amd.solvers.inducing import METHODS

import inducing_cases as IC
from inducing_cases import LOG, _check, _check_grad, _check_predict
from oracle import kernels_np
from test_gpu_grad_reference import _masks

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


def _solver(kernel, x, yerr, u, method, rel_jitter, strip):
    s = InducingSolver(kernel, inducing=u, method=method, jitter=rel_jitter, strip_points=strip)
    s.compute(x, yerr)
    return s


def _check_solves(s, r, ref, tol, inverse=True):
    n = len(r)
    _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
    _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
    Y = np.column_stack([r] + list(np.random.RandomState(5).randn(4, n)))
    for B in (r, Y):
        out = s.apply_inverse(B)
        _check("apply_inverse nrhs=%d" % (1 if B.ndim == 1 else B.shape[1]), out, ref.solve(B), tol["alpha"])
        Bc = B.copy()
        assert s.apply_inverse(Bc, in_place=True) is Bc and np.array_equal(Bc, out)
    if inverse:
        _check("get_inverse", s.get_inverse(), ref.solve(np.eye(n)), tol["Cinv"])


# ------------------------------------------------------------------ a. parameter count x dimension
def test_a_the_table_above_is_the_kernels():
    rows = {1: (1, 10752), 4: (3, 15872), 5: (2, 15872), 16: (4, 29184), 17: (4, 30208), "deep8": (16, 45568), 37: (16, 62976),
            64: (16, 90624)}
    assert set(rows) == set(IC.PCASE_NAMES)
    for name, (ndim, lds) in rows.items():
        kernel, x = IC.pcase(name)[:2]
        P = kernels_np.full_size(kernel)
        assert P == (20 if name == "deep8" else name) and x.shape == (300, ndim) and IC.grad_lds_bytes(P, ndim) == lds
    assert IC.grad_lds_bytes(37, 16) <= 64 * 1024 < IC.grad_lds_bytes(64, 16) <= 128 * 1024


@METHOD
@pytest.mark.parametrize("case", IC.PCASE_NAMES)
def test_a_parameter_count_and_dimension(case, method):
    kernel, x, yerr, r, xs, u = IC.pcase(case)
    rel_jitter, _, ref, tol = IC.pcase_bounds(case, method)
    for strip in (128, 0):
        print("strip_points", strip)
        s = _solver(kernel, x, yerr, u, method, rel_jitter, strip)
        _check("log_determinant", s.log_determinant, ref.logdet, tol["logdet"])
        _check("dot_solve", s.dot_solve(r), ref.quad, tol["quad"])
        _check_grad(s, kernel, r, ref, tol)
        _check_predict(s, kernel, r, xs, ref, tol, (7,))


# ------------------------------------------------------------------ b. masks
@METHOD
@pytest.mark.parametrize("P", [5, 17, 64])
def test_b_masks_zero_frozen_entries_and_leave_the_rest_bitwise(P, method):
    kernel, x, yerr, r, xs, u = IC.pcase(P)
    s = _solver(kernel, x, yerr, u, method, 1e-10, 128)
    g_all, a_all, d_all = s.grad(r, np.ones(P, dtype=np.uint32))
    assert np.any(g_all != 0.0)
    for name, m in _masks(P).items():
        g, a, d = s.grad(r, m.astype(np.uint32))
        assert np.all(g[~m] == 0.0), name
        assert np.array_equal(g[m], g_all[m]), name
        assert np.array_equal(a, a_all) and np.array_equal(d, d_all), name


# ------------------------------------------------------------------ c. more than 4096 points in a strip
@METHOD
def test_c_more_than_4096_points_in_a_strip(method):
    """N = 4200: one automatic strip (two workgroups of the diagonal kernel, 66 tile rows), 4096 + 104, and strips of 256"""
    kernel, x, yerr, r, xs, u = IC.m32_case(4200, 65)
    rel_jitter, _, ref, tol = IC.m32_bounds(4200, 65, method)
    runs = []
    for strip in (0, 4096, 256):
        print("strip_points", strip)
        runs.append(_check_grad(_solver(kernel, x, yerr, u, method, rel_jitter, strip), kernel, r, ref, tol))
    for g, alpha, diagA in runs[1:]:
        _check("against one strip: kernel", g, runs[0][0], tol["kgrad"], scale=ref.S)
        _check("  .. alpha", alpha, runs[0][1], tol["alpha"])
        _check("  .. diagA", diagA, runs[0][2], tol["diagA"])


# ------------------------------------------------------------------ d. tile and strip edges
@METHOD
@pytest.mark.parametrize("m", [63, 64, 65])
@pytest.mark.parametrize("n", [64, 65, 128, 129, 256, 257, 512])
def test_d_tile_and_strip_edges(n, m, method):
    """strips of 256: a last strip of one point (257), N a multiple of the strip (512), N the strip (256: the second pass
    re-uses the first one's F and R); the gradient tile's edge in m; test points in strips of 256 likewise"""
    kernel, x, yerr, r, xs, u = IC.m32_case(n, m, "random")
    rel_jitter, _, ref, tol = IC.m32_bounds(n, m, method, "random")
    s = _solver(kernel, x, yerr, u, method, rel_jitter, 256)
    _check_solves(s, r, ref, tol)
    _check_grad(s, kernel, r, ref, tol)
    _check_predict(s, kernel, r, xs, ref, tol, (128, 129, 256, 257))


# ------------------------------------------------------------------ e. wide solves
@METHOD
def test_e_more_than_128_right_hand_sides(method):
    """129 and 300 columns (rp = 256 and 384) and the inverse, N = 300 in strips of 128.  Column 0 of the 129-column solve has
    the bits of the one-column solve: every GEMM of the solve has a column-major operand, so gh_launch_gemm takes the one
    128 x 128-tile kernel whatever the column count, a tile of C belongs to one workgroup that walks K in order, and column
    0 sits in the same place of the same tile."""
    n = 300
    kernel, x, yerr, r, xs, u = IC.m32_case(n, 65)
    rel_jitter, _, ref, tol = IC.m32_bounds(n, 65, method)
    s = _solver(kernel, x, yerr, u, method, rel_jitter, 128)
    B = np.column_stack([r] + list(np.random.RandomState(6).randn(299, n)))
    wide = {}
    for nrhs in (129, 300):
        wide[nrhs] = s.apply_inverse(np.ascontiguousarray(B[:, :nrhs]))
        _check("apply_inverse nrhs=%d" % nrhs, wide[nrhs], ref.solve(B[:, :nrhs]), tol["Cinv"])
    _check("get_inverse", s.get_inverse(), ref.solve(np.eye(n)), tol["Cinv"])
    one = s.apply_inverse(r)
    assert np.array_equal(wide[129][:, 0], one) and np.array_equal(wide[300][:, 0], one)


# ------------------------------------------------------------------ f. no parameters
@METHOD
def test_f_a_kernel_without_parameters(method):
    """DotProductKernel, m = 2: no gradient launch at all; ``grad`` still gives alpha and diag(A)"""
    kernel, x, yerr, r, xs, u = IC.dot_problem()
    _, ref, tol = IC.bounds("dot", kernel, x, yerr, r, xs, u, 1e-10, method)
    for strip in (128, 0):
        s = _solver(kernel, x, yerr, u, method, 1e-10, strip)
        _check_solves(s, r, ref, tol)
        g, alpha, diagA = s.grad(r, kernel.unfrozen_mask.astype(np.uint32))
        assert g.shape == (0,) and ref.kgrad.shape == (0,)
        _check("grad: alpha", alpha, ref.alpha, tol["alpha"])
        _check("grad: diagA", diagA, ref.diagA, tol["diagA"])
        _check_predict(s, kernel, r, xs, ref, tol, (7,))


# ------------------------------------------------------------------ g. a handle that held another problem
def _everything(s, kernel, r, xs):
    B = np.column_stack([r] + list(np.random.RandomState(5).randn(4, len(r))))
    mu, var, _ = s.predict(kernel, r, xs, return_var=True)
    return [np.float64(s.log_determinant), np.float64(s.dot_solve(r)), s.apply_inverse(B)] + \
        list(s.grad(r, np.ones(len(kernel.unfrozen_mask), dtype=np.uint32))) + [mu, var, s.predict(kernel, r, xs, return_cov=True)[2]]


@METHOD
@pytest.mark.parametrize("first,second", [((4, 300), (64, 65)), ((64, 65), (4, 300))], ids=["m300_3d-then-m65_16d", "m65_16d-then-m300_3d"])
def test_g_a_handle_that_held_another_problem(first, second, method):
    """A parked handle keeps its buffers: after m = 300 in 3-D it serves m = 65 in 16-D (every buffer larger than needed, a new
    pitch), and the other way round.  The results have the bits of a fresh handle's."""
    options = dict(method=method, jitter=1e-10, strip_points=128)
    key = (0, METHODS[method], 128)
    InducingSolver.release_pool()
    kernel, x, yerr, r, xs, u = IC.pcase(first[0], 300, first[1])
    a = InducingSolver(kernel, inducing=u, **options)
    a.compute(x, yerr)
    address = a._handle.value
    del a
    gc.collect()
    assert [h.value for h in InducingSolver._HPOOL[key]] == [address]
    kernel, x, yerr, r, xs, u = IC.pcase(second[0], 300, second[1])
    b = InducingSolver(kernel, inducing=u, **options)
    b.compute(x, yerr)
    assert b._handle.value == address and not InducingSolver._HPOOL[key]
    got = _everything(b, kernel, r, xs)
    del b
    gc.collect()
    InducingSolver.release_pool()
    assert not InducingSolver._HPOOL
    c = InducingSolver(kernel, inducing=u, **options)
    c.compute(x, yerr)
    want = _everything(c, kernel, r, xs)
    assert len(got) == len(want) == 9
    for i, (p, q) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(q)) and np.array_equal(p, q), i
