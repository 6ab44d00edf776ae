"""GP.append / GP.truncate on the device (``-m gpu``): a factor extended in place against a fresh factorisation of the
concatenated data and against the CPU oracle, the untouched leading block, the three paths of the new rows, truncation,
failure, pickling, and the full-size problem against the real reference's scalars.

Bounds: "same mathematics, other summation order" -- log-determinant 1e-10 and log-likelihood 1e-9 relative, as
tests/test_gpu_distributed.py and tests/test_gpu_solver.py; everything else as test_gpu_solver.py:62-74."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

import zoo
from oracle import solver_np
import george_amd
from george_amd import kernels, GP, BasicSolver
from george_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hyper_kernel():
    """docs/tutorials/hyper.rst:91-95: 17 nodes, the postfix walker"""
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


KINDS = ["expsq", "hyper", "matern3d"]


def _problem(kind, n, seed=0):
    """(make_gp, x, yerr, y, mean, white_noise) at n points; hyper and matern3d have a fitted mean and fitted white noise"""
    rng = np.random.RandomState(seed + n)
    if kind == "expsq":
        x, yerr, y = zoo.bench_data(n)
        amp = float(np.var(y))
        return (lambda: GP(amp * kernels.ExpSquaredKernel(1.0))), x, yerr, y, 0.0, np.log(george_amd.gp.TINY)
    if kind == "hyper":
        x = np.sort(rng.uniform(0, 40, n))
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
        mean, wn = 0.1, np.log(0.05)
        make = lambda: GP(_hyper_kernel(), mean=mean, fit_mean=True, white_noise=wn, fit_white_noise=True)    # noqa: E731
    else:
        x = rng.uniform(0, 4, (n, 3))
        x = x[np.argsort(x[:, 0])]
        y = np.sin(x[:, 0]) * np.cos(x[:, 1]) + 0.2 * rng.randn(n)
        mean, wn = -0.3, np.log(0.03)
        make = lambda: GP(1.5 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3),    # noqa: E731
                          mean=mean, fit_mean=True, white_noise=wn, fit_white_noise=True)
    yerr = (0.1 + 0.05 * rng.rand(n)) * max(1.0, np.sqrt(n / 300.0))
    return make, x, yerr, y, mean, wn


def _as2d(x):
    return x[:, None] if x.ndim == 1 else x


def _close(a, b, rel, what):
    err = abs(a - b) / abs(b)
    print("%s: %.17g vs %.17g, relative difference %.3g (bound %.0e)" % (what, a, b, err, rel))
    assert err <= rel, (what, a, b, err)


def _same_answers(gp, fresh, x, y, oracle=None, grad=True):
    """the assertions of test 1: gp (appended to / truncated) against a GP computed afresh on the same data"""
    _close(gp.solver.log_determinant, fresh.solver.log_determinant, 1e-10, "log-det vs fresh")
    _close(gp.log_likelihood(y), fresh.log_likelihood(y), 1e-9, "log-like vs fresh")
    if oracle is not None:
        _close(gp.solver.log_determinant, oracle[0], 1e-9, "log-det vs oracle")
        _close(gp.log_likelihood(y), oracle[1], 1e-9, "log-like vs oracle")
    assert gp.solver._n == len(y) == len(gp._x) == int(N.lib.gh_chol_size(gp.solver._handle))
    np.testing.assert_allclose(gp.apply_inverse(y), fresh.apply_inverse(y), rtol=1e-6, atol=1e-8)
    lo, hi = _as2d(x).min(axis=0), _as2d(x).max(axis=0)
    t = lo + (hi - lo) * np.random.RandomState(11).rand(50, _as2d(x).shape[1])
    t = t[:, 0] if x.ndim == 1 else t
    mu, var = gp.predict(y, t, return_var=True)
    mu0, var0 = fresh.predict(y, t, return_var=True)
    np.testing.assert_allclose(mu, mu0, rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(var, var0, rtol=1e-6, atol=1e-9)
    mu16, cov = gp.predict(y, t[:16])
    mu16_0, cov0 = fresh.predict(y, t[:16])
    np.testing.assert_allclose(cov, cov0, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(mu16, mu16_0, rtol=1e-7, atol=1e-8)
    if grad:
        np.testing.assert_allclose(gp.grad_log_likelihood(y), fresh.grad_log_likelihood(y), rtol=1e-6, atol=1e-6)


def _export(solver):
    h = solver._handle
    L = np.empty(int(N.lib.gh_chol_factor_size(h)))
    dinv = np.empty(int(N.lib.gh_chol_dinv_size(h)))
    N.check(N.lib.gh_chol_export_factor(h, N.ptr(L), N.ptr(dinv)))
    return L, dinv


# ------------------------------------------------------------------ 1. parity with a fresh factorisation and the oracle
NM = [(100, 1), (100, 27), (100, 28), (100, 29), (127, 1), (127, 2), (128, 1), (300, 700), (1000, 24), (1000, 25),
      (2048, 4), (2048, 129), (5000, 3), (8192, 1024)]


@pytest.mark.parametrize("n,m", NM)
@pytest.mark.parametrize("kind", KINDS)
def test_append_matches_a_fresh_factorisation_and_the_oracle(kind, n, m):
    make, x, yerr, y, mean, wn = _problem(kind, n + m)
    gp = make()
    gp.compute(x[:n], yerr[:n])
    gp.append(x[n:], yerr[n:])
    fresh = make()
    fresh.compute(x, yerr)
    d = solver_np.DenseOracle(fresh.kernel)
    ll = solver_np.gp_log_likelihood(d, _as2d(x), yerr, y, mean=mean, white_noise=wn)
    _same_answers(gp, fresh, x, y, oracle=(d.log_determinant, ll))


def _one_by_one(kind):
    make, x, yerr, y, mean, wn = _problem(kind, 350)
    gp = make()
    gp.compute(x[:50], yerr[:50])
    for i in range(50, 350):
        gp.append(x[i:i + 1], yerr[i])                     # (one point: a row of x, a scalar error bar)
    fresh = make()
    fresh.compute(x, yerr)
    d = solver_np.DenseOracle(fresh.kernel)
    ll = solver_np.gp_log_likelihood(d, _as2d(x), yerr, y, mean=mean, white_noise=wn)
    return gp, fresh, x, y, (d.log_determinant, ll)


def test_three_hundred_appends_of_one_point():
    """From n = 50 to 350 one point at a time (two tile crossings): the same answers as one factorisation.  On the 3-D Matern
    problem: cond(K) is about 1.6 * 350 / 0.04 = 1e4, so two correct factorisations differ in alpha = K^-1 y by about
    cond * 1e-16 * |alpha| = 1e-11 -- inside the element-wise bound (rtol 1e-6, atol 1e-8) this file takes from
    test_gpu_solver.py.  (Not so for the hyper.rst kernel at this size: the test below.)"""
    gp, fresh, x, y, oracle = _one_by_one("matern3d")
    _same_answers(gp, fresh, x, y, oracle=oracle)


def test_three_hundred_appends_of_one_point_on_the_composite_kernel():
    """The same on the 17-node kernel.  Its amplitude of 66^2 over a noise floor of 0.06 makes cond(K) about 2.5e7 and
    |alpha| about 50: two correct factorisations differ by about cond * 1e-16 * |alpha| = 1e-7 in elements of alpha, so the
    element-wise bound of the test above (atol 1e-8) cannot tell a wrong factor from rounding there (measured: one element of
    350 off by 2.7e-8).  The scalars keep their bounds; alpha is compared on the scale of the vector, as
    test_gpu_fullsize.py:45-46 does for the same reason."""
    gp, fresh, x, y, oracle = _one_by_one("hyper")
    _close(gp.solver.log_determinant, fresh.solver.log_determinant, 1e-10, "log-det vs fresh")
    _close(gp.log_likelihood(y), fresh.log_likelihood(y), 1e-9, "log-like vs fresh")
    _close(gp.solver.log_determinant, oracle[0], 1e-9, "log-det vs oracle")
    _close(gp.log_likelihood(y), oracle[1], 1e-9, "log-like vs oracle")
    alpha, ref = gp.apply_inverse(y), fresh.apply_inverse(y)
    print("alpha: largest difference %.3g on a scale of %.3g" % (np.abs(alpha - ref).max(), np.abs(ref).max()))
    assert np.abs(alpha - ref).max() <= 1e-6 * np.abs(ref).max()
    # what supports "rounding": the CPU oracle's alpha (LAPACK on the same matrix) is no nearer to the fresh device factor's
    # than the appended factor's is -- the three agree with one another at the same level
    d = solver_np.DenseOracle(fresh.kernel)
    d.compute(_as2d(x), np.sqrt(fresh._yerr2 + np.exp(fresh._call_white_noise(fresh._x))))
    cpu = d.apply_inverse(fresh._residual(y))
    far_fresh, far_app = np.abs(ref - cpu).max(), np.abs(alpha - cpu).max()
    print("alpha against the CPU oracle: fresh %.3g, appended %.3g" % (far_fresh, far_app))
    assert far_app <= 1e-6 * np.abs(cpu).max() and far_fresh <= 1e-6 * np.abs(cpu).max()

# ------------------------------------------------------------------ 2. the leading block is untouched
@pytest.mark.parametrize("n,m", [(300, 5), (300, 700), (1000, 25), (1024, 3)])
def test_rows_of_the_full_tiles_keep_their_bits(n, m):
    make, x, yerr, y, _, _ = _problem("matern3d", n + m)
    gp = make()
    gp.compute(x[:n], yerr[:n])
    L0, d0 = _export(gp.solver)
    gp.append(x[n:], yerr[n:])
    L1, d1 = _export(gp.solver)
    n0 = 128 * (n // 128)
    assert len(L1) == (n + m) * (n + m + 1) // 2
    assert np.array_equal(L0[:n0 * (n0 + 1) // 2], L1[:n0 * (n0 + 1) // 2])
    assert np.array_equal(d0[:(n0 // 128) * 128 * 128], d1[:(n0 // 128) * 128 * 128])


# ------------------------------------------------------------------ 3. the paths of the new rows
@pytest.mark.parametrize("m", [2, 4, 7])
def test_one_row_sweeps_and_multi_row_sweeps_give_the_same_bits(m):
    """m = 2 and m = 4 are the instantiated widths; 7 = 4 + 2 + 1 takes both and the one-row kernel"""
    make, x, yerr, y, _, _ = _problem("hyper", 1000 + m)
    out = {}
    try:
        for path in (1, 2, 3):
            N.lib.gh_debug_set_append_path(path)
            gp = make()
            gp.compute(x[:1000], yerr[:1000])
            gp.append(x[1000:], yerr[1000:])
            out[path] = (_export(gp.solver), gp)
    finally:
        N.lib.gh_debug_set_append_path(0)
    (L1, d1), (L2, d2) = out[1][0], out[2][0]
    assert np.array_equal(L1, L2) and np.array_equal(d1, d2)
    _same_answers(out[3][1], out[1][1], x, y)
    assert np.abs(out[3][0][0] - L1).max() <= 1e-9 * np.abs(L1).max()


def test_the_blocked_substitution_on_few_and_many_rows():
    make, x, yerr, y, _, _ = _problem("expsq", 2048 + 300)
    fresh = make()
    fresh.compute(x, yerr)
    try:
        for path in (2, 3):
            N.lib.gh_debug_set_append_path(path)
            gp = make()
            gp.compute(x[:2048], yerr[:2048])
            gp.append(x[2048:2048 + 40], yerr[2048:2048 + 40])
            gp.append(x[2048 + 40:], yerr[2048 + 40:])
            _same_answers(gp, fresh, x, y)
    finally:
        N.lib.gh_debug_set_append_path(0)


# ------------------------------------------------------------------ 4. truncate
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [950, 896, 300])
def test_truncate_matches_compute_on_the_leading_points(kind, k):
    """k inside the last tile, on a tile boundary, several tiles down"""
    make, x, yerr, y, _, _ = _problem(kind, 1000)
    gp = make()
    gp.compute(x, yerr)
    gp.truncate(k)
    fresh = make()
    fresh.compute(x[:k], yerr[:k])
    _same_answers(gp, fresh, x[:k], y[:k])
    np.testing.assert_allclose(gp.solver.get_inverse(), fresh.solver.get_inverse(), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("n,m", [(1000, 37), (100, 5), (1024, 128)])
def test_append_then_truncate_gives_the_likelihood_back(n, m):
    make, x, yerr, y, _, _ = _problem("expsq", n + m)
    gp = make()
    gp.compute(x[:n], yerr[:n])
    before = gp.log_likelihood(y[:n])
    gp.append(x[n:], yerr[n:])
    gp.truncate(n)
    _close(gp.log_likelihood(y[:n]), before, 1e-12, "log-like after append + truncate")
    assert len(gp._x) == n


def test_truncate_argument_checks():
    make, x, yerr, y, _, _ = _problem("expsq", 300)
    gp = make()
    gp.compute(x, yerr)
    before = gp.log_likelihood(y)
    L0, d0 = _export(gp.solver)
    gp.truncate(300)                                       # a no-op
    L1, d1 = _export(gp.solver)
    assert np.array_equal(L0, L1) and np.array_equal(d0, d1) and gp.log_likelihood(y) == before
    for bad in (0, 301):
        with pytest.raises(ValueError):
            gp.truncate(bad)
        with pytest.raises(ValueError):
            gp.solver.truncate(bad)
    out = ctypes.c_double(0.0)
    for bad in (0, 301):
        with pytest.raises(ValueError):
            N.check(N.lib.gh_chol_truncate(gp.solver._handle, bad, ctypes.byref(out)))
    assert gp.log_likelihood(y) == before


def test_native_calls_refuse_a_handle_that_is_not_computed():
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    h = s._ensure_handle()
    N.lib.gh_chol_release_buffers(h)                       # (a pooled handle may hold somebody's factor)
    from george_amd.program import DeviceKernel
    dk = DeviceKernel(s.kernel)
    out, buf = ctypes.c_double(0.0), np.zeros(4)
    with pytest.raises(RuntimeError, match="compute"):
        N.check(N.lib.gh_chol_append(h, dk.handle, N.ptr(buf), 1, N.ptr(buf), ctypes.byref(out)))
    with pytest.raises(RuntimeError, match="compute"):
        N.check(N.lib.gh_chol_truncate(h, 1, ctypes.byref(out)))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_append(h, dk.handle, N.ptr(buf), 0, N.ptr(buf), ctypes.byref(out)))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_append(h, dk.handle, None, 1, N.ptr(buf), ctypes.byref(out)))


# ------------------------------------------------------------------ 5. failure leaves the GP usable
@pytest.mark.parametrize("n", [300, 256])
def test_a_failing_append_leaves_the_factor_bit_for_bit(n):
    """Five copies of x = 1e6 without noise behind points in [0, 1]: the cross-covariances underflow to exactly 0, the new
    block is exactly the all-ones matrix, and the second new pivot is exactly 1 - 1 * 1 = 0.  n = 256: the new rows open a
    tile of their own (the factor moves into larger buffers); n = 300: they fill the last tile in place."""
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0, 1, n))
    y = np.sin(6 * x)
    xn = np.full(5, 1e6)
    d = solver_np.DenseOracle(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(np.linalg.LinAlgError):             # the CPU agrees that this is singular
        d.compute(np.concatenate([x, xn])[:, None], np.sqrt(np.concatenate([np.full(n, 0.01), np.zeros(5)]) + np.exp(-80.0)))
    gp = GP(kernels.ExpSquaredKernel(1.0), white_noise=-80.0)
    gp.compute(x, 0.1)
    before = gp.log_likelihood(y)
    L0, d0 = _export(gp.solver)
    with pytest.raises(np.linalg.LinAlgError, match=r"^%d-th leading minor" % (n + 2)):
        gp.append(xn, 0.0)
    assert int(N.lib.gh_chol_info(gp.solver._handle)) == n + 2
    assert len(gp._x) == n and len(gp._yerr2) == n and gp.computed and gp.solver._n == n
    assert int(N.lib.gh_chol_size(gp.solver._handle)) == n
    assert gp.log_likelihood(y) == before                  # bit for bit
    L1, d1 = _export(gp.solver)
    assert np.array_equal(L0, L1) and np.array_equal(d0, d1)
    # and it still takes points that do extend it
    gp.append(np.array([1.5, 2.0]), 0.1)
    fresh = GP(kernels.ExpSquaredKernel(1.0), white_noise=-80.0)
    fresh.compute(np.concatenate([x, [1.5, 2.0]]), 0.1)
    y2 = np.concatenate([y, [0.3, -0.2]])
    _close(gp.log_likelihood(y2), fresh.log_likelihood(y2), 1e-9, "log-like after the failed and a good append")


# ------------------------------------------------------------------ 6. pickle
def test_an_appended_gp_pickles_with_its_factor():
    make, x, yerr, y, _, _ = _problem("matern3d", 350)
    gp = make()
    gp.compute(x[:300], yerr[:300])
    gp.append(x[300:], yerr[300:])
    t = x[::7] + 0.01
    mu, var = gp.predict(y, t, return_var=True)
    gp2 = pickle.loads(pickle.dumps(gp, -1))
    assert gp2.computed and gp2.solver._n == 350 and gp2.solver._x_host.shape == (350, 3)
    mu2, var2 = gp2.predict(y, t, return_var=True)
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
    assert gp2.log_likelihood(y) == gp.log_likelihood(y)
    # the restored factor can be extended again (the error bars travel in the solver's state: gh_chol_set_yerr)
    gp2.append(x[:3] + 0.5, 0.2)
    fresh = make()
    fresh.compute(np.concatenate([x, x[:3] + 0.5]), np.concatenate([yerr, np.full(3, 0.2)]))
    y3 = np.concatenate([y, y[:3]])
    _close(gp2.solver.log_determinant, fresh.solver.log_determinant, 1e-10, "log-det, restored + appended vs fresh")
    _close(gp2.log_likelihood(y3), fresh.log_likelihood(y3), 1e-9, "log-like, restored + appended vs fresh")


def test_a_solver_restored_without_error_bars_takes_the_fallback():
    """a state pickled before the solver kept its error bars: GP.append computes the concatenated inputs afresh"""
    make, x, yerr, y, _, _ = _problem("expsq", 300)
    gp = make()
    gp.compute(x[:280], yerr[:280])
    gp.solver = pickle.loads(pickle.dumps(gp.solver))
    gp.solver.__dict__.pop("_yerr_host")
    assert not gp.solver.appendable and gp.computed
    with pytest.raises(RuntimeError, match="error bars"):
        gp.solver.append(_as2d(x[280:]), yerr[280:])
    old = gp.solver
    gp.append(x[280:], yerr[280:])
    assert gp.solver is not old and gp.solver.appendable
    fresh = make()
    fresh.compute(x, yerr)
    assert gp.log_likelihood(y) == fresh.log_likelihood(y)
    gp.truncate(290)                                       # and a restored solver can still be cut
    assert len(gp._x) == 290


# ------------------------------------------------------------------ 7. full size against the real reference's numbers
@pytest.mark.parametrize("m", [1000, 3])
def test_full_size_append_against_reference_scalars(m):
    with open(os.path.join(ROOT, "tests", "golden", "large.json")) as f:
        g = json.load(f)["NS"]
    n = 65536
    assert g["n"] == n
    x, yerr, y = zoo.bench_data(n)
    gp = GP(np.var(y) * kernels.ExpSquaredKernel(1.0))
    gp.compute(x[:n - m], yerr[:n - m])
    gp.append(x[n - m:], yerr[n - m:])
    _close(gp.solver.log_determinant, g["logdet"], 1e-10, "log-det vs reference")
    _close(gp.log_likelihood(y), g["loglike"], 1e-9, "log-like vs reference")
