"""GP.remove on the host side (no GPU): the NumPy model of the blocked update (tests/remove_ref.py) against a factorisation of
the kept points, the ABI table, the argument rule that runs before any device call, and the fallback of ``GP.remove`` for a
solver without ``remove`` -- a NumPy stand-in (``oracle.solver_np.DenseOracle``)."""
import ctypes
import os
import re

import numpy as np
import pytest

import remove_ref
from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from george_amd.modeling import Model
from oracle import solver_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


class NoiseRamp(Model):
    """log white-noise variance that depends on the point: evaluated at the wrong points it gives the wrong matrix"""
    parameter_names = ("a", "c")

    def get_value(self, t):
        return self.a + self.c * t


def _hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _cases():
    rng = np.random.RandomState(3)
    x = np.sort(rng.uniform(0, 10, 40))
    yield (lambda: GP(1.5 * kernels.Matern32Kernel(2.0), mean=0.3, fit_mean=True, white_noise=np.log(0.01),
                      fit_white_noise=True, solver=solver_np.DenseOracle)), x
    yield (lambda: GP(_hyper_kernel(), mean=LinearMean(m=0.2, b=-1.0), white_noise=NoiseRamp(a=np.log(0.02), c=0.3),
                      fit_white_noise=True, solver=solver_np.DenseOracle)), x
    x3 = rng.uniform(0, 3, (40, 3))
    yield (lambda: GP(2.0 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3),
                      solver=solver_np.DenseOracle)), x3


# ------------------------------------------------------------------ the NumPy model of the blocked update
REF_CASES = [(100, [0]), (100, list(range(5))), (100, [3, 40, 41, 99]), (129, [128]), (257, [16]), (200, list(range(100, 140))),
             (300, sorted(np.random.RandomState(37).choice(300, 37, replace=False).tolist())), (640, [127, 128, 129, 383, 384])]


@pytest.mark.parametrize("n,removed", REF_CASES, ids=["%d-%d" % (n, len(r)) for n, r in REF_CASES])
@pytest.mark.parametrize("T", [16, 128])
def test_the_blocked_update_gives_the_factor_of_the_kept_points(T, n, removed):
    """unit amplitude, unit diagonal: the factor's entries are at most 1 and 1e-12 absolute is 4e3 rounding errors"""
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0, 10, n))
    K = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2) + 0.01 * np.eye(n)
    L = np.linalg.cholesky(K)
    keep, rem = remove_ref.split(n, removed)
    want = np.linalg.cholesky(K[np.ix_(keep, keep)])
    got = remove_ref.remove_ref(L, removed, T=T)
    err = np.abs(got - want).max()
    print("T = %d, n = %d, %d removed: largest difference %.3g" % (T, n, len(rem), err))
    assert got.shape == want.shape and err <= 1e-12
    j0 = remove_ref.first_tile(rem, T)
    assert np.array_equal(got[:j0], L[:j0, :len(keep)])               # rows in front of the first affected tile: the old bits


def test_split_means_what_numpy_delete_means():
    keep, rem = remove_ref.split(10, [7, 2, 2])
    assert keep.tolist() == np.delete(np.arange(10), [7, 2, 2]).tolist() and rem.tolist() == [2, 7]
    with pytest.raises(IndexError):
        remove_ref.split(10, [10])


# ------------------------------------------------------------------ ABI
def test_signature_table_and_headers_agree():
    text = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+gh_chol_remove\(gh_chol\* s, const int64_t\* idx, int64_t m, double\* logdet_out\);", text)
    assert re.search(r"GH_REFACTORIZE = 8", text)
    dbg = open(os.path.join(ROOT, "include", "george_amd_debug.h")).read()
    assert "int gh_debug_set_remove_path(int path);" in dbg
    assert "int gh_debug_check_remove_args(int64_t n, const int64_t* idx, int64_t m);" in dbg
    _vp, _i64, _pd = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
    assert N.SIGNATURES["gh_chol_remove"] == (ctypes.c_int, [_vp, _vp, _i64, _pd])
    assert N.SIGNATURES["gh_debug_set_remove_path"] == (ctypes.c_int, [ctypes.c_int])
    assert N.SIGNATURES["gh_debug_check_remove_args"] == (ctypes.c_int, [_i64, _vp, _i64])
    assert N.GH_REFACTORIZE == 8
    for name in ("gh_chol_remove", "gh_debug_set_remove_path", "gh_debug_check_remove_args"):
        assert hasattr(N.lib, name)
    # struct sizes do not change
    assert ctypes.sizeof(N.gh_chol_opts) == 8 * 4 and ctypes.sizeof(N.gh_chol_profile) == 11 * 8


def test_native_calls_reject_bad_arguments_without_a_gpu():
    """A computed handle needs a device, so the rule gh_chol_remove applies to (n, idx, m) is exported as host code of its own
    (gh_debug_check_remove_args) and checked here; tests/test_gpu_remove.py checks that the entry point applies it."""
    out = ctypes.c_double(0.0)
    one = np.zeros(1, dtype=np.int64)
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_remove(None, N.ptr(one), 1, ctypes.byref(out)))

    def rule(n, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return N.lib.gh_debug_check_remove_args(n, N.ptr(idx) if len(idx) else N.ptr(one), len(idx))
    assert rule(10, [0]) == N.GH_OK and rule(10, [0, 3, 9]) == N.GH_OK and rule(10, list(range(1, 10))) == N.GH_OK
    for what, n, idx in [("m = 0", 10, []), ("m = n", 4, [0, 1, 2, 3]), ("unsorted", 10, [3, 2]), ("duplicate", 10, [2, 2]),
                         ("negative", 10, [-1, 2]), ("too large", 10, [2, 10])]:
        with pytest.raises(ValueError):
            N.check(rule(n, idx))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_debug_check_remove_args(10, None, 1))
    # the path switch is host state: it keeps what it was given and maps anything unknown to the automatic rule
    prev = N.lib.gh_debug_set_remove_path(2)
    try:
        assert N.lib.gh_debug_set_remove_path(1) == 2
        assert N.lib.gh_debug_set_remove_path(7) == 1
        assert N.lib.gh_debug_set_remove_path(-1) == 0
        assert N.lib.gh_debug_set_remove_path(0) == 0
    finally:
        N.lib.gh_debug_set_remove_path(prev)
    # a solver that was never computed has nothing to take points from
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):
        s.remove([0])
    gp = GP(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="You need to compute the model first"):
        gp.remove([0])


# ------------------------------------------------------------------ GP.remove through the fallback
def _data(x, seed):
    rng = np.random.RandomState(seed)
    y = np.sin(np.atleast_2d(x.T)[0]) + 0.1 * rng.randn(len(x))
    return y, 0.05 + 0.01 * rng.rand(len(x))


@pytest.mark.parametrize("form", ["list", "mask", "slice", "negative"])
@pytest.mark.parametrize("case", range(3))
def test_remove_takes_the_fallback_for_a_solver_without_remove(case, form):
    """case 1 has a point-dependent white-noise model (NoiseRamp): it must be evaluated at the kept points"""
    make, x = list(_cases())[case]
    y, yerr = _data(x, case)
    n = len(x)
    indices = {"list": [3, 17, 18, 39], "mask": np.arange(n) % 7 == 2, "slice": slice(0, 5), "negative": [-1, -40, 5]}[form]
    keep = np.delete(np.arange(n), indices)
    part = make()
    part.compute(x[keep], yerr[keep])
    gp = make()
    assert not hasattr(gp.solver_type, "remove")
    gp.compute(x, yerr)
    first = gp.solver
    gp.remove(indices)
    assert gp.solver is not first and gp.computed                     # a fresh compute of the kept inputs
    assert gp._x.shape == part._x.shape and np.array_equal(gp._x, part._x)
    assert np.array_equal(gp._yerr2, part._yerr2)
    assert gp.solver.log_determinant == part.solver.log_determinant
    assert gp.log_likelihood(y[keep]) == part.log_likelihood(y[keep])
    assert np.array_equal(gp.apply_inverse(y[keep]), part.apply_inverse(y[keep]))
    with pytest.raises(ValueError):
        gp.log_likelihood(y)                                          # y has the new length from here on


def test_remove_nothing_everything_and_bad_indices():
    make, x = list(_cases())[0]
    y, yerr = _data(x, 0)
    gp = make()
    gp.compute(x, yerr)
    solver, before = gp.solver, gp.log_likelihood(y)
    for nothing in ([], np.zeros(len(x), dtype=bool), slice(5, 5), np.empty(0, dtype=np.int64)):
        gp.remove(nothing)
        assert gp.solver is solver and len(gp._x) == len(x) and gp.log_likelihood(y) == before
    for everything in (slice(None), np.ones(len(x), dtype=bool), list(range(len(x)))):
        with pytest.raises(ValueError):
            gp.remove(everything)
    for bad in ([len(x)], [-len(x) - 1], [0, 400], np.ones(len(x) + 1, dtype=bool), [1.5]):
        with pytest.raises(IndexError):
            gp.remove(bad)
    assert gp.solver is solver and len(gp._x) == len(x) and gp.log_likelihood(y) == before
    gp.remove([4, 4, -36])                                             # duplicates and aliases name one point, as for np.delete
    assert len(gp._x) == len(x) - 1


def test_a_dirty_model_is_recomputed_on_the_kept_inputs():
    make, x = list(_cases())[0]
    gp = make()
    gp.compute(x, 0.1)
    v = gp.get_parameter_vector()
    gp.set_parameter_vector(v + 0.1)
    assert not gp.computed
    gp.remove(slice(0, 40, 3))
    keep = np.delete(np.arange(40), slice(0, 40, 3))
    part = make()
    part.set_parameter_vector(v + 0.1)
    part.compute(x[keep], 0.1)
    y = np.cos(x[keep])
    assert gp.computed and gp.log_likelihood(y) == part.log_likelihood(y)


class _Refusing(solver_np.DenseOracle):
    """a solver whose ``remove`` sends the caller to ``compute``, and whose ``compute`` can be made to fail"""
    fail = False

    def compute(self, x, yerr):
        if _Refusing.fail:
            raise np.linalg.LinAlgError("refused")
        return super(_Refusing, self).compute(x, yerr)

    def remove(self, indices):
        raise RuntimeError("compute afresh")


def test_an_exception_leaves_the_gp_unchanged():
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 1, 30))
    y = np.sin(x)
    gp = GP(kernels.ExpSquaredKernel(1.0), solver=_Refusing)
    gp.compute(x, 0.1)
    before, solver, x0, e0 = gp.log_likelihood(y), gp.solver, gp._x, gp._yerr2
    _Refusing.fail = True
    try:
        with pytest.raises(np.linalg.LinAlgError):
            gp.remove([3, 4])
    finally:
        _Refusing.fail = False
    assert gp.solver is solver and gp.computed and gp._x is x0 and gp._yerr2 is e0
    assert gp.log_likelihood(y) == before
    gp.remove([3, 4])                                                  # the solver's RuntimeError: computed afresh on the kept points
    assert gp.solver is not solver and len(gp._x) == 28
    part = GP(kernels.ExpSquaredKernel(1.0), solver=solver_np.DenseOracle)
    part.compute(np.delete(x, [3, 4]), 0.1)
    assert gp.log_likelihood(np.delete(y, [3, 4])) == part.log_likelihood(np.delete(y, [3, 4]))
