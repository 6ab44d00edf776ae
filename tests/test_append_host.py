"""GP.append / GP.truncate on the host side (no GPU): the ABI table, the argument checks that run before any device call, and
the fallback of ``GP.append`` for a solver without ``append`` -- a NumPy stand-in (``oracle.solver_np.DenseOracle``)."""
import ctypes
import os
import re

import numpy as np
import pytest

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


def test_signature_table_and_headers_agree():
    text = open(os.path.join(ROOT, "include", "george_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+gh_chol_append\(gh_chol\* s, gh_kernel\* k, const double\* x_new, int64_t m, "
                     r"const double\* yerr_new, double\* logdet_out\);", text)
    assert re.search(r"int\s+gh_chol_truncate\(gh_chol\* s, int64_t n_keep, double\* logdet_out\);", text)
    dbg = open(os.path.join(ROOT, "include", "george_amd_debug.h")).read()
    assert "int gh_debug_set_append_path(int path);" in dbg
    _vp, _i64, _pd = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_double)
    assert N.SIGNATURES["gh_chol_append"] == (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp, _pd])
    assert N.SIGNATURES["gh_chol_truncate"] == (ctypes.c_int, [_vp, _i64, _pd])
    assert N.SIGNATURES["gh_debug_set_append_path"] == (ctypes.c_int, [ctypes.c_int])
    for name in ("gh_chol_append", "gh_chol_truncate", "gh_debug_set_append_path"):
        assert hasattr(N.lib, name)
    # struct sizes do not change
    assert ctypes.sizeof(N.gh_chol_opts) == 8 * 4 and ctypes.sizeof(N.gh_chol_profile) == 11 * 8


def test_native_calls_reject_bad_arguments_without_a_gpu():
    out = ctypes.c_double(0.0)
    buf = np.zeros(4)
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_append(None, None, N.ptr(buf), 1, N.ptr(buf), ctypes.byref(out)))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_chol_truncate(None, 1, ctypes.byref(out)))
    # the path switch is host state: it keeps what it was given and maps anything unknown to the automatic rule
    prev = N.lib.gh_debug_set_append_path(2)
    try:
        assert N.lib.gh_debug_set_append_path(7) == 2
        assert N.lib.gh_debug_set_append_path(0) == 0
    finally:
        N.lib.gh_debug_set_append_path(prev)
    # a solver that was never computed has nothing to extend
    s = BasicSolver(kernels.ExpSquaredKernel(1.0))
    with pytest.raises(RuntimeError, match="compute"):
        s.append(np.zeros((1, 1)), 0.1)
    with pytest.raises(RuntimeError, match="compute"):
        s.truncate(1)
    import george_amd
    if george_amd.device_count() == 0:
        # no device: nothing quietly computes on the host instead
        gp = GP(kernels.ExpSquaredKernel(1.0))
        with pytest.raises(RuntimeError):
            gp.append(np.arange(4.0), 0.1)


@pytest.mark.parametrize("case", range(3))
def test_append_takes_the_fallback_for_a_solver_without_append(case):
    make, x = list(_cases())[case]
    rng = np.random.RandomState(case)
    n, m = 29, 11
    y = np.sin(np.atleast_2d(x.T)[0]) + 0.1 * rng.randn(len(x))
    yerr = 0.05 + 0.01 * rng.rand(len(x))
    whole = make()
    whole.compute(x, yerr)
    gp = make()
    assert not hasattr(gp.solver_type, "append")
    gp.compute(x[:n], yerr[:n])
    first = gp.solver
    gp.append(x[n:], yerr[n:])
    assert gp.solver is not first and gp.computed                     # a fresh compute of the concatenated inputs
    assert gp._x.shape == whole._x.shape and np.array_equal(gp._x, whole._x)
    assert np.array_equal(gp._yerr2, whole._yerr2)
    assert gp.solver.log_determinant == whole.solver.log_determinant
    assert gp.log_likelihood(y) == whole.log_likelihood(y)            # white noise and mean at all n + m points
    assert np.array_equal(gp.apply_inverse(y), whole.apply_inverse(y))
    with pytest.raises(ValueError):
        gp.log_likelihood(y[:n])                                      # y has the new length from here on
    # and back
    gp.truncate(n)
    part = make()
    part.compute(x[:n], yerr[:n])
    assert np.array_equal(gp._x, part._x) and np.array_equal(gp._yerr2, part._yerr2)
    assert gp.log_likelihood(y[:n]) == part.log_likelihood(y[:n])
    gp.truncate(n)                                                    # keeping everything: nothing happens
    assert len(gp._x) == n
    for bad in (0, n + 1, -3):
        with pytest.raises(ValueError):
            gp.truncate(bad)


def test_append_scalar_and_vector_error_bars_and_shapes():
    make, x = list(_cases())[0]
    gp = make()
    gp.append(x[:10], 0.1)                                            # never computed: append is compute
    assert gp.computed and len(gp._x) == 10 and np.array_equal(gp._yerr2, np.full(10, 0.1) ** 2)
    gp.append(x[10:13], [0.2, 0.3, 0.4])
    assert np.array_equal(gp._yerr2[10:], np.array([0.2, 0.3, 0.4]) ** 2)
    gp.append(x[13], 0.5)                                             # one point, scalar
    assert len(gp._x) == 14 and gp._yerr2[-1] == 0.25
    with pytest.raises(ValueError):
        gp.append(x[14:16], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        gp.append(np.zeros((2, 3)), 0.1)                              # wrong input dimension
    assert len(gp._x) == 14
    gp.append(np.empty(0), 0.1)                                       # nothing to add
    assert len(gp._x) == 14


def test_a_dirty_model_is_recomputed_on_the_concatenated_inputs():
    make, x = list(_cases())[0]
    gp = make()
    gp.compute(x[:20], 0.1)
    v = gp.get_parameter_vector()
    gp.set_parameter_vector(v + 0.1)
    assert not gp.computed
    gp.append(x[20:], 0.1)
    whole = make()
    whole.set_parameter_vector(v + 0.1)
    whole.compute(x, 0.1)
    y = np.cos(x)
    assert gp.computed and gp.log_likelihood(y) == whole.log_likelihood(y)


def test_a_failing_append_leaves_the_gp_unchanged():
    gp = GP(kernels.ExpSquaredKernel(1.0), white_noise=-80.0, solver=solver_np.DenseOracle)
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 1, 30))
    y = np.sin(x)
    gp.compute(x, 0.1)
    before = gp.log_likelihood(y)
    solver = gp.solver
    with pytest.raises(np.linalg.LinAlgError):
        gp.append(np.full(5, 1e6), 0.0)                               # five identical points without noise: singular
    assert gp.solver is solver and gp.computed and len(gp._x) == 30 and len(gp._yerr2) == 30
    assert gp.log_likelihood(y) == before
