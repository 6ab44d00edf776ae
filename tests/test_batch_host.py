"""GP.log_likelihood_batch on the host side (no GPU): the mapping of (B, len(gp)) parameter vectors to the per-member
inputs of the batched device call, and the argument checks that run before any device call."""
import numpy as np
import pytest

from george_amd import GP, kernels
from george_amd.modeling import Model


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


def _hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _pretend_computed(gp, x, yerr):
    # what compute() records before it factorises (the mapping needs nothing else)
    gp._x = np.ascontiguousarray(gp.parse_samples(x), dtype=np.float64)
    gp._yerr2 = np.ascontiguousarray(np.broadcast_to(yerr, (len(gp._x),)) ** 2, dtype=np.float64)


def _loop_inputs(gp, vectors, y):
    kp, sig, res = [], [], []
    v0 = gp.get_parameter_vector()
    for v in vectors:
        gp.set_parameter_vector(v)
        kp.append(gp.kernel.get_parameter_vector(include_frozen=True))
        sig.append(np.sqrt(gp._yerr2 + np.exp(gp._call_white_noise(gp._x))))
        res.append(y - gp._call_mean(gp._x))
    gp.set_parameter_vector(v0)
    return np.array(kp), np.array(sig), np.array(res)


def _cases():
    rng = np.random.RandomState(3)
    x = np.sort(rng.uniform(0, 10, 40))
    # a frozen kernel parameter, a fitted constant mean and fitted white noise
    k = 1.5 * kernels.Matern32Kernel(2.0)
    k.freeze_parameter("k1:log_constant")
    yield GP(k, mean=0.3, fit_mean=True, white_noise=np.log(0.01), fit_white_noise=True), x
    # a Model subclass mean, the 17-node composite kernel with one of its parameters frozen
    k = _hyper_kernel()
    k.freeze_parameter("k1:k1:k2:k2:log_period")
    yield GP(k, mean=LinearMean(m=0.2, b=-1.0), white_noise=np.log(0.02), fit_white_noise=True), x
    # 3-D axis-aligned Matern52 + Constant, default mean and white noise
    x3 = rng.uniform(0, 3, (40, 3))
    yield GP(2.0 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3)), x3


@pytest.mark.parametrize("case", range(3))
def test_batch_inputs_match_the_one_vector_path(case):
    gp, x = list(_cases())[case]
    rng = np.random.RandomState(case)
    y = np.sin(np.atleast_2d(x.T)[0]) + 0.1 * rng.randn(len(x))
    _pretend_computed(gp, x, 0.05 + 0.01 * rng.rand(len(x)))
    p0 = gp.get_parameter_vector()
    vectors = p0 + 1e-2 * rng.randn(7, len(p0))
    kp, sig, res, ok = gp._batch_inputs(vectors, y, quiet=True)
    kp0, sig0, res0 = _loop_inputs(gp, vectors, y)
    assert kp.shape == (7, gp.kernel.full_size)
    assert np.array_equal(kp, kp0)
    assert np.array_equal(sig, sig0)
    assert np.array_equal(res, res0)
    assert ok.all()
    # the GP's own parameters are untouched by the mapping
    assert np.array_equal(gp.get_parameter_vector(), p0)


def test_batch_inputs_flag_a_failing_mean():
    gp, x = list(_cases())[1]
    _pretend_computed(gp, x, 0.1)
    p0 = gp.get_parameter_vector()
    vectors = np.tile(p0, (3, 1))
    vectors[1, 0] = np.inf                              # mean slope
    _, _, _, ok = gp._batch_inputs(vectors, np.zeros(len(x)), quiet=True)
    assert ok.tolist() == [True, False, True]
    with pytest.raises(ValueError, match="member 1"):
        gp._batch_inputs(vectors, np.zeros(len(x)), quiet=False)


def test_argument_checks_before_any_device_call():
    gp = GP(kernels.ExpSquaredKernel(1.0))
    p = gp.get_parameter_vector()
    with pytest.raises(RuntimeError, match="compute"):
        gp.log_likelihood_batch(p[None, :], np.zeros(5))
    x = np.linspace(0, 1, 5)
    _pretend_computed(gp, x, 0.1)
    with pytest.raises(ValueError):
        gp.log_likelihood_batch(np.zeros((3, len(p) + 1)), np.zeros(5))     # wrong width
    with pytest.raises(ValueError):
        gp.log_likelihood_batch(p, np.zeros(5))                             # 1-D vectors
    with pytest.raises(ValueError):
        gp.log_likelihood_batch(p[None, :], np.zeros(6))                    # wrong y length
    with pytest.raises(ValueError):
        gp.log_likelihood_batch(p[None, :], np.zeros((5, 2)))               # 2-D y
    out = gp.log_likelihood_batch(np.zeros((0, len(p))), np.zeros(5))
    assert isinstance(out, np.ndarray) and out.shape == (0,)


def test_batch_routing_limits_are_documented_defaults():
    from george_amd import BasicSolver
    assert BasicSolver.BATCH_MAX_N == 8192
    assert BasicSolver.BATCH_MAX_BYTES == 8 << 30
    assert callable(getattr(BasicSolver, "objective_batch", None))
