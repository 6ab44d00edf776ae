"""GP.nll_and_grad_batch / grad_log_likelihood_batch on the host side (no GPU): the per-member assembly of the mean and
white-noise blocks from the device's alpha and diag(A), the argument checks and prior screening that run before any device
call, the failure handling around it (with the device call replaced by a stand-in), and the routing limits."""
import numpy as np
import pytest

from george_amd import GP, BasicSolver, HODLRSolver, kernels
from george_amd.modeling import ConstantModel, Model


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


def _pretend_computed(gp, x, yerr):
    # what compute() records before it factorises (the host logic needs nothing else)
    gp._x = np.ascontiguousarray(gp.parse_samples(x), dtype=np.float64)
    gp._yerr2 = np.ascontiguousarray(np.broadcast_to(yerr, (len(gp._x),)) ** 2, dtype=np.float64)


def _cases():
    rng = np.random.RandomState(3)
    x = np.sort(rng.uniform(0, 10, 40))
    # a frozen kernel parameter, a fitted constant mean and fitted white noise
    k = 1.5 * kernels.Matern32Kernel(2.0)
    k.freeze_parameter("k1:log_constant")
    yield GP(k, mean=0.3, fit_mean=True, white_noise=np.log(0.01), fit_white_noise=True), x
    # a Model subclass mean, white noise, a frozen metric
    k = 0.7 * kernels.ExpSquaredKernel(1.2) + 0.2 * kernels.Matern52Kernel(0.5)
    k.freeze_parameter("k2:k2:metric:log_M_0_0")
    yield GP(k, mean=LinearMean(m=0.2, b=-1.0), white_noise=np.log(0.02), fit_white_noise=True), x
    # 3-D axis-aligned Matern52 + Constant, fitted white noise, default mean
    yield (GP(2.0 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3),
              white_noise=np.log(0.03), fit_white_noise=True), rng.uniform(0, 3, (40, 3)))
    # 3-D, nothing but the kernel fitted
    yield GP(1.1 * kernels.ExpSquaredKernel([1.0, 0.5, 2.0], ndim=3)), rng.uniform(0, 3, (40, 3))


@pytest.mark.parametrize("case", range(4))
def test_assembly_matches_the_one_vector_path(case):
    gp, x = list(_cases())[case]
    rng = np.random.RandomState(case)
    _pretend_computed(gp, x, 0.05 + 0.01 * rng.rand(len(x)))
    p0 = gp.get_parameter_vector()
    B, n = 7, len(x)
    vectors = p0 + 1e-2 * rng.randn(B, len(p0))
    alpha, diagA = rng.randn(B, n), rng.randn(B, n)
    kgrad = rng.randn(B, gp.kernel.full_size)
    grad, ok = gp._assemble_grad_batch(vectors, alpha, diagA, kgrad)
    assert ok.all() and grad.shape == (B, len(gp))
    assert np.array_equal(gp.get_parameter_vector(), p0)
    for b, v in enumerate(vectors):
        gp.set_parameter_vector(v)
        expect = gp._assemble_grad(alpha[b], diagA[b], kgrad[b][gp.kernel.unfrozen_mask], True)
        assert np.array_equal(grad[b], expect), b
    gp.set_parameter_vector(p0)


def test_a_mean_gradient_that_is_not_finite_zeroes_its_row():
    class LogMean(Model):
        parameter_names = ("a",)

        def get_value(self, t):
            return self.a * np.log(t)

    gp = GP(kernels.ExpSquaredKernel(1.0), mean=LogMean(a=1.0), white_noise=np.log(0.1), fit_white_noise=True)
    _pretend_computed(gp, np.linspace(0, 5, 10), 0.1)           # log(0): the finite-difference gradient is NaN at x = 0
    vectors = np.tile(gp.get_parameter_vector(), (3, 1))
    rng = np.random.RandomState(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        grad, ok = gp._assemble_grad_batch(vectors, rng.randn(3, 10), rng.randn(3, 10), rng.randn(3, 1))
    assert not ok.any() and (grad == 0).all()


def _gp(n=30, **kw):
    rng = np.random.RandomState(1)
    x = np.sort(rng.uniform(0, 10, n))
    gp = GP(0.5 * kernels.ExpSquaredKernel(1.0), mean=ConstantModel(0.1, bounds=dict(value=(-1.0, 1.0))),
            white_noise=np.log(0.02), fit_white_noise=True, **kw)
    _pretend_computed(gp, x, 0.1)
    return gp, np.sin(x)


class _StandIn(object):
    """replaces BasicSolver.objective_grad_batch: records the rows it is given and returns made-up values (info[b] = 3
    for the rows listed in ``fail``)"""

    def __init__(self, fail=()):
        self.calls, self.fail = [], set(fail)

    def __call__(self, solver, params, x, sigma, r, which=None):
        self.calls.append(np.array(params))
        B, n = len(params), len(x)
        info = np.array([3 if tuple(p) in self.fail else 0 for p in params], dtype=np.int64)
        logdet, quad = np.sum(params, axis=1), np.ones(B)
        grad, alpha, diagA = 2.0 * params, 0.1 * r, 0.01 * sigma
        for a in (logdet, quad, grad, alpha, diagA):
            a[info != 0] = np.nan
        return logdet, quad, grad, alpha, diagA, info


def test_checks_before_any_device_call(monkeypatch):
    stand_in = _StandIn()
    monkeypatch.setattr(BasicSolver, "objective_grad_batch", lambda s, *a, **k: stand_in(s, *a, **k))
    gp, y = _gp()
    P = len(gp)
    with pytest.raises(ValueError):
        gp.nll_and_grad_batch(np.zeros((3, P + 1)), y)
    with pytest.raises(ValueError):
        gp.grad_log_likelihood_batch(np.zeros(P), y)
    with pytest.raises(ValueError):
        gp.nll_and_grad_batch(np.zeros((3, P)), y[:-1])
    with pytest.raises(RuntimeError):
        GP(kernels.ExpSquaredKernel(1.0)).grad_log_likelihood_batch(np.zeros((1, 2)), y)
    nll, g = gp.nll_and_grad_batch(np.zeros((0, P)), y)
    assert nll.shape == (0,) and g.shape == (0, P)
    assert gp.grad_log_likelihood_batch(np.zeros((0, P)), y).shape == (0, P)
    # every row outside the prior: nothing is evaluated
    vec = np.tile(gp.get_parameter_vector(), (4, 1))
    vec[:, 0] = 5.0
    nll, g = gp.nll_and_grad_batch(vec, y)
    assert (nll == np.inf).all() and (g == 0).all() and not stand_in.calls


def test_prior_rows_and_failures_around_the_device_call(monkeypatch):
    gp, y = _gp()
    p0 = gp.get_parameter_vector()
    rng = np.random.RandomState(2)
    vec = p0 + 1e-2 * rng.randn(6, len(p0))
    vec[1, 0] = 5.0                                              # outside the mean's bounds
    kp = gp._batch_inputs(vec, y, True)[0]
    stand_in = _StandIn(fail=[tuple(kp[4])])
    monkeypatch.setattr(BasicSolver, "objective_grad_batch", lambda s, *a, **k: stand_in(s, *a, **k))
    nll, g = gp.nll_and_grad_batch(vec, y)
    assert len(stand_in.calls) == 1 and np.array_equal(stand_in.calls[0], kp[[0, 2, 3, 4, 5]])
    assert nll[1] == np.inf and (g[1] == 0).all() and nll[4] == np.inf and (g[4] == 0).all()
    assert np.isfinite(nll[[0, 2, 3, 5]]).all() and (g[[0, 2, 3, 5]] != 0).any(axis=1).all()
    # grad_log_likelihood_batch has no prior screen; the row names of errors are the caller's
    stand_in.calls.clear()
    G = gp.grad_log_likelihood_batch(vec, y)
    assert np.array_equal(stand_in.calls[0], kp) and (G[4] == 0).all()
    assert np.array_equal(G[[0, 2, 3, 5]], -g[[0, 2, 3, 5]])
    with pytest.raises(np.linalg.LinAlgError, match="member 4"):
        gp.nll_and_grad_batch(vec, y, quiet=False)
    with pytest.raises(np.linalg.LinAlgError, match="member 4"):
        gp.grad_log_likelihood_batch(vec, y, quiet=False)
    assert np.array_equal(gp.get_parameter_vector(), p0)


def test_grad_batch_bytes_formula():
    for n in (1, 127, 128, 129, 468, 1024, 4097, 8192):
        np_ = -(-n // 128) * 128
        nt, gm = np_ // 128, -(-n // 64)
        tiles = nt + 1 + nt * (nt + 1) // 2
        want = 8 * ((2 * np_ + 128) * np_ + np_ * 128 + tiles * 128 * 128 + 64 + 2 * n + gm * (gm + 1) // 2 * 64)
        assert BasicSolver.grad_batch_bytes(n) == want
    assert BasicSolver.grad_batch_bytes(BasicSolver.BATCH_MAX_N) <= BasicSolver.BATCH_MAX_BYTES


def test_routing_limits(monkeypatch):
    gp, _ = _gp(n=300)
    assert gp._grad_batch_on_device()
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 300)
    assert gp._grad_batch_on_device()
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 299)
    assert not gp._grad_batch_on_device()
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 8192)
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_BYTES", BasicSolver.grad_batch_bytes(300))
    assert gp._grad_batch_on_device()
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_BYTES", BasicSolver.grad_batch_bytes(300) - 1)
    assert not gp._grad_batch_on_device()
    monkeypatch.undo()
    hodlr, _ = _gp(n=300, solver=HODLRSolver)
    assert not hodlr._grad_batch_on_device()


def test_the_loop_route_runs_the_one_vector_path_on_the_host():
    # no kernel: the host TrivialSolver, so the per-vector loop runs here; rows must equal nll_and_grad / grad_log_likelihood
    rng = np.random.RandomState(4)
    x = np.sort(rng.uniform(0, 10, 25))
    y = np.sin(x) + 0.1 * rng.randn(25)
    gp = GP(mean=LinearMean(m=0.1, b=0.2), white_noise=np.log(0.05), fit_white_noise=True)
    gp.compute(x, 0.1)
    p0 = gp.get_parameter_vector()
    vec = p0 + 0.1 * rng.randn(5, len(p0))
    nll, g = gp.nll_and_grad_batch(vec, y)
    G = gp.grad_log_likelihood_batch(vec, y)
    assert np.array_equal(gp.get_parameter_vector(), p0) and gp.computed
    for b, v in enumerate(vec):
        n1, g1 = gp.nll_and_grad(v, y)
        assert n1 == nll[b] and np.array_equal(g1, g[b])
        gp.set_parameter_vector(v)
        assert np.array_equal(gp.grad_log_likelihood(y), G[b])
    gp.set_parameter_vector(p0)
