"""GP.predict_batch / sample_conditional_batch on the host side (no GPU): the mapping of (B, len(gp)) parameter vectors
to the per-member inputs of the batched device call (the mean model at the test points included), the argument checks
that run before any device call, the routing limits, and the order in which draws consume the random stream."""
import numpy as np
import pytest

from george_amd import GP, BasicSolver, kernels
from george_amd.modeling import Model


class LinearMean(Model):
    parameter_names = ("m", "b")

    def get_value(self, t):
        return self.m * t + self.b


def _pretend_computed(gp, x, yerr):
    # what compute() records before it factorises (the mapping needs nothing else)
    gp._x = np.ascontiguousarray(gp.parse_samples(x), dtype=np.float64)
    gp._yerr2 = np.ascontiguousarray(np.broadcast_to(yerr, (len(gp._x),)) ** 2, dtype=np.float64)


def _cases():
    rng = np.random.RandomState(3)
    x = np.sort(rng.uniform(0, 10, 40))
    t = np.linspace(-1, 11, 23)
    # a frozen kernel parameter, a fitted constant mean and fitted white noise
    k = 1.5 * kernels.Matern32Kernel(2.0)
    k.freeze_parameter("k1:log_constant")
    yield GP(k, mean=0.3, fit_mean=True, white_noise=np.log(0.01), fit_white_noise=True), x, t
    # a Model subclass mean (its value at t differs from its value at x), white noise, a frozen metric
    k = 0.7 * kernels.ExpSquaredKernel(1.2) + 0.2 * kernels.Matern52Kernel(0.5)
    k.freeze_parameter("k2:k2:metric:log_M_0_0")
    yield GP(k, mean=LinearMean(m=0.2, b=-1.0), white_noise=np.log(0.02), fit_white_noise=True), x, t
    # 3-D axis-aligned Matern52 + Constant, default mean and white noise
    yield (GP(2.0 * kernels.Matern52Kernel([1.0, 2.0, 0.5], ndim=3) + kernels.ConstantKernel(0.1, ndim=3)),
           rng.uniform(0, 3, (40, 3)), rng.uniform(0, 3, (23, 3)))


@pytest.mark.parametrize("case", range(3))
def test_inputs_with_test_points_match_the_one_vector_path(case):
    gp, x, t = list(_cases())[case]
    rng = np.random.RandomState(case)
    y = np.sin(np.atleast_2d(x.T)[0]) + 0.1 * rng.randn(len(x))
    _pretend_computed(gp, x, 0.05 + 0.01 * rng.rand(len(x)))
    xs = np.ascontiguousarray(gp.parse_samples(t), dtype=np.float64)
    p0 = gp.get_parameter_vector()
    vectors = p0 + 1e-2 * rng.randn(7, len(p0))
    kp, sig, res, ok, mean_t = gp._batch_inputs(vectors, y, quiet=True, t=xs)
    for b, v in enumerate(vectors):
        gp.set_parameter_vector(v)
        assert np.array_equal(kp[b], gp.kernel.get_parameter_vector(include_frozen=True))
        assert np.array_equal(sig[b], np.sqrt(gp._yerr2 + np.exp(gp._call_white_noise(gp._x))))
        assert np.array_equal(res[b], y - gp._call_mean(gp._x))
        assert np.array_equal(mean_t[b], gp._call_mean(xs))
    gp.set_parameter_vector(p0)
    assert ok.all() and mean_t.shape == (7, len(xs))
    # without test points the tuple of log_likelihood_batch is what it was
    four = gp._batch_inputs(vectors, y, quiet=True)
    assert len(four) == 4 and all(np.array_equal(a, b) for a, b in zip(four, (kp, sig, res, ok)))
    assert np.array_equal(gp.get_parameter_vector(), p0)


def test_a_mean_that_fails_only_at_the_test_points_is_flagged():
    class LogMean(Model):
        parameter_names = ("a",)

        def get_value(self, t):
            return self.a * np.log(t)

    gp = GP(kernels.ExpSquaredKernel(1.0), mean=LogMean(a=1.0))
    x = np.linspace(1, 5, 10)
    _pretend_computed(gp, x, 0.1)
    xs = np.ascontiguousarray(gp.parse_samples(np.array([-1.0, 2.0])), dtype=np.float64)
    vectors = np.tile(gp.get_parameter_vector(), (3, 1))
    vectors[0, 0] = 0.0                                             # 0 * log(-1) is NaN too
    with np.errstate(invalid="ignore"):
        _, _, _, ok4 = gp._batch_inputs(vectors, np.zeros(10), quiet=True)
        _, _, _, ok, _ = gp._batch_inputs(vectors, np.zeros(10), quiet=True, t=xs)
        assert ok4.all() and not ok.any()
        with pytest.raises(ValueError, match="member 0"):
            gp._batch_inputs(vectors, np.zeros(10), quiet=False, t=xs)
        with pytest.raises(ValueError, match="member 0"):
            gp.predict_batch(vectors, np.zeros(10), np.array([-1.0, 2.0]))


def test_argument_checks_before_any_device_call():
    gp = GP(kernels.ExpSquaredKernel(1.0))
    p = gp.get_parameter_vector()
    t = np.linspace(0, 1, 4)
    with pytest.raises(RuntimeError, match="compute"):
        gp.predict_batch(p[None, :], np.zeros(5), t)
    with pytest.raises(RuntimeError, match="compute"):
        gp.sample_conditional_batch(p[None, :], np.zeros(5), t)
    _pretend_computed(gp, np.linspace(0, 1, 5), 0.1)
    with pytest.raises(ValueError):
        gp.predict_batch(np.zeros((3, len(p) + 1)), np.zeros(5), t)         # wrong width
    with pytest.raises(ValueError):
        gp.predict_batch(p, np.zeros(5), t)                                 # 1-D vectors
    with pytest.raises(ValueError):
        gp.predict_batch(p[None, :], np.zeros(6), t)                        # wrong y length
    with pytest.raises(ValueError):
        gp.predict_batch(p[None, :], np.zeros(5), np.zeros((4, 2)))         # test points of the wrong dimension
    # the solver layer: shapes are ValueError, a dimension mismatch RuntimeError
    s = BasicSolver(gp.kernel)
    x, xs = np.zeros((5, 1)), np.zeros((4, 1))
    kp = np.tile(gp.kernel.get_parameter_vector(include_frozen=True), (2, 1))
    with pytest.raises(ValueError):
        s.predict_batch(kp[:, :0], x, 0.1, np.zeros((2, 5)), xs)
    with pytest.raises(ValueError):
        s.predict_batch(kp, x, 0.1, np.zeros((2, 4)), xs)
    with pytest.raises(ValueError):
        s.predict_batch(kp, x, 0.1, np.zeros((2, 5)), np.zeros(4))
    with pytest.raises(RuntimeError):
        s.predict_batch(kp, x, 0.1, np.zeros((2, 5)), np.zeros((4, 2)))
    with pytest.raises(RuntimeError):
        s.predict_batch(kp, np.zeros((5, 2)), 0.1, np.zeros((2, 5)), np.zeros((4, 2)))
    # B = 0 returns empty arrays of the documented shapes without a device call
    mu, cov = gp.predict_batch(np.zeros((0, len(p))), np.zeros(5), t)
    assert mu.shape == (0, 4) and cov.shape == (0, 4, 4)
    mu, var = gp.predict_batch(np.zeros((0, len(p))), np.zeros(5), t, return_var=True, return_cov=True)
    assert mu.shape == (0, 4) and var.shape == (0, 4)
    assert gp.predict_batch(np.zeros((0, len(p))), np.zeros(5), t, return_cov=False).shape == (0, 4)
    out = s.predict_batch(kp[:0], x, 0.1, np.zeros((0, 5)), xs, return_var=True)
    assert out[0].shape == (0, 4) and out[1].shape == (0, 4) and out[2] is None and out[3].shape == (0,)


def test_routing_limits_are_documented_defaults():
    assert BasicSolver.BATCH_MAX_N == 8192
    assert BasicSolver.BATCH_MAX_BYTES == 8 << 30
    assert callable(getattr(BasicSolver, "predict_batch", None))
    # one member: panel (Np + 128 + Mp) x Np, the diagonal inverses, the output tiles, the results
    assert BasicSolver.predict_batch_bytes(468, 250) == ((512 + 128 + 256) * 512 + 512 * 128 + 3 * 128 ** 2 + 250) * 8
    assert BasicSolver.predict_batch_bytes(468, 250, return_var=True) == \
        ((512 + 128 + 256) * 512 + 512 * 128 + 5 * 128 ** 2 + 500) * 8
    assert BasicSolver.predict_batch_bytes(468, 250, return_cov=True) == \
        ((512 + 128 + 256) * 512 + 512 * 128 + 6 * 128 ** 2 + 250 + 250 ** 2) * 8
    assert BasicSolver.predict_batch_bytes(468, 250, True, True) == BasicSolver.predict_batch_bytes(468, 250, True)


class _Recorder(object):
    """Stands in for the routes of predict_batch: records which one ran, returns the one-vector answers it is given."""

    def __init__(self, answer):
        self.answer, self.calls = answer, []

    def __call__(self, route):
        def run(vectors, y, xs, want_var, want_cov, quiet):
            self.calls.append((route, want_var, want_cov, quiet, len(vectors)))
            return self.answer(vectors, xs, want_var, want_cov)
        return run


def _fake_answer(vectors, xs, want_var, want_cov):
    B, m = len(vectors), len(xs)
    mu = np.arange(B * m, dtype=float).reshape(B, m)
    return mu, (np.ones((B, m)) if want_var else None), (np.tile(np.eye(m), (B, 1, 1)) if want_cov else None)


def test_routing_and_return_modes(monkeypatch):
    gp = GP(kernels.ExpSquaredKernel(1.0))
    p = gp.get_parameter_vector()
    _pretend_computed(gp, np.linspace(0, 1, 5), 0.1)
    rec = _Recorder(_fake_answer)
    monkeypatch.setattr(gp, "_predict_batch_device", rec("device"))
    monkeypatch.setattr(gp, "_predict_batch_loop", rec("loop"))
    v = np.tile(p, (3, 1))
    t = np.linspace(0, 1, 4)
    mu, cov = gp.predict_batch(v, np.zeros(5), t)
    assert mu.shape == (3, 4) and cov.shape == (3, 4, 4)
    mu, var = gp.predict_batch(v, np.zeros(5), t, return_var=True)                 # return_var wins
    assert var.shape == (3, 4)
    assert gp.predict_batch(v, np.zeros(5), t, return_cov=False).shape == (3, 4)
    assert [c[:4] for c in rec.calls] == [("device", False, True, False), ("device", True, False, False),
                                          ("device", False, False, False)]
    rec.calls.clear()
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 4)                             # N = 5 > BATCH_MAX_N
    gp.predict_batch(v, np.zeros(5), t, quiet=True)
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 8192)
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_BYTES", BasicSolver.predict_batch_bytes(5, 4, False, True) - 1)
    gp.predict_batch(v, np.zeros(5), t)                                            # one member does not fit
    gp.predict_batch(v, np.zeros(5), t, return_cov=False)                          # ... but without cov it does
    gp.solver_type = type("OtherSolver", (BasicSolver,), {})
    gp.predict_batch(v, np.zeros(5), t)                                            # not the BasicSolver itself
    assert [c[0] for c in rec.calls] == ["loop", "loop", "device", "loop"]
    assert rec.calls[0][3] is True


def test_sample_conditional_batch_consumes_the_stream_as_the_loop(monkeypatch):
    gp = GP(kernels.ExpSquaredKernel(1.0))
    p = gp.get_parameter_vector()
    _pretend_computed(gp, np.linspace(0, 1, 5), 0.1)
    B, m = 4, 6
    rng = np.random.RandomState(0)
    mus = rng.randn(B, m)
    A = rng.randn(B, m, m)
    covs = np.einsum("bij,bkj->bik", A, A)
    seen = []

    def fake_predict_batch(vectors, y, t, return_cov=True, return_var=False, quiet=False):
        seen.append((len(vectors), return_cov, return_var, quiet))
        return mus.copy(), covs.copy()

    monkeypatch.setattr(gp, "predict_batch", fake_predict_batch)
    v = np.tile(p, (B, 1))
    for size in (1, 3):
        np.random.seed(42)
        got = gp.sample_conditional_batch(v, np.zeros(5), np.linspace(0, 1, m), size=size)
        np.random.seed(42)
        want = [np.random.multivariate_normal(mus[b], covs[b], size) for b in range(B)]
        want = np.array([w[0] for w in want]) if size == 1 else np.array(want)
        assert got.shape == ((B, m) if size == 1 else (B, size, m))
        assert np.array_equal(got, want)
    assert seen == [(B, True, False, False)] * 2
