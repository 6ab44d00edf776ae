"""The solver protocol on the host: which class offers which optional call, who inherits from whom, what every call
does before ``compute`` and how right-hand sides are coerced.  No device is touched."""
import pickle

import numpy as np
import pytest

from george_amd import kernels
from george_amd.distributed import DistributedBasicSolver
from george_amd.solvers import BasicSolver, HODLRSolver, InducingSolver, MultiGPUHODLRSolver, MultiGPUSolver, VecchiaSolver
from george_amd.solvers.multigpu import _MultiDeviceSolver
from george_amd.solvers.protocol import NativeSolver, rhs_matrix, rhs_rows, rhs_vector

BATCH = ("objective_batch", "predict_batch", "sample_conditional_batch", "objective_grad_batch")
OPTIONAL = ("objective", "grad", "predict", "predict_gradient", "sample_conditional", "loo", "loo_objective", "lgo", "fisher",
            "append", "truncate", "remove", "profile") + BATCH
OFFERS = {
    BasicSolver: set(OPTIONAL),
    HODLRSolver: {"predict", "grad"},
    MultiGPUSolver: {"predict"},
    MultiGPUHODLRSolver: set(),
    DistributedBasicSolver: set(),
    VecchiaSolver: {"predict", "grad"},
    InducingSolver: {"predict", "grad"},
}
DENSE_ONLY = ("truncate", "append", "remove", "sample_conditional", "objective", "loo", "loo_objective", "lgo", "fisher",
              "predict_gradient", "_restore", "_ensure_batch_handle") + BATCH
CLASSES = list(OFFERS)
# the classes without ``apply_sqrt``, and what its message calls them
NO_SQRT = {HODLRSolver: "HODLRSolver", MultiGPUHODLRSolver: "HODLRSolver", VecchiaSolver: "VecchiaSolver",
           InducingSolver: "InducingSolver"}


def _kernel():
    return 1.0 * kernels.ExpSquaredKernel(1.0)


def _make(cls):
    if issubclass(cls, _MultiDeviceSolver):
        return cls(_kernel(), devices=[0, 0])
    return cls(_kernel())


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_capability_table(cls):
    assert {name for name in OPTIONAL if callable(getattr(cls, name, None))} == OFFERS[cls]


@pytest.mark.parametrize("cls", [HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver, VecchiaSolver, InducingSolver],
                         ids=lambda c: c.__name__)
def test_dense_only_calls_are_not_reachable(cls):
    for name in DENSE_ONLY:
        assert not callable(getattr(cls, name, None)), name
    s = _make(cls)
    for name in DENSE_ONLY:
        assert not callable(getattr(s, name, None)), name


def test_class_relations():
    assert not issubclass(HODLRSolver, BasicSolver)
    assert not issubclass(MultiGPUHODLRSolver, MultiGPUSolver) and not issubclass(MultiGPUSolver, MultiGPUHODLRSolver)
    for cls in (VecchiaSolver, InducingSolver):
        assert not any(issubclass(cls, other) or issubclass(other, cls) for other in CLASSES if other is not cls)
    for cls in (BasicSolver, HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver, VecchiaSolver, InducingSolver):
        assert issubclass(cls, NativeSolver)


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_no_method_comes_from_another_back_end(cls):
    # a method that takes a native handle is defined by the class that made the handle, by the multi-device base (which
    # creates the handle through the subclass's own entry points) or by the protocol base (which calls the entry points the
    # subclass names): nothing else may be on the way
    allowed = {cls, NativeSolver, object}
    if issubclass(cls, _MultiDeviceSolver):
        allowed.add(_MultiDeviceSolver)
    assert set(cls.__mro__) <= allowed
    for name in dir(cls):
        if name.startswith("_") or not callable(getattr(cls, name)):
            continue
        owner = next(c for c in cls.__mro__ if name in c.__dict__)
        assert owner in allowed, (name, owner)


def _calls_needing_a_factor(s):
    k, r, xs = s.kernel, np.zeros(3), np.zeros((2, 1))
    calls = {
        "apply_inverse": lambda: s.apply_inverse(r),
        "apply_inverse_in_place": lambda: s.apply_inverse(r, in_place=True),
        "dot_solve": lambda: s.dot_solve(r),
        "get_inverse": lambda: s.get_inverse(),
        "apply_sqrt": lambda: s.apply_sqrt(r),
        "predict": lambda: s.predict(k, r, xs, return_var=True),
        "grad": lambda: s.grad(r, np.ones(2, dtype=np.uint32)),
        "predict_gradient": lambda: s.predict_gradient(k, r, xs),
        "sample_conditional": lambda: s.sample_conditional(k, r, xs, np.zeros((1, 2))),
        "loo": lambda: s.loo(r),
        "lgo": lambda: s.lgo(r, np.arange(3), np.array([0, 3])),
        "fisher": lambda: s.fisher(),
        "append": lambda: s.append(xs, 0.1),
        "truncate": lambda: s.truncate(1),
        "remove": lambda: s.remove([0]),
        "profile": lambda: s.profile(),
        "ranks": lambda: s.ranks(),
        "rows": lambda: s.rows(),
    }
    return {name: call for name, call in calls.items() if callable(getattr(s, name.replace("_in_place", ""), None))}


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_before_compute(cls):
    s = _make(cls)
    assert not s.computed and s.log_determinant is None
    calls = _calls_needing_a_factor(s)
    assert {"apply_inverse", "dot_solve", "get_inverse", "apply_sqrt"} <= set(calls)
    assert OFFERS[cls] - {"objective", "loo_objective"} - set(BATCH) <= set(calls)
    for name, call in calls.items():
        if name == "apply_sqrt" and cls in NO_SQRT:
            with pytest.raises(NotImplementedError, match="^apply_sqrt is not implemented for the %s$" % NO_SQRT[cls]):
                call()
            continue
        with pytest.raises(RuntimeError, match="you must call 'compute' first"):
            call()


# ------------------------------------------------------------------ right-hand sides
N_PTS = 5


def test_rhs_matrix():
    rng = np.random.RandomState(0)
    v, m = rng.randn(N_PTS), rng.randn(N_PTS, 3)
    for y, nrhs in ((v, 1), (m, 3), (np.empty((N_PTS, 0)), 0)):
        yc, k = rhs_matrix(y, N_PTS)
        assert yc is y and k == nrhs                                   # contiguous float64: no copy
    for y in (np.asfortranarray(m), m[:, ::-1], rng.randn(2 * N_PTS, 3)[::2], m.astype(np.float32), m.tolist(),
              np.arange(N_PTS)):
        yc, k = rhs_matrix(y, N_PTS)
        assert yc.dtype == np.float64 and yc.flags.c_contiguous and yc.flags.writeable
        assert np.array_equal(yc, np.asarray(y, dtype=np.float64)) and k == (1 if yc.ndim == 1 else 3)
    ro = m.copy()
    ro.flags.writeable = False
    yc, k = rhs_matrix(ro, N_PTS)
    assert yc is ro and k == 3
    for bad in (np.float64(1.0), 1.0, np.zeros((N_PTS, 2, 2)), np.zeros(N_PTS + 1), np.zeros((N_PTS - 1, 3)), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            rhs_matrix(bad, N_PTS)


def test_rhs_vector():
    rng = np.random.RandomState(1)
    v = rng.randn(N_PTS)
    assert rhs_vector(v, N_PTS) is not None and np.shares_memory(rhs_vector(v, N_PTS), v)
    for y in (v[:, None], v[None, :], np.asfortranarray(v[:, None]), rng.randn(2 * N_PTS)[::2], v.astype(np.float32),
              v.tolist(), np.arange(N_PTS)):
        yc = rhs_vector(y, N_PTS)
        assert yc.shape == (N_PTS,) and yc.dtype == np.float64 and yc.flags.c_contiguous
        assert np.array_equal(yc, np.asarray(y, dtype=np.float64).reshape(-1))
    ro = v.copy()
    ro.flags.writeable = False
    assert np.array_equal(rhs_vector(ro, N_PTS), v)
    for bad in (np.float64(1.0), np.zeros(N_PTS + 1), np.zeros((N_PTS, 2)), np.zeros(0)):
        with pytest.raises(ValueError, match="dimension mismatch"):
            rhs_vector(bad, N_PTS)


def test_rhs_rows():
    rng = np.random.RandomState(2)
    v, m = rng.randn(N_PTS), rng.randn(3, N_PTS)
    r2, one_d = rhs_rows(v, N_PTS)
    assert one_d and r2.shape == (1, N_PTS) and np.array_equal(r2[0], v)
    r2, one_d = rhs_rows(m, N_PTS)
    assert not one_d and r2 is m
    assert rhs_rows(np.empty((0, N_PTS)), N_PTS)[0].shape == (0, N_PTS)
    for r in (np.asfortranarray(m), rng.randn(3, 2 * N_PTS)[:, ::2], m.astype(np.float32), m.tolist()):
        r2, one_d = rhs_rows(r, N_PTS)
        assert not one_d and r2.dtype == np.float64 and r2.flags.c_contiguous
        assert np.array_equal(r2, np.asarray(r, dtype=np.float64))
    ro = m.copy()
    ro.flags.writeable = False
    assert np.array_equal(rhs_rows(ro, N_PTS)[0], m)
    for bad in (np.float64(1.0), np.zeros((2, N_PTS, N_PTS)), np.zeros(N_PTS + 1), np.zeros((3, N_PTS - 1))):
        with pytest.raises(ValueError, match="dimension mismatch"):
            rhs_rows(bad, N_PTS)


@pytest.mark.parametrize("cls", [BasicSolver, HODLRSolver, MultiGPUSolver, MultiGPUHODLRSolver, VecchiaSolver, InducingSolver],
                         ids=lambda c: c.__name__)
def test_in_place_policy(cls):
    # (the policy alone: which array the native solve writes and which one gets the values back)
    s = _make(cls)
    y = np.zeros((N_PTS, 3))
    views = {"contiguous": y, "fortran": np.asfortranarray(y), "strided": np.zeros((2 * N_PTS, 3))[::2]}
    for name, yin in views.items():
        yc = np.ascontiguousarray(yin)
        out, back = s._solve_target(yin, yc, False)
        assert back is None and out is not yin and out.shape == yc.shape and out.flags.c_contiguous
        out, back = s._solve_target(yin, yc, True)
        if cls is HODLRSolver:
            assert back is None and not np.shares_memory(out, yin)
        elif cls is BasicSolver and name == "contiguous":
            assert out is yin and back is None
        else:
            assert back is yin and not np.shares_memory(out, yin)
    ro = y.copy()
    ro.flags.writeable = False
    out, back = s._solve_target(ro, ro, True)
    assert out is not ro and out.flags.writeable
    if cls in (VecchiaSolver, InducingSolver):
        # these two copy back into every writable array, whatever its dtype, and never write into the caller's array
        assert back is None
        yi = np.zeros((N_PTS, 3), dtype=np.int64)
        out, back = s._solve_target(yi, np.ascontiguousarray(yi, dtype=np.float64), True)
        assert back is yi and out.dtype == np.float64 and not np.shares_memory(out, yi)
        out, back = s._solve_target(yi.tolist(), np.ascontiguousarray(yi, dtype=np.float64), True)
        assert back is None


@pytest.mark.parametrize("cls", CLASSES, ids=lambda c: c.__name__)
def test_pickle_round_trip_of_an_uncomputed_solver(cls):
    s = _make(cls)
    t = pickle.loads(pickle.dumps(s, -1))
    assert type(t) is cls and not t.computed and t.log_determinant is None
    assert t.kernel.get_parameter_vector().tolist() == s.kernel.get_parameter_vector().tolist()
    if cls is not DistributedBasicSolver:
        assert t._handle is None
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        t.dot_solve(np.zeros(3))
