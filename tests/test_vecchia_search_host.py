"""The device-side neighbour search of the Vecchia solver, as far as the host reaches: the two ABI entries and their argument
checks (host code, run before any device call), the ``search=`` option and its pickling, ``device=None`` leaving the host
search as it is, and -- where no device is visible -- the loud failure of everything that would need one.  No device is touched.
"""
import ctypes
import inspect
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import GP, kernels
from george_amd import _native as N
from george_amd.solvers import VecchiaSolver
from george_amd.solvers.vecchia import vecchia_neighbors, vecchia_query_neighbors

import vecchia_local_ref
import vecchia_ref


def _search(x, q, m, limit=None, n=None, nq=None, ndim=None, occupancy=0, table=True):
    x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    q = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
    n = len(x) if n is None else n
    nq = len(q) if nq is None else nq
    ndim = x.shape[1] if ndim is None else ndim
    out = np.full((max(nq, 0), max(m, 1)), 7, dtype=np.int32) if table else None
    rc = N.lib.gh_vecchia_search(0, N.ptr(x), n, ndim, N.ptr(q), nq, N.ptr(limit), m, occupancy, N.ptr(out))
    return rc, out


def test_entry_points_are_declared_and_exported():
    for name in ("gh_vecchia_search", "gh_vecchia_predict_local_search"):
        assert name in N.SIGNATURES and hasattr(N.lib, name)
    assert len(N.SIGNATURES["gh_vecchia_search"][1]) == 10
    assert len(N.SIGNATURES["gh_vecchia_predict_local_search"][1]) == 11
    assert len(N.SIGNATURES["gh_vecchia_predict_local"][1]) == 10          # (unchanged)
    assert ctypes.sizeof(N.gh_vecchia_opts) == 16


def test_argument_checks_run_on_the_host():
    x, q = np.random.RandomState(0).rand(9, 3), np.random.RandomState(1).rand(4, 3)
    for m in (0, -1, 65):
        assert _search(x, q, m)[0] == N.GH_ERR_BAD_ARG
    assert _search(None, q, 3, n=9, ndim=3)[0] == N.GH_ERR_BAD_ARG
    assert _search(x, None, 3, nq=4)[0] == N.GH_ERR_BAD_ARG
    assert _search(x, q, 3, table=False)[0] == N.GH_ERR_BAD_ARG
    assert _search(x, q, 3, n=-1)[0] == N.GH_ERR_BAD_ARG
    assert _search(x, q, 3, occupancy=-2)[0] == N.GH_ERR_BAD_ARG
    for ndim in (0, -3, N.GH_MAX_NDIM + 1):
        assert _search(x, q, 3, ndim=ndim)[0] == N.GH_ERR_DIM
    with pytest.raises(ValueError):
        N.check(_search(x, q, 65)[0])
    with pytest.raises(RuntimeError):
        N.check(_search(x, q, 3, ndim=17)[0])
    # the fused call: a null handle is refused before anything else
    assert N.lib.gh_vecchia_predict_local_search(None, None, None, None, None, 1, 3, 0, None, None, None) == N.GH_ERR_BAD_ARG


def test_empty_inputs_give_a_table_of_minus_one_and_do_no_work():
    x, q = np.zeros((0, 2)), np.random.RandomState(1).rand(4, 2)
    rc, out = _search(x, q, 3)
    assert rc == N.GH_OK and np.array_equal(out, np.full((4, 3), -1))       # n == 0: no device is needed
    rc, out = _search(np.ones((5, 2)), q[:0], 3)
    assert rc == N.GH_OK and out.shape == (0, 3)
    assert np.array_equal(vecchia_query_neighbors(x, q, 3, device=0), np.full((4, 3), -1))
    assert vecchia_neighbors(x, 3, device=0).shape == (0, 3)


def test_search_option_is_checked_and_pickled():
    k = 1.0 * kernels.ExpSquaredKernel(1.0)
    with pytest.raises(ValueError):
        VecchiaSolver(k, search="smoke")
    with pytest.raises(ValueError):
        VecchiaSolver(k, search=None)
    assert VecchiaSolver(k).search == "host"
    assert inspect.signature(VecchiaSolver.__init__).parameters["search"].default == "host"
    assert inspect.signature(VecchiaSolver.predict_local).parameters["search"].default is None
    assert inspect.signature(vecchia_query_neighbors).parameters["device"].default is None
    assert inspect.signature(vecchia_neighbors).parameters["device"].default is None
    for mode in ("host", "device"):
        s = pickle.loads(pickle.dumps(VecchiaSolver(k, m=5, search=mode, predict="local")))
        assert s.search == mode and s.predict_mode == "local" and s.m == 5 and not s.computed
    gp = pickle.loads(pickle.dumps(GP(k, solver=VecchiaSolver, search="device", predict="local")))
    assert gp.solver_kwargs["search"] == "device"


@pytest.mark.parametrize("ndim", [1, 3])
def test_device_none_is_the_host_search(ndim):
    rng = np.random.RandomState(5)
    x, t = rng.rand(400, ndim), rng.rand(60, ndim)
    assert np.array_equal(vecchia_query_neighbors(x, t, 7, device=None), vecchia_query_neighbors(x, t, 7))
    assert np.array_equal(vecchia_query_neighbors(x, t, 7, device=None), vecchia_local_ref.query_neighbors(x, t, 7))
    assert np.array_equal(vecchia_neighbors(x, 7, device=None), vecchia_neighbors(x, 7))
    assert np.array_equal(vecchia_neighbors(x, 7, device=None), vecchia_ref.brute_force_neighbors(x, 7))
    assert vecchia_query_neighbors(x, t, 100, device=None).shape == (60, 100)       # (the host search has no cap on m)
    with pytest.raises(ValueError):
        vecchia_query_neighbors(x, t, 65, device=0)
    with pytest.raises(ValueError):
        vecchia_neighbors(x, 65, device=0)


def test_device_search_fails_loudly_without_a_device():
    if george_amd.device_count() > 0:
        return                                              # (a device is visible: tests/test_gpu_vecchia_search.py runs the search)
    rng = np.random.RandomState(6)
    x, t = rng.rand(50, 2), rng.rand(8, 2)
    with pytest.raises(RuntimeError):
        vecchia_query_neighbors(x, t, 4, device=0)
    with pytest.raises(RuntimeError):
        vecchia_neighbors(x, 4, device=0)
    k = 1.0 * kernels.ExpSquaredKernel(1.0, ndim=2)
    with pytest.raises(RuntimeError):
        VecchiaSolver(k, m=4, search="device").compute(x, 0.1 * np.ones(50))
    gp = GP(k, solver=VecchiaSolver, m=4, search="device", predict="local")
    with pytest.raises(RuntimeError):
        gp.compute(x, 0.1)
