"""The device-side selection of inducing points, as far as the host reaches: the NumPy restatement (``maxmin_ref.maxmin``)
against ``inducing_points``, ``return_dmin`` on the host route, the ABI entry ``gh_inducing_select`` and its argument checks
(host code, run before any device call), the ``select=`` option, and -- where no device is visible -- the loud failure of
everything that would need one.  No device is touched.
"""
import ctypes
import inspect
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import GP, kernels
from george_amd import _native as N
from george_amd.solvers import InducingSolver
from george_amd.solvers.inducing import inducing_points

import maxmin_ref


def _select(x, m, first=0, n=None, ndim=None, idx=True, dmin=False):
    x = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
    n = len(x) if n is None else n
    ndim = x.shape[1] if ndim is None else ndim
    out = np.full(max(min(m, n), 1), -7, dtype=np.int64) if idx else None
    dm = np.full(max(n, 1), -7.0) if dmin else None
    rc = N.lib.gh_inducing_select(0, N.ptr(x), n, ndim, first, m, N.ptr(out), N.ptr(dm))
    return rc, out, dm


def test_entry_point_is_declared_and_exported():
    assert "gh_inducing_select" in N.SIGNATURES and hasattr(N.lib, "gh_inducing_select")
    res, args = N.SIGNATURES["gh_inducing_select"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[0] is ctypes.c_int32 and args[3] is ctypes.c_int32
    assert args[2] is ctypes.c_int64 and args[4] is ctypes.c_int64 and args[5] is ctypes.c_int64


@pytest.mark.parametrize("m", [1, 2, 64, 300])
@pytest.mark.parametrize("kind", maxmin_ref.KINDS)
def test_reference_equals_the_host_routine(kind, m):
    x = maxmin_ref.data(kind)
    want_idx, want_dmin = maxmin_ref.reference(kind, m)
    assert np.array_equal(inducing_points(x, m), want_idx)
    idx, dmin = inducing_points(x, m, return_dmin=True)
    assert idx.dtype == np.int64 and dmin.dtype == np.float64
    assert np.array_equal(idx, want_idx) and np.array_equal(dmin, want_dmin)
    assert np.array_equal(inducing_points(x, m, device=None), want_idx)
    if kind == "all_equal":
        assert np.all(idx[1:] == 0) and np.all(dmin == 0.0)
    if kind == "lattice" and m == 300:
        assert len(set(idx[:144].tolist())) == 144 and np.all(idx[144:] == 0)         # exhausted data: index 0 again and again


def test_dmin_is_the_distance_to_the_chosen_set():
    x = maxmin_ref.data("3d")
    idx, dmin = inducing_points(x, 40, return_dmin=True)
    want = ((x[:, None, :] - x[idx][None, :, :]) ** 2).sum(axis=-1).min(axis=1)
    assert np.array_equal(dmin, want)
    assert np.all(dmin[idx] == 0.0)
    idx, dmin = inducing_points(x[:0], 3, return_dmin=True)
    assert idx.shape == (0,) and dmin.shape == (0,)
    idx, dmin = inducing_points(x[:5], 9, return_dmin=True)
    assert sorted(idx.tolist()) == [0, 1, 2, 3, 4] and np.all(dmin == 0.0)


def test_argument_checks_run_on_the_host():
    x = np.random.RandomState(0).rand(9, 3)
    for m in (0, -1):
        assert _select(x, m)[0] == N.GH_ERR_BAD_ARG
    assert _select(x, 3, n=-1)[0] == N.GH_ERR_BAD_ARG
    assert _select(x, 3, n=0x7ffffff1)[0] == N.GH_ERR_BAD_ARG
    assert _select(x, 3, idx=False)[0] == N.GH_ERR_BAD_ARG
    assert _select(None, 3, n=9, ndim=3)[0] == N.GH_ERR_BAD_ARG
    for first in (-1, 9, 1 << 40):
        assert _select(x, 3, first=first)[0] == N.GH_ERR_BAD_ARG
    for ndim in (0, -3, N.GH_MAX_NDIM + 1):
        assert _select(x, 3, ndim=ndim)[0] == N.GH_ERR_DIM
    with pytest.raises(ValueError):
        N.check(_select(x, 0)[0])
    with pytest.raises(RuntimeError):
        N.check(_select(x, 3, ndim=17)[0])


def test_no_points_write_nothing_and_need_no_device():
    rc, idx, dmin = _select(np.zeros((0, 2)), 3, first=5, dmin=True)          # (first is not looked at without points)
    assert rc == N.GH_OK and np.all(idx == -7) and np.all(dmin == -7.0)
    rc, idx, _ = _select(None, 3, n=0, ndim=2)
    assert rc == N.GH_OK and np.all(idx == -7)
    assert inducing_points(np.zeros((0, 2)), 3, device=0).shape == (0,)


def test_select_option_is_checked_and_pickled():
    k = 1.0 * kernels.ExpSquaredKernel(1.0)
    for bad in ("gpu", None, 0):
        with pytest.raises(ValueError):
            InducingSolver(k, select=bad)
    assert InducingSolver(k).select == "host"
    assert inspect.signature(InducingSolver.__init__).parameters["select"].default == "host"
    assert inspect.signature(inducing_points).parameters["device"].default is None
    assert inspect.signature(inducing_points).parameters["return_dmin"].default is False
    for mode in ("host", "device"):
        s = pickle.loads(pickle.dumps(InducingSolver(k, inducing=5, select=mode)))
        assert s.select == mode and s.inducing == 5 and not s.computed
    gp = pickle.loads(pickle.dumps(GP(k, solver=InducingSolver, inducing=7, select="device")))
    assert gp.solver_kwargs["select"] == "device"


def test_device_route_refuses_points_that_are_not_finite():
    x = np.random.RandomState(1).rand(20, 2)
    for bad in (np.nan, np.inf, -np.inf):
        xb = x.copy()
        xb[7, 1] = bad
        with pytest.raises(ValueError):
            inducing_points(xb, 4, device=0)
    with pytest.raises(ValueError):
        inducing_points(x, 0, device=0)


def test_device_selection_fails_loudly_without_a_device():
    if george_amd.device_count() > 0:
        pytest.skip("a GPU is visible")
    x = np.random.RandomState(2).rand(50, 2)
    assert _select(x, 4)[0] == N.GH_ERR_HIP
    with pytest.raises(RuntimeError):
        inducing_points(x, 4, device=0)
    with pytest.raises(RuntimeError):
        inducing_points(x, 4, device=0, return_dmin=True)
    k = 1.0 * kernels.ExpSquaredKernel(1.0, ndim=2)
    with pytest.raises(RuntimeError):
        InducingSolver(k, inducing=4, select="device").compute(x, 0.1 * np.ones(50))
    gp = GP(k, solver=InducingSolver, inducing=4, select="device")
    with pytest.raises(RuntimeError):
        gp.compute(x, 0.1)
