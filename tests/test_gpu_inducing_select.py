"""The greedy max-min selection on the device (``gh_inducing_select``, george_amd/csrc/gh_inducing_select.hip) against the NumPy
restatement ``maxmin_ref.maxmin``, whose squared distance is the device's left-to-right sum in any dimension: the indices and
``dmin`` are compared with ``np.array_equal``, bit for bit.  Up to 7 dimensions the host routine ``inducing_points(x, m)`` is
compared too; from 8 on NumPy adds pairwise and only the restatement is the reference.

The grid has one workgroup per 1024 points, at most 1024 of them, and the last workgroup reduces the partial keys 256 at a time:
1500 points use two workgroups, 40 000 use 40, 300 000 use 293 (a second round of the reduction of the partials) and 1 100 000
use 1024 with a second round of the threads' walk over the points.  The lattices put exact ties across every one of these seams.
"""
import numpy as np
import pytest

import devptr
from devptr import Out
from george_amd import GP, InducingSolver, kernels
from george_amd import _native as N
from george_amd.solvers import inducing
from george_amd.solvers.inducing import inducing_points

import maxmin_ref

pytestmark = pytest.mark.gpu

L = N.lib
MS = [1, 2, 64, 300]


def _device(x, m, first=None, want_dmin=True):
    """``gh_inducing_select`` on host arrays: (idx, dmin or None); ``first`` defaults to the centroid rule"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    first = maxmin_ref.centroid_first(x) if first is None else first
    idx = np.full(min(m, n), -7, dtype=np.int64)
    dmin = np.full(n, -7.0) if want_dmin else None
    N.check(L.gh_inducing_select(0, N.ptr(x), n, x.shape[1], first, m, N.ptr(idx), N.ptr(dmin)))
    return idx, dmin


def _assert_equal(got, want, what):
    idx, dmin = got
    widx, wdmin = want
    bad = np.flatnonzero(idx != widx)
    assert idx.shape == widx.shape and not len(bad), (what, "pick", bad[:5], idx[bad[:5]], widx[bad[:5]])
    bad = np.flatnonzero(dmin != wdmin)
    assert dmin.shape == wdmin.shape and not len(bad), (what, "dmin", bad[:5], dmin[bad[:5]], wdmin[bad[:5]])


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", maxmin_ref.KINDS)
def test_selection_equals_the_restatement_and_the_host_route(kind, m):
    x = maxmin_ref.data(kind)
    want = maxmin_ref.reference(kind, m)
    _assert_equal(_device(x, m), want, (kind, m))
    _assert_equal(inducing_points(x, m, device=0, return_dmin=True), inducing_points(x, m, return_dmin=True), (kind, m, "routes"))
    assert np.array_equal(inducing_points(x, m, device=0), want[0])
    if kind == "all_equal":
        assert np.all(want[0][1:] == 0)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", maxmin_ref.KINDS_MANY_DIMS)
def test_many_dimensions_equal_the_restatement(kind, m):
    _assert_equal(_device(maxmin_ref.data(kind), m), maxmin_ref.reference(kind, m), (kind, m))


@pytest.mark.parametrize("extra", [0, 5])
def test_full_ordering(extra):
    x = maxmin_ref.data("3d")
    n = len(x)
    idx, dmin = _device(x, n + extra)
    _assert_equal((idx, dmin), maxmin_ref.reference("3d", n + extra), extra)
    assert idx.shape == (n,) and np.array_equal(np.sort(idx), np.arange(n))     # min(m, N) picks: a permutation
    assert np.all(dmin == 0.0)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1500])
def test_sizes_around_the_wavefront_and_the_workgroup(n):
    _assert_equal(_device(maxmin_ref.data("3d", n), 40), maxmin_ref.reference("3d", 40, n), n)


@pytest.mark.parametrize("kind,n,m", [("3d", 40000, 40), ("lattice", 40000, 40), ("3d", 300000, 8), ("lattice", 300000, 8),
                                      ("1d_unsorted", 1100000, 4), ("lattice", 1100000, 4)])
def test_many_workgroups(kind, n, m):
    """40 workgroups at 40 000 points; 293 at 300 000: the partial keys are reduced in two rounds; 1024 at 1 100 000: a thread
    walks the points in two rounds.  On the lattices exact ties span every workgroup boundary and the lower index must win."""
    _assert_equal(_device(maxmin_ref.data(kind, n), m), maxmin_ref.reference(kind, m, n), (kind, n, m))


@pytest.mark.parametrize("kind", ["3d", "lattice"])
def test_first_point_from_the_caller(kind):
    x = maxmin_ref.data(kind)
    for first in (0, len(x) - 1, 777):
        idx, dmin = _device(x, 64, first=first)
        assert idx[0] == first
        _assert_equal((idx, dmin), maxmin_ref.reference(kind, 64, first=first), (kind, first))


def test_pointer_routes():
    """``x`` as device memory (also 8-byte aligned only), ``dmin_out`` as device memory and as NULL; ``idx_out`` is host memory"""
    x = maxmin_ref.data("3d")
    n, m = len(x), 64
    first = maxmin_ref.centroid_first(x)
    want = maxmin_ref.reference("3d", m)
    res = devptr.check_routes("gh_inducing_select",
                              lambda p: L.gh_inducing_select(0, p["x"], n, 3, first, m, p["idx_out"], p["dmin_out"]),
                              {"x": x}, {"idx_out": Out((m,), np.int64), "dmin_out": Out((n,), np.float64)},
                              host_only=("idx_out",), odd=("x",))
    for route, (rc, out) in res.items():
        assert rc == N.GH_OK
        _assert_equal((out["idx_out"], out["dmin_out"]), want, route)
    res = devptr.check_routes("gh_inducing_select",
                              lambda p: L.gh_inducing_select(0, p["x"], n, 3, first, m, p["idx_out"], None),
                              {"x": x}, {"idx_out": Out((m,), np.int64)}, host_only=("idx_out",), odd=("x",))
    for route, (rc, out) in res.items():
        assert rc == N.GH_OK and np.array_equal(out["idx_out"], want[0]), route
    idx, none = _device(x, m, want_dmin=False)
    assert none is None and np.array_equal(idx, want[0])
    assert np.array_equal(_device(x, 1, want_dmin=False)[0], want[0][:1])       # (no step at all)


def test_two_calls_give_the_same_bits_and_a_smaller_call_after_a_larger_one():
    """the pooled buffers of the larger call come back with its contents, and the ticket must stand at zero again"""
    small, big = maxmin_ref.data("lattice"), maxmin_ref.data("3d", 40000)
    fresh = _device(small, 200)
    _assert_equal(fresh, maxmin_ref.reference("lattice", 200), "fresh")
    _assert_equal(_device(big, 40), maxmin_ref.reference("3d", 40, 40000), "big")
    for what in ("after a larger call", "again"):
        _assert_equal(_device(small, 200), fresh, what)
    _assert_equal(_device(big, 40), maxmin_ref.reference("3d", 40, 40000), "big again")
    _assert_equal(_device(maxmin_ref.data("3d", 257), 40), maxmin_ref.reference("3d", 40, 257), "one workgroup after many")


# ------------------------------------------------------------------ end to end
def _problem():
    rng = np.random.RandomState(2000)
    x = rng.uniform(0, 2, (2000, 2))
    yerr = 0.1 + 0.05 * rng.rand(2000)
    y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.randn(2000)
    return 0.8 * kernels.ExpSquaredKernel([0.5, 0.7], ndim=2), x, yerr, y


def test_solver_and_gp_with_the_device_selection(monkeypatch):
    kernel, x, yerr, y = _problem()
    calls = []
    real = inducing.inducing_points

    def counted(*args, **kwargs):
        calls.append(kwargs.get("device"))
        return real(*args, **kwargs)

    monkeypatch.setattr(inducing, "inducing_points", counted)
    out = {}
    for mode in ("host", "device"):
        InducingSolver._TABLES[:] = []
        del calls[:]
        s = InducingSolver(kernel, inducing=128, jitter=1e-8, select=mode)
        s.compute(x, yerr)
        assert calls == [0 if mode == "device" else None]   # one selection, on the route asked for
        gp = GP(kernel, solver=InducingSolver, inducing=128, jitter=1e-8, select=mode)
        gp.compute(x, yerr)
        out[mode] = (s.u.copy(), s.log_determinant, s.dot_solve(y), gp.log_likelihood(y))
        before = len(calls)
        s.compute(x, yerr)                                  # the same data again: the kept selection
        gp.compute(x, yerr)
        assert len(calls) == before and np.array_equal(s.u, out[mode][0])
    assert out["host"][0].shape == (128, 2) and np.array_equal(out["host"][0], out["device"][0])
    assert out["host"][1:] == out["device"][1:]
    assert np.array_equal(out["host"][0], x[maxmin_ref.maxmin(x, 128, maxmin_ref.centroid_first(x))[0]])
