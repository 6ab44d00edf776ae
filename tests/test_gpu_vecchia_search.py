"""The exact nearest-neighbour search on the device (``vecchia_search_kernel``, george_amd/csrc/gh_vecchia_search.hip) against
the brute-force searches of the NumPy restatements (``vecchia_local_ref.query_neighbors``, ``vecchia_ref.brute_force_neighbors``),
and the calls built on it -- ``predict_local(search="device")``, ``compute`` with ``search="device"``, ``GP`` -- against the
host-search route of the same build, bit for bit.

Up to 7 input dimensions the device's squared distance is the double NumPy computes, so tables are compared with
``np.array_equal``, ties and near-ties included.  ``occupancy`` 2 makes a fine grid (many rings at m = 64), ``occupancy`` N the
one-cell grid (brute force on the device), 0 the automatic choice.  For 9 and 16 dimensions NumPy adds the squares pairwise and the
device left to right: two sums of at most 16 non-negative terms differ by at most about 30 eps relative, so a row S passes when
``min D[outside S] >= max D[S] (1 - 64 eps)`` under NumPy's distances D.
"""
import ctypes
import functools

import numpy as np
import pytest

import george_amd
from george_amd import GP, VecchiaSolver, kernels
from george_amd import _native as N
from george_amd.solvers import vecchia
from george_amd.solvers.vecchia import vecchia_neighbors, vecchia_query_neighbors

import vecchia_local_ref
import vecchia_ref

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KINDS = ["1d_unsorted", "2d", "3d", "5d", "lattice", "clusters", "const_col"]


@functools.lru_cache(maxsize=None)
def _data(kind):
    rng = np.random.RandomState(sum(map(ord, kind)))
    if kind == "1d_unsorted":
        x = rng.uniform(0, 10, (1500, 1))
    elif kind == "lattice":
        x = rng.randint(0, 12, (1500, 2)).astype(np.float64)            # repeated points, exact ties
    elif kind == "clusters":                                            # two tight clusters far apart: nearly every cell is empty
        x = 1e-3 * rng.randn(1000, 2)
        x[500:] += 100.0
        x = x[rng.permutation(1000)]
    elif kind == "const_col":                                           # an axis of zero extent
        x = rng.uniform(0, 1, (1500, 3))
        x[:, 1] = 0.25
    else:
        x = rng.uniform(0, 1, (1500, int(kind[0])))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _queries(kind):
    """300 test points: in and around the box, on data points, far outside the box, and on its corners"""
    x = _data(kind)
    rng = np.random.RandomState(len(kind))
    lo, hi = x.min(axis=0), x.max(axis=0)
    ext = np.where(hi > lo, hi - lo, 1.0)
    t = lo - 0.1 * ext + 1.2 * ext * rng.rand(300, x.shape[1])
    if kind == "lattice":
        t[::3] = np.round(t[::3])                                       # on the lattice and between its points: exact ties
    t[::5] = x[rng.choice(len(x), len(t[::5]), replace=False)]
    t[1] = lo - 10.0 * ext
    t[2] = hi + 7.0 * ext
    t[3] = lo
    t[4] = hi
    t[6] = np.where(np.arange(x.shape[1]) % 2 == 0, lo, hi)
    t[7] = 0.5 * (lo + hi) + 1000.0 * ext * (np.arange(x.shape[1]) == 0)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _brute_query(kind, m):
    tab = vecchia_local_ref.query_neighbors(_data(kind), _queries(kind), m)
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def _brute_pred(kind, m, shuffled):
    tab = vecchia_ref.brute_force_neighbors(_pred_data(kind, shuffled), m)
    tab.setflags(write=False)
    return tab


def _pred_data(kind, shuffled):
    x = _data(kind)[:1000]
    return x[np.random.RandomState(3).permutation(len(x))] if shuffled else x


def _occ(occ, n):
    return n if occ == "N" else occ


@pytest.mark.parametrize("occ", [0, 2, "N"])
@pytest.mark.parametrize("m", [1, 7, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_query_table_equals_brute_force(kind, m, occ):
    x, t = _data(kind), _queries(kind)
    tab = vecchia._device_search(x, t, None, m, 0, occupancy=_occ(occ, len(x)))
    assert tab.shape == (300, m) and tab.dtype == np.int32
    want = _brute_query(kind, m)
    bad = np.flatnonzero((tab != want).any(axis=1))
    assert not len(bad), (kind, m, occ, bad[:5], tab[bad[:2]], want[bad[:2]])
    if occ == 0:                                                        # the public function, and the same bits twice
        assert np.array_equal(vecchia_query_neighbors(x, t, m, device=0), want)


def test_padding_when_the_data_set_is_small():
    rng = np.random.RandomState(11)
    x, t = rng.rand(5, 2), rng.rand(9, 2)
    for occ in (0, 1, 2, 5):
        tab = vecchia._device_search(x, t, None, 7, 0, occupancy=occ)
        assert np.array_equal(tab, np.tile(np.array([0, 1, 2, 3, 4, -1, -1], dtype=np.int32), (9, 1)))
    assert np.array_equal(vecchia_query_neighbors(x[:1], t, 3, device=0), np.tile(np.array([0, -1, -1], dtype=np.int32), (9, 1)))
    assert np.array_equal(vecchia_query_neighbors(x[:1, 0], t[:, 0], 1, device=0), np.zeros((9, 1), dtype=np.int32))
    assert np.array_equal(vecchia_neighbors(x[:1], 2, device=0), np.full((1, 2), -1, dtype=np.int32))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("m", [7, 64])
@pytest.mark.parametrize("kind", ["3d", "lattice"])
def test_predecessor_table_equals_brute_force(kind, m, shuffled):
    """limit[i] = i: the early rows find fewer than m eligible points and walk the whole grid"""
    x = _pred_data(kind, shuffled)
    want = _brute_pred(kind, m, shuffled)
    for occ in (0, 2):
        tab = vecchia._device_search(x, x, np.arange(len(x)), m, 0, occupancy=occ)
        assert np.all(tab[0] == -1)
        assert all(np.count_nonzero(tab[i] >= 0) == i for i in range(m))
        bad = np.flatnonzero((tab != want).any(axis=1))
        assert not len(bad), (kind, m, occ, bad[:5], tab[bad[:2]], want[bad[:2]])
    assert np.array_equal(vecchia_neighbors(x, m, device=0), want)
    assert np.array_equal(vecchia_neighbors(x, m), want)                # (and the host search agrees: one table, two routes)


@pytest.mark.parametrize("m", [1, 7, 64])
@pytest.mark.parametrize("ndim", [9, 16])
def test_many_dimensions_give_a_nearest_set(ndim, m):
    rng = np.random.RandomState(ndim)
    x, t = rng.uniform(0, 1, (1200, ndim)), rng.uniform(-0.1, 1.1, (200, ndim))
    t[::5] = x[rng.choice(len(x), 40, replace=False)]
    D = ((x[None, :, :] - t[:, None, :]) ** 2).sum(axis=-1)
    for occ in (0, 2):
        tab = vecchia._device_search(x, t, None, m, 0, occupancy=occ)
        assert np.all(tab >= 0) and np.all(tab < len(x))
        assert np.all(np.diff(tab, axis=1) > 0)                         # ascending: no entry twice
        inside = np.zeros(D.shape, dtype=bool)
        np.put_along_axis(inside, tab.astype(np.int64), True, axis=1)
        worst_in = np.where(inside, D, -np.inf).max(axis=1)
        best_out = np.where(inside, np.inf, D).min(axis=1)
        assert np.all(best_out >= worst_in * (1.0 - 64 * EPS)), (ndim, m, occ)


# ------------------------------------------------------------------ the fused call and what sits on it
def _kernel3():
    return 0.8 * kernels.ExpSquaredKernel([0.4, 0.6, 0.9], ndim=3)


@functools.lru_cache(maxsize=None)
def _problem(n=777, seed=0):
    rng = np.random.RandomState(100 + seed)
    x = rng.uniform(0, 2, (n, 3))
    yerr = 0.1 + 0.05 * rng.rand(n)
    r = np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n)
    xs = rng.uniform(-0.2, 2.2, (300, 3))
    xs[::7] = x[rng.choice(n, len(xs[::7]), replace=False)]
    return x, yerr, r, xs


def _same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("order", [None, "coordinate"])
@pytest.mark.parametrize("m", [7, 64])
def test_fused_prediction_equals_the_host_search_route(m, order):
    x, yerr, r, xs = _problem()
    kernel = _kernel3()
    solver = VecchiaSolver(kernel, m=m, order=order)
    solver.compute(x, yerr)
    host = solver.predict_local(kernel, r, xs, return_var=True, search="host")
    dev = solver.predict_local(kernel, r, xs, return_var=True, search="device")
    assert _same(dev, host)
    assert _same(solver.predict_local(kernel, r, xs, return_var=True, search="device"), host)      # the kept grid
    mu, none = solver.predict_local(kernel, r, xs, search="device")
    assert none is None and np.array_equal(mu, host[0])
    s2 = VecchiaSolver(kernel, m=m, order=order, search="device", predict="local")               # its own table from the device, too
    VecchiaSolver._TABLES[:] = []
    s2.compute(x, yerr)
    assert s2.log_determinant == solver.log_determinant
    assert _same(s2.predict_local(kernel, r, xs, return_var=True), host)
    assert _same(s2.predict(kernel, r, xs, return_var=True)[:2], host)
    assert _same(s2.predict_local(kernel, r, xs, return_var=True, m=3), solver.predict_local(kernel, r, xs, return_var=True, m=3))
    with pytest.raises(ValueError):
        solver.predict_local(kernel, r, xs, search="smoke")
    nbr = vecchia_query_neighbors(x, xs, m)[:, ::-1]                    # an explicit table ignores the option
    assert _same(s2.predict_local(kernel, r, xs, return_var=True, neighbors=nbr),
                 solver.predict_local(kernel, r, xs, return_var=True, neighbors=nbr))


def test_fused_prediction_with_a_component_kernel():
    x, yerr, r, xs = _problem()
    k1, k2 = _kernel3(), 0.3 * kernels.Matern32Kernel([0.5, 0.5, 0.5], ndim=3)
    kernel = k1 + k2
    solver = VecchiaSolver(kernel, m=7)
    solver.compute(x, yerr)
    for comp in (k1, k2):
        assert _same(solver.predict_local(comp, r, xs, return_var=True, search="device"),
                     solver.predict_local(comp, r, xs, return_var=True, search="host"))


def _fused_abi(solver, r, xs, m, occupancy=0):
    mu, var = np.empty(len(xs)), np.empty(len(xs))
    tab = np.full((len(xs), m), -7, dtype=np.int32)
    N.check(N.lib.gh_vecchia_predict_local_search(solver._handle, solver._dk.handle, solver._dk.handle, N.ptr(np.ascontiguousarray(r)),
                                                  N.ptr(np.ascontiguousarray(xs)), len(xs), m, occupancy, N.ptr(mu), N.ptr(var), N.ptr(tab)))
    return mu, var, tab


def test_table_out_and_the_kept_grid():
    x, yerr, r, xs = _problem()
    kernel = _kernel3()
    solver = VecchiaSolver(kernel, m=7)
    solver.compute(x, yerr)
    host = solver.predict_local(kernel, r, xs, return_var=True)
    want = vecchia_query_neighbors(x, xs, 7)
    for occ in (0, 0, 3, 0):                                            # built, kept, built for another occupancy, built again
        mu, var, tab = _fused_abi(solver, r, xs, 7, occ)
        assert np.array_equal(tab, want) and _same((mu, var), host)
    # compute() on other points drops the grid: same size, other size, and a handle picked up from the pool by a new solver
    for n2, seed in ((777, 1), (500, 2)):
        xb, yerrb, rb, _ = _problem(n2, seed)
        solver.compute(xb, yerrb)
        got = solver.predict_local(kernel, rb, xs, return_var=True, search="device")
        fresh = VecchiaSolver(kernel, m=7)
        fresh.compute(xb, yerrb)
        assert _same(got, fresh.predict_local(kernel, rb, xs, return_var=True, search="host"))
        assert _same(got, fresh.predict_local(kernel, rb, xs, return_var=True, search="device"))
        assert np.array_equal(_fused_abi(solver, rb, xs, 7)[2], vecchia_query_neighbors(xb, xs, 7))
    del solver, fresh
    s3 = VecchiaSolver(kernel, m=7)                                     # (a parked handle, with the grid of the last points)
    s3.compute(x, yerr)
    assert _same(s3.predict_local(kernel, r, xs, return_var=True, search="device"), host)


def test_gp_with_the_device_search():
    x, yerr, r, xs = _problem()
    out = {}
    for mode in ("host", "device"):
        VecchiaSolver._TABLES[:] = []
        vecchia._TREES[:] = []
        gp = GP(_kernel3(), solver=VecchiaSolver, m=16, search=mode, predict="local")
        gp.compute(x, yerr)
        mu, var = gp.predict(r, xs, return_var=True)
        out[mode] = (gp.log_likelihood(r), mu, var)
        if mode == "device":
            assert not vecchia._TREES                                   # no host search was made
    assert out["host"][0] == out["device"][0]
    assert _same(out["host"][1:], out["device"][1:])
