"""Local (nearest-neighbour) prediction of the Vecchia solver on the host: the query search against a brute-force search, the
NumPy restatement (tests/vecchia_local_ref.py) against dense LAPACK, what the local variance guarantees where the variance
through ``Q`` fails, the inputs that are refused, and the ABI entry.  No device is touched.

Observed on the CPU: restatement against dense at N = 60 with every point in every set, mu 1.3e-14 / 1.3e-14 and var 3.9e-15 /
5.5e-15 (Matern-3/2 1-D / ExpSquared 2-D), relative to the largest entry.  Property test (1-D ExpSquared, N = 2000, m = 16): the
variance through ``Q`` has its minimum at -0.399, the local one at 7.1e-4; the local variance over the dense one lies in
1.02 .. 2.82; the smallest local - dense difference is 4.5e-5 against an allowance of 1.5e-9.
"""
import ctypes
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import GP, kernels
from george_amd import _native as N
from george_amd.solvers import VecchiaSolver
from george_amd.solvers import vecchia
from george_amd.solvers.vecchia import vecchia_neighbors, vecchia_query_neighbors

from oracle import solver_np

import vecchia_local_ref
import vecchia_ref

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------ the query search
def _inputs(kind, n=500, nt=200):
    """(x, t): a fifth of the test points coincide with data points"""
    rng = np.random.RandomState(17)
    if kind == "1d_sorted":
        x = np.sort(rng.uniform(0, 10, n))[:, None]
    elif kind == "1d_unsorted":
        x = rng.uniform(0, 10, n)[:, None]
    elif kind == "1d_duplicates":
        x = np.sort(rng.randint(0, 120, n).astype(np.float64))[:, None]
    elif kind == "2d_lattice":
        x = rng.randint(0, 12, (n, 2)).astype(np.float64)               # exact ties and repeated points
    else:
        x = rng.uniform(0, 1, (n, int(kind[0])))
    lo, hi = x.min(axis=0), x.max(axis=0)
    t = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * rng.rand(nt, x.shape[1])   # some outside the data's box
    if kind in ("1d_duplicates", "2d_lattice"):
        t[::3] = np.round(t[::3])                                       # on the lattice, between its points: exact ties
    t[::5] = x[rng.choice(n, len(t[::5]), replace=False)]
    return x, t


@pytest.mark.parametrize("m", [1, 7, 64])
@pytest.mark.parametrize("kind", ["1d_sorted", "1d_unsorted", "1d_duplicates", "2d", "2d_lattice", "3d"])
def test_query_neighbors_equal_brute_force(kind, m):
    x, t = _inputs(kind)
    tab = vecchia_query_neighbors(x, t, m)
    assert tab.shape == (200, m) and tab.dtype == np.int32
    assert np.array_equal(tab, vecchia_local_ref.query_neighbors(x, t, m))
    assert np.array_equal(vecchia_query_neighbors(x, t, m), tab)       # (the kept tree)


@pytest.mark.parametrize("kind", ["1d_sorted", "1d_unsorted", "2d"])
def test_query_neighbors_pad_when_the_data_set_is_small(kind):
    x, t = _inputs(kind, n=5, nt=9)
    tab = vecchia_query_neighbors(x, t, 7)
    assert np.array_equal(tab, np.tile(np.array([0, 1, 2, 3, 4, -1, -1], dtype=np.int32), (9, 1)))
    assert np.array_equal(tab, vecchia_local_ref.query_neighbors(x, t, 7))
    assert vecchia_query_neighbors(x, t[:0], 7).shape == (0, 7)
    assert vecchia_query_neighbors(x[:, 0], t[:, 0], 3).shape == (9, 3) if x.shape[1] == 1 else True
    with pytest.raises(ValueError):
        vecchia_query_neighbors(x, t, 0)
    with pytest.raises(ValueError):
        vecchia_query_neighbors(x, np.zeros((3, x.shape[1] + 1)), 2)


def test_the_tree_is_built_once_per_data_set():
    x, t = _inputs("3d")
    del vecchia._TREES[:]
    vecchia_query_neighbors(x, t, 4)
    assert len(vecchia._TREES) == 1
    tree = vecchia._TREES[0][1]
    vecchia_query_neighbors(x.copy(), t[:10], 9)
    assert len(vecchia._TREES) == 1 and vecchia._TREES[0][1] is tree
    for shift in (1.0, 2.0, 3.0):
        vecchia_query_neighbors(x + shift, t, 4)
    assert len(vecchia._TREES) == vecchia._TREES_MAX


# ------------------------------------------------------------------ the restatement
def _problem(name, n, seed=3):
    rng = np.random.RandomState(seed)
    if name == "m32_1d":
        kernel, x, amp = 1.7 * kernels.Matern32Kernel(0.8), np.sort(rng.uniform(0, 10, n))[:, None], np.sqrt(1.7)
    else:
        kernel, amp = 0.9 * kernels.ExpSquaredKernel([0.3, 0.5], ndim=2), np.sqrt(0.9)
        x = rng.uniform(0, 2, (n, 2))
        x = x[np.argsort(x[:, 0], kind="stable")]
    return kernel, x, 0.1 * amp * np.ones(n), amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))


@pytest.mark.parametrize("name", ["m32_1d", "expsq_2d"])
def test_restatement_is_dense_with_every_point_in_every_set(name):
    """N = 60 <= 64.  Both routes solve the same 60 x 60 system in float64: with error bars 0.1 of the amplitude its condition
    number is at most 60 / 0.01, so they agree to ~ eps * 6e3 = 1e-12; asserted at 1e-10, the bound of
    tests/test_vecchia_host.py for the same comparison of the likelihood restatement."""
    kernel, x, yerr, r = _problem(name, 60)
    xs = np.random.RandomState(5).uniform(-0.2, 2.2, (25, x.shape[1]))
    xs[3] = x[7]
    g, (mu, var), d = vecchia_local_ref.gaps(kernel, x, yerr, r, xs)
    print(name, g)
    assert g["mu"] <= 1e-10 and g["var"] <= 1e-10
    # any order, padding anywhere: the same answers
    tab = np.full((25, 64), -1, dtype=np.int32)
    rng = np.random.RandomState(6)
    for c in range(25):
        tab[c, np.sort(rng.choice(64, 60, replace=False))] = rng.permutation(60)
    mu2, var2 = vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs, tab)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    # an empty row: the prior
    tab[4] = -1
    mu3, var3 = vecchia_local_ref.predict(kernel, kernel, x, yerr, r, xs, tab)
    assert mu3[4] == 0.0 and var3[4] == solver_np.kernel_matrix(kernel, xs[4:5], diag=True)[0]


def test_local_variance_is_a_variance_where_the_global_one_is_not():
    """1-D ExpSquared, 20 points per length scale, error bars 0.1, m = 16: too few neighbours for this kernel.  The variance through
    ``Q`` goes negative; the local one is the variance of a conditional distribution given FEWER observations than the dense one:
    positive, at most the prior variance, at least the dense variance.

    Allowance for the last comparison: the dense variance comes from a LAPACK solve with K = k(x, x) + 0.01 I, whose error is
    ~ eps * kappa(K) * k**; kappa <= (largest row sum of |K|) / 0.01 (Gershgorin above, the noise floor below).  1000 times that."""
    n, m = 2000, 16
    rng = np.random.RandomState(2000)
    x = np.sort(rng.uniform(0, 100, n))[:, None]
    kernel = 1.0 * kernels.ExpSquaredKernel(1.0)
    y = np.sin(3.0 * x[:, 0]) + 0.1 * rng.randn(n)
    xs = rng.uniform(0, 100, (300, 1))
    glob = vecchia_ref.reference(kernel, x, 0.1, vecchia_neighbors(x, m), r=y)
    var_global = glob.predict(kernel, xs)[1]
    print("variance through Q: min %.3g" % var_global.min())
    assert var_global.min() < -0.1                       # (observed: -0.42) not vacuous
    d = vecchia_ref.dense(kernel, x, 0.1, y, xs)
    mu, var = vecchia_local_ref.predict(kernel, kernel, x, 0.1, y, xs, vecchia_query_neighbors(x, xs, m))
    kss = solver_np.kernel_matrix(kernel, xs, diag=True)
    K = solver_np.kernel_matrix(kernel, x)
    allow = 1000.0 * EPS * (np.abs(K).sum(axis=1).max() + 0.01) / 0.01 * kss.max()
    print("local variance: min %.3g, over dense %.3g .. %.3g, min(local - dense) %.3g, allowance %.3g"
          % (var.min(), (var / d["var"]).min(), (var / d["var"]).max(), (var - d["var"]).min(), allow))
    assert allow < 1e-8
    assert np.all(var > 0.0) and np.all(var <= kss)
    assert np.all(var >= d["var"] - allow)
    assert np.all(np.isfinite(mu))


# ------------------------------------------------------------------ refused inputs, protocol
def _kernel():
    return 1.0 * kernels.ExpSquaredKernel(1.0)


def test_refused_inputs():
    for bad in ("nearest", "", None, 1):
        with pytest.raises(ValueError, match="'global' or 'local'"):
            VecchiaSolver(_kernel(), predict=bad)
    s = VecchiaSolver(_kernel(), m=8, predict="local")
    assert s.predict_mode == "local" and VecchiaSolver(_kernel()).predict_mode == "global"
    assert s.failed_test_point is None
    r, xs = np.zeros(3), np.zeros((2, 1))
    for m in (0, 65, -1):
        with pytest.raises(ValueError, match="1 <= m <= 64"):
            s.predict_local(s.kernel, r, xs, m=m)
    with pytest.raises(ValueError, match="conditionally independent"):
        s.predict(s.kernel, r, xs, return_cov=True)
    for call in (lambda: s.predict_local(s.kernel, r, xs), lambda: s.predict_local(s.kernel, r, xs, return_var=True, m=3),
                 lambda: s.predict(s.kernel, r, xs), lambda: s.predict(s.kernel, r, xs, return_var=True),
                 lambda: VecchiaSolver(_kernel()).predict_local(s.kernel, r, xs, neighbors=np.zeros((2, 32), dtype=int))):
        with pytest.raises(RuntimeError, match="you must call 'compute' first"):
            call()
    # GP hands the option through, and asks for a covariance by default
    gp = GP(_kernel(), solver=VecchiaSolver, m=8, predict="local")
    assert gp.solver_kwargs == dict(m=8, predict="local")
    with pytest.raises(ValueError):
        GP(_kernel(), solver=VecchiaSolver, predict="both").compute(np.arange(4.0), 0.1)


def test_query_table_checks():
    """what ``predict_local(neighbors=...)`` runs on the host before the native call"""
    good = np.array([[0, 3, -1], [-1, 5, 2], [-1, -1, -1], [4, 1, 0]])
    out = vecchia._check_query_neighbors(good, 4, 3, 6)
    assert out.dtype == np.int32 and out.flags.c_contiguous and np.array_equal(out, good)
    assert vecchia._check_query_neighbors(np.array([[0, 3, 1]], dtype=np.uint8), 1, 3, 6).dtype == np.int32
    for i, s, v in ((0, 0, 6), (1, 0, -2), (3, 2, 100)):
        bad = good.copy()
        bad[i, s] = v
        with pytest.raises(ValueError, match="data points"):
            vecchia._check_query_neighbors(bad, 4, 3, 6)
    dup = good.copy()
    dup[3] = [4, 1, 4]
    with pytest.raises(ValueError, match="twice"):
        vecchia._check_query_neighbors(dup, 4, 3, 6)
    for shape_bad in (good[:3], good[:, :2], good.astype(np.float64), good.ravel()):
        with pytest.raises(ValueError, match="integer table of shape"):
            vecchia._check_query_neighbors(shape_bad, 4, 3, 6)


def test_pickling_keeps_the_option():
    s = VecchiaSolver(_kernel(), m=7, order="coordinate", predict="local")
    t = pickle.loads(pickle.dumps(s, -1))
    assert type(t) is VecchiaSolver and not t.computed and t._handle is None and t._xo is None
    assert (t.m, t.order, t.predict_mode) == (7, "coordinate", "local")
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        t.predict_local(t.kernel, np.zeros(3), np.zeros((2, 1)))
    gp = pickle.loads(pickle.dumps(GP(_kernel(), solver=VecchiaSolver, predict="local"), -1))
    assert gp.solver_kwargs == dict(predict="local")


# ------------------------------------------------------------------ C ABI
def test_abi_entry():
    assert "gh_vecchia_predict_local" in N.SIGNATURES and hasattr(N.lib, "gh_vecchia_predict_local")
    assert len(N.SIGNATURES["gh_vecchia_predict_local"][1]) == 10
    assert "vecchia_query_neighbors" in vecchia.__all__ and "vecchia_neighbors" in vecchia.__all__
    assert ctypes.sizeof(N.gh_vecchia_opts) == 4 * 4
    # a null handle is an argument error, not a fault
    buf = np.zeros(4)
    tab = np.zeros((1, 1), dtype=np.int32)
    assert N.lib.gh_vecchia_predict_local(None, None, None, N.ptr(buf), N.ptr(buf), 1, N.ptr(tab), 1, N.ptr(buf), None) == N.GH_ERR_BAD_ARG
    assert george_amd.VecchiaSolver is VecchiaSolver
