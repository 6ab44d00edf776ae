"""The Vecchia solver on the host: the NumPy restatement (tests/vecchia_ref.py) against dense LAPACK and against finite
differences of itself, the default neighbour table against a brute-force search, the solver protocol before ``compute``,
the inputs that are refused, and the argument checks of the C ABI.  No device is touched."""
import ctypes
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import kernels
from george_amd import _native as N
from george_amd.solvers import VecchiaSolver
from george_amd.solvers.protocol import NativeSolver
from george_amd.solvers.vecchia import vecchia_neighbors

import vecchia_ref


def _problem(name, n, seed=3):
    """(kernel, x, yerr, r): error bars 0.1 of the amplitude"""
    rng = np.random.RandomState(seed)
    if name == "m32_1d":
        kernel, x, amp = 1.7 * kernels.Matern32Kernel(0.8), np.sort(rng.uniform(0, 10, n))[:, None], np.sqrt(1.7)
    else:
        kernel, amp = 0.9 * kernels.ExpSquaredKernel([0.3, 0.5], ndim=2), np.sqrt(0.9)
        x = rng.uniform(0, 2, (n, 2))
        x = x[np.argsort(x[:, 0], kind="stable")]
    return kernel, x, 0.1 * amp * np.ones(n), amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["m32_1d", "expsq_2d"])
def test_restatement_is_dense_with_every_predecessor(name):
    """m = N - 1: the product of conditionals IS the joint density.  Observed at N = 60: log-determinant 1e-15 relative, Q
    against K^-1 2e-14 of its largest entry; asserted with three orders of margin."""
    kernel, x, yerr, r = _problem(name, 60)
    xs = np.random.RandomState(5).uniform(0, 2, (7, x.shape[1]))
    g, ref, d = vecchia_ref.gaps(kernel, x, yerr, r, xs)
    print(g)
    assert g["logdet"] <= 1e-12 and g["quad"] <= 1e-11
    assert abs(ref.log_likelihood() - (-0.5 * (d["quad"] + d["logdet"] + 60 * np.log(2 * np.pi)))) <= 1e-11 * abs(ref.log_likelihood())
    for key in ("Kinv", "alpha", "kgrad", "diagA", "mu", "var", "cov"):
        assert g[key] <= 1e-10, (key, g[key])


def test_restatement_gradient_matches_finite_differences():
    """m = 12: the gradient of the restatement -- kernel, white-noise and mean parameters through the assembly formula of
    ``GP._assemble_grad`` -- against central differences of its own value."""
    kernel, x, yerr, y = _problem("expsq_2d", 90)
    nbr = vecchia_ref.brute_force_neighbors(x, 12)
    p0 = np.concatenate([[0.3, np.log(0.02)], kernel.get_parameter_vector()])          # mean | white noise | kernel

    def parts(p, want_grad):
        kernel.set_parameter_vector(p[2:])
        sigma = np.sqrt(yerr ** 2 + np.exp(p[1]))
        return vecchia_ref.reference(kernel, x, sigma, nbr, r=y - p[0], want_grad=want_grad)

    ref = parts(p0, True)
    grad = np.concatenate([[np.sum(ref.alpha)], [0.5 * np.sum(np.exp(p0[1]) * ref.diagA)], ref.kgrad])
    for a in range(len(p0)):
        h = 1e-5 * max(1.0, abs(p0[a]))
        up, dn = p0.copy(), p0.copy()
        up[a] += h
        dn[a] -= h
        fd = (parts(up, False).log_likelihood() - parts(dn, False).log_likelihood()) / (2 * h)
        assert abs(fd - grad[a]) <= 1e-6 * max(1.0, abs(grad[a])), (a, fd, grad[a])
    kernel.set_parameter_vector(p0[2:])


# ------------------------------------------------------------------ neighbours
def _inputs(kind, n=500):
    rng = np.random.RandomState(11)
    if kind == "1d_sorted":
        return np.sort(rng.uniform(0, 10, n))[:, None]
    if kind == "1d_unsorted":
        return rng.uniform(0, 10, n)[:, None]
    if kind == "1d_duplicates":
        return np.sort(rng.randint(0, 120, n).astype(np.float64))[:, None]
    if kind == "2d_duplicates":
        return rng.randint(0, 12, (n, 2)).astype(np.float64)            # a lattice: many exact ties and repeated points
    return rng.uniform(0, 1, (n, int(kind[0])))


@pytest.mark.parametrize("m", [1, 7, 64])
@pytest.mark.parametrize("kind", ["1d_sorted", "1d_unsorted", "1d_duplicates", "2d", "2d_duplicates", "3d"])
def test_neighbors_equal_brute_force(kind, m):
    x = _inputs(kind)
    tab = vecchia_neighbors(x, m)
    assert tab.shape == (500, m) and tab.dtype == np.int32
    assert np.array_equal(tab, vecchia_ref.brute_force_neighbors(x, m))


def test_neighbors_of_sorted_1d_are_the_previous_points():
    tab = vecchia_neighbors(np.arange(10.0), 3)
    assert tab[0].tolist() == [-1, -1, -1] and tab[2].tolist() == [0, 1, -1] and tab[9].tolist() == [6, 7, 8]
    assert np.array_equal(vecchia_neighbors(np.arange(10.0)[:, None], 3), tab)


# ------------------------------------------------------------------ protocol
def _kernel():
    return 1.0 * kernels.ExpSquaredKernel(1.0)


def test_before_compute_and_class_relations():
    s = VecchiaSolver(_kernel())
    assert not s.computed and s.log_determinant is None and s.m == 32
    r, xs = np.zeros(3), np.zeros((2, 1))
    for call in (lambda: s.apply_inverse(r), lambda: s.apply_inverse(r, in_place=True), lambda: s.dot_solve(r), lambda: s.get_inverse(),
                 lambda: s.predict(s.kernel, r, xs, return_var=True), lambda: s.grad(r, np.ones(2, dtype=np.uint32))):
        with pytest.raises(RuntimeError, match="you must call 'compute' first"):
            call()
    with pytest.raises(NotImplementedError):
        s.apply_sqrt(r)
    assert set(VecchiaSolver.__mro__) <= {VecchiaSolver, NativeSolver, object}
    assert "VecchiaSolver" in george_amd.__all__ and "VecchiaSolver" in george_amd.solvers.__all__
    assert george_amd.VecchiaSolver is VecchiaSolver


def test_pickle_round_trip_of_an_uncomputed_solver():
    s = VecchiaSolver(_kernel(), m=7, order="coordinate")
    t = pickle.loads(pickle.dumps(s, -1))
    assert type(t) is VecchiaSolver and not t.computed and t.log_determinant is None and t._handle is None
    assert (t.m, t.order) == (7, "coordinate")
    assert t.kernel.get_parameter_vector().tolist() == s.kernel.get_parameter_vector().tolist()
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        t.dot_solve(np.zeros(3))


# ------------------------------------------------------------------ refused inputs: ValueError, on the host
def test_refused_inputs():
    for m in (0, 65, -3):
        with pytest.raises(ValueError):
            VecchiaSolver(_kernel(), m=m)
    with pytest.raises(ValueError):
        VecchiaSolver(_kernel(), order="maxmin")
    x = np.linspace(0, 1, 6)[:, None]
    good = vecchia_neighbors(x, 2)
    cases = {"an entry >= i": (3, 0, 3), "a later point": (2, 1, 5), "below -1": (4, 0, -2)}
    for why, (i, s, v) in cases.items():
        bad = good.copy()
        bad[i, s] = v
        with pytest.raises(ValueError):
            VecchiaSolver(_kernel(), m=2, neighbors=bad).compute(x, 0.1)
    dup = good.copy()
    dup[4] = [1, 1]
    with pytest.raises(ValueError, match="twice"):
        VecchiaSolver(_kernel(), m=2, neighbors=dup).compute(x, 0.1)
    for shape_bad in (good[:5], good[:, :1], np.full((6, 3), -1), good.astype(np.float64)):
        with pytest.raises(ValueError):
            VecchiaSolver(_kernel(), m=2, neighbors=shape_bad).compute(x, 0.1)
    for order in ([0, 1, 2, 3, 4, 4], [0, 1, 2], np.arange(6) + 1, np.arange(6.0)):
        with pytest.raises(ValueError, match="permutation"):
            VecchiaSolver(_kernel(), m=2, order=order).compute(x, 0.1)


# ------------------------------------------------------------------ C ABI
def test_abi_argument_checks():
    assert ctypes.sizeof(N.gh_vecchia_opts) == 4 * 4
    for name in ("gh_vecchia_create", "gh_vecchia_destroy", "gh_vecchia_compute", "gh_vecchia_info", "gh_vecchia_solve",
                 "gh_vecchia_dot_solve", "gh_vecchia_grad", "gh_vecchia_predict"):
        assert name in N.SIGNATURES and hasattr(N.lib, name)
    o, h = N.gh_vecchia_opts(), N._vp()
    for m in (0, 65, -1):
        o.m = m
        assert N.lib.gh_vecchia_create(ctypes.byref(o), ctypes.byref(h)) == N.GH_ERR_BAD_ARG
        with pytest.raises(ValueError):
            N.check(N.lib.gh_vecchia_create(ctypes.byref(o), ctypes.byref(h)))
    assert N.lib.gh_vecchia_info(None) == 0
    if george_amd.device_count() == 0:
        o.m = 32
        with pytest.raises(RuntimeError):
            N.check(N.lib.gh_vecchia_create(ctypes.byref(o), ctypes.byref(h)))
        with pytest.raises(RuntimeError):
            VecchiaSolver(_kernel()).compute(np.linspace(0, 1, 6)[:, None], 0.1)
