"""The inducing-point solver on the host: the NumPy restatement (tests/inducing_ref.py) against LAPACK on the explicit matrix
``C`` and against central differences of itself, its block-wise gradient route against the stacked one, the bound of the device
tests against deliberately wrong gradients, ``u = x`` against the dense GP, the max-min selection against a brute-force
loop, the accuracy claim against the Vecchia restatement, the solver protocol before ``compute``, the inputs that are refused,
and the argument checks of the C ABI.  No device is touched."""
import ctypes
import json
import os
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import kernels
from george_amd import _native as N
from george_amd.solvers import InducingSolver
from george_amd.solvers.inducing import inducing_points
from george_amd.solvers.protocol import NativeSolver
from george_amd.solvers.vecchia import vecchia_neighbors

import inducing_cases
import inducing_ref
import vecchia_ref
from oracle import solver_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(name, n, seed=3):
    """(kernel, x, yerr, r): error bars 0.1 of the amplitude"""
    rng = np.random.RandomState(seed)
    if name == "m32_1d":
        kernel, x, amp = 1.7 * kernels.Matern32Kernel(0.8), np.sort(rng.uniform(0, 10, n))[:, None], np.sqrt(1.7)
    elif name == "m32_3d":
        kernel, x, amp = 1.3 * kernels.Matern32Kernel(0.6, ndim=3), rng.uniform(0, 2, (n, 3)), np.sqrt(1.3)
    else:
        kernel = 0.8 * kernels.Matern32Kernel([0.5, 0.7, 0.9], ndim=3) + 0.3 * kernels.ExpSquaredKernel(0.6, ndim=3)
        x, amp = rng.uniform(0, 2, (n, 3)), 1.0
    return kernel, x, 0.1 * amp * np.ones(n), amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("name,m", [("m32_1d", 40), ("comp_3d", 60)])
def test_restatement_against_the_explicit_matrix(name, m, method):
    """The restatement's O(N m^2) route against Cholesky, solves and a term-by-term derivative of the N x N matrix.  Observed at
    N = 300: 1e-16 .. 3e-13; asserted with three orders of margin."""
    kernel, x, yerr, r = _problem(name, 300)
    u = x[inducing_points(x, m)]
    xs = np.random.RandomState(5).uniform(0, 2, (9, x.shape[1]))
    jitter = 1e-10 * np.mean(solver_np.kernel_matrix(kernel, u, diag=True))
    g, ref, d = inducing_ref.gaps(kernel, x, yerr, u, jitter, method, r, xs)
    print(g)
    assert g["logdet"] <= 1e-12 and g["quad"] <= 1e-11
    assert abs(ref.log_likelihood() - (-0.5 * (d["quad"] + d["logdet"] + 300 * np.log(2 * np.pi)))) <= 1e-11 * abs(ref.log_likelihood())
    for key in ("Cinv", "alpha", "kgrad", "diagA", "mu", "var", "cov"):
        assert g[key] <= 1e-10, (key, g[key])
    # the model covariance is what the header says: V^T V + diag(lambda)
    V = np.dot(ref.LA, ref.H)
    assert np.allclose(d["C"], np.dot(V.T, V) + np.diag(ref.lam), rtol=0, atol=1e-10 * np.max(np.abs(d["C"])))


@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_restatement_gradient_matches_central_differences(method):
    """N = 150, m = 20: the gradient of the restatement -- kernel, white-noise and mean parameters through the assembly formula
    of ``GP._assemble_grad`` -- against central differences of its own value (the absolute jitter held fixed)."""
    kernel, x, yerr, y = _problem("comp_3d", 150)
    u = x[inducing_points(x, 20)]
    p0 = np.concatenate([[0.3, np.log(0.02)], kernel.get_parameter_vector()])          # mean | white noise | kernel

    def parts(p, want_grad):
        kernel.set_parameter_vector(p[2:])
        sigma = np.sqrt(yerr ** 2 + np.exp(p[1]))
        return inducing_ref.reference(kernel, x, sigma, u, 1e-9, method, r=y - p[0], want_grad=want_grad)

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


@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("name,n", [("m32_1d", 200), ("m32_3d", 300)])
def test_every_point_an_inducing_point_is_the_dense_gp(name, n, method):
    """u = x, jitter = 0: Q = K, the FITC correction vanishes, and both methods ARE the dense GP.  Observed: log-likelihood
    2e-15 .. 2e-14 relative, alpha / diagA 4e-13, the gradient 4e-16 of its scale; asserted with three orders of margin."""
    kernel, x, yerr, r = _problem(name, n)
    ref = inducing_ref.reference(kernel, x, yerr, x, 0.0, method, r=r, want_grad=True)
    d = vecchia_ref.dense(kernel, x, yerr, r)
    ll = -0.5 * (d["quad"] + d["logdet"] + n * np.log(2 * np.pi))
    assert abs(ref.log_likelihood() - ll) <= 1e-11 * abs(ll)
    assert inducing_ref.rel(ref.alpha, d["alpha"]) <= 1e-10 and inducing_ref.rel(ref.diagA, d["diagA"]) <= 1e-10
    assert np.max(np.abs(ref.kgrad - d["kgrad"]) / d["S"]) <= 1e-12


@pytest.mark.parametrize("method", ["dtc", "fitc"])
def test_blockwise_gradient_equals_the_stacked_one(method):
    """N = 300 (blocks of 256 + 44 points), m = 60, six parameters: the two routes add the same terms in another grouping.
    Observed: 3e-17 of ``S``; asserted at 4 eps, the least the tolerance rule takes two CPU routes to differ by."""
    kernel, x, yerr, r = _problem("comp_3d", 300)
    u = x[inducing_points(x, 60)]
    jitter = 1e-10 * np.mean(solver_np.kernel_matrix(kernel, u, diag=True))
    a = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True)
    b = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, route="blocks")
    assert inducing_ref.BLOCK < 300 and a.kgrad.shape == b.kgrad.shape == (6,)
    assert np.array_equal(a.alpha, b.alpha) and np.array_equal(a.diagA, b.diagA)
    print(np.abs(a.kgrad - b.kgrad) / a.S, np.abs(a.S - b.S) / a.S)
    assert np.all(np.abs(a.kgrad - b.kgrad) <= 4 * inducing_cases.EPS * a.S)
    # S is a sum of 300 * 60 + 60^2 + 300 non-negative terms and only a scale: any order of adding n such terms is within n eps
    assert np.all(np.abs(a.S - b.S) <= (300 * 60 + 60 * 60 + 300) * inducing_cases.EPS * a.S)
    with pytest.raises(ValueError):
        inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, route="tiles")
    with pytest.raises(ValueError):
        inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, defect="none")


def test_a_kernel_without_parameters():
    """``gaps`` and both routes on the DotProductKernel: an empty gradient, a gap of 0"""
    kernel, x, yerr, r, xs, u = inducing_cases.dot_problem()
    for method in ("dtc", "fitc"):
        jitter, ref, tol = inducing_cases.bounds("dot", kernel, x, yerr, r, xs, u, 1e-10, method)
        assert ref.kgrad.shape == ref.S.shape == (0,) and tol["kgrad"] == 4000 * inducing_cases.EPS
        b = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, route="blocks")
        assert b.kgrad.shape == (0,) and np.array_equal(b.diagA, ref.diagA)


# Where a defect changes the gradient at all: the FITC ones under FITC, the 4096-point one beyond 4096 points.
def _applies(defect, method, n):
    if defect in ("fitc_first_4096", "fitc_weight_one", "z_phi_zero") and method == "dtc":
        return False
    return defect != "fitc_first_4096" or n > inducing_ref.DIAG_POINTS


@pytest.mark.parametrize("method", ["dtc", "fitc"])
@pytest.mark.parametrize("case", [4, 64, "N4200"])
def test_the_bound_of_the_device_tests_rejects_every_defect(case, method):
    """The problems of tests/test_gpu_inducing_grad.py at P = 4 and P = 64 (N = 300, m = 65) and at N = 4200 (m = 65, 273 000
    pairs), with the bound those tests put on the gradient -- 1000 x the gap of the two CPU routes, over ``S``: every wrong
    gradient of ``inducing_ref.DEFECTS`` is further from the restatement than that, the single missing pair included.  A
    defect that cannot change the gradient of a problem (``_applies``) must leave every bit of it."""
    if case == "N4200":
        kernel, x, yerr, r, xs, u = inducing_cases.m32_case(4200, 65)
        _, jitter, ref, tol = inducing_cases.m32_bounds(4200, 65, method)
    else:
        kernel, x, yerr, r, xs, u = inducing_cases.pcase(case)
        _, jitter, ref, tol = inducing_cases.pcase_bounds(case, method)
    route = "blocks" if len(x) > inducing_cases.GAP_MAX_N else "stacked"
    for defect in inducing_ref.DEFECTS:
        bad = inducing_ref.reference(kernel, x, yerr, u, jitter, method, r=r, want_grad=True, route=route, defect=defect)
        err = float(np.max(np.abs(bad.kgrad - ref.kgrad) / ref.S))
        print("%-16s error %.3g  bound %.3g" % (defect, err, tol["kgrad"]))
        if _applies(defect, method, len(x)):
            assert err > tol["kgrad"], (defect, err, tol["kgrad"])
        else:
            assert np.array_equal(bad.kgrad, ref.kgrad), defect


# ------------------------------------------------------------------ the selection of inducing points
def _inputs(kind, n=200):
    rng = np.random.RandomState(11)
    if kind == "1d":
        return rng.uniform(0, 10, n)[:, None]
    if kind == "lattice":
        return rng.randint(0, 6, (n, 2)).astype(np.float64)                 # many exact ties and repeated points
    return rng.uniform(0, 1, (n, 3))


@pytest.mark.parametrize("m", [1, 7, 40])
@pytest.mark.parametrize("kind", ["1d", "lattice", "3d"])
def test_inducing_points_equal_brute_force(kind, m):
    x = _inputs(kind)
    idx = inducing_points(x, m)
    assert idx.dtype == np.int64 and len(idx) == m
    assert np.array_equal(idx, inducing_ref.max_min_points(x, m))


def test_inducing_points_edge_cases():
    x = np.arange(5.0)
    assert inducing_points(x, 1).tolist() == [2]                             # nearest the centroid
    assert inducing_points(x, 3).tolist() == [2, 0, 4]                       # the tie between 0 and 4 goes to the lower index
    assert sorted(inducing_points(x, 9).tolist()) == [0, 1, 2, 3, 4]         # min(m, N) points
    with pytest.raises(ValueError):
        inducing_points(x, 0)
    with pytest.raises(ValueError):
        inducing_points(np.zeros((2, 2, 2)), 1)


# ------------------------------------------------------------------ the accuracy claim
def test_more_accurate_than_vecchia_on_smooth_kernels():
    """The two ExpSquared problems of ``scripts/bench_vecchia.py --what accuracy`` (N = 2000): the restatement at m = 128 max-min
    points has a smaller log-likelihood error than the Vecchia restatement at m = 64, for both methods.  The values are those
    of ``profiles/inducing/accuracy.json``, which ``scripts/bench_inducing.py --what accuracy`` writes with the same code."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_inducing", os.path.join(ROOT, "scripts", "bench_inducing.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rows = bench.run_accuracy(cases=("1-D ExpSquared", "2-D ExpSquared"), ms=(128,))
    assert len(rows) == 2
    recorded = {(r["case"], r["m"]): r for r in json.load(open(os.path.join(ROOT, "profiles", "inducing", "accuracy.json")))}
    for row in rows:
        print(row)
        assert row["rel_diff_dtc"] < row["rel_diff_vecchia_m64"] and row["rel_diff_fitc"] < row["rel_diff_vecchia_m64"]
        assert row["rel_diff_vecchia_m64"] > 1e-2 and max(row["rel_diff_dtc"], row["rel_diff_fitc"]) < 1e-5
        rec = recorded[(row["case"], 128)]
        assert abs(rec["ll_dense"] - row["ll_dense"]) <= 1e-9 * abs(row["ll_dense"])
        assert rec["rel_diff_vecchia_m64"] > max(rec["rel_diff_dtc"], rec["rel_diff_fitc"])


# ------------------------------------------------------------------ protocol
def _kernel():
    return 1.0 * kernels.ExpSquaredKernel(1.0)


def test_before_compute_and_class_relations():
    s = InducingSolver(_kernel())
    assert not s.computed and s.log_determinant is None and s.inducing == 512 and s.method == "fitc" and s.jitter == 1e-10
    r, xs = np.zeros(3), np.zeros((2, 1))
    for call in (lambda: s.apply_inverse(r), lambda: s.apply_inverse(r, in_place=True), lambda: s.dot_solve(r), lambda: s.get_inverse(),
                 lambda: s.predict(s.kernel, r, xs, return_var=True), lambda: s.grad(r, np.ones(2, dtype=np.uint32))):
        with pytest.raises(RuntimeError, match="you must call 'compute' first"):
            call()
    with pytest.raises(NotImplementedError):
        s.apply_sqrt(r)
    assert set(InducingSolver.__mro__) <= {InducingSolver, NativeSolver, object}
    assert "InducingSolver" in george_amd.__all__ and "InducingSolver" in george_amd.solvers.__all__
    assert george_amd.InducingSolver is InducingSolver
    # capabilities, as GP routes on them
    for name in ("compute", "apply_inverse", "dot_solve", "get_inverse", "grad", "predict", "apply_sqrt"):
        assert callable(getattr(InducingSolver, name, None))
    for name in ("objective", "append", "truncate", "remove", "loo", "sample_conditional", "predict_local"):
        assert getattr(InducingSolver, name, None) is None


def test_pickle_round_trip_of_an_uncomputed_solver():
    u = np.linspace(0, 1, 5)[:, None]
    for s in (InducingSolver(_kernel(), inducing=7, method="dtc", jitter=1e-8), InducingSolver(_kernel(), inducing=u)):
        t = pickle.loads(pickle.dumps(s, -1))
        assert type(t) is InducingSolver and not t.computed and t.log_determinant is None and t._handle is None
        assert (t.method, t.jitter) == (s.method, s.jitter) and np.array_equal(t.inducing, s.inducing)
        assert t.kernel.get_parameter_vector().tolist() == s.kernel.get_parameter_vector().tolist()
        with pytest.raises(RuntimeError, match="you must call 'compute' first"):
            t.dot_solve(np.zeros(3))


# ------------------------------------------------------------------ refused inputs: ValueError, on the host
def test_refused_inputs():
    for m in (0, 8193, -3):
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), inducing=m)
    for method in ("vfe", "FITC", None, 1):
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), method=method)
    for jitter in (-1e-10, np.nan):
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), jitter=jitter)
    with pytest.raises(ValueError):
        InducingSolver(_kernel(), strip_points=-1)
    for bad in (np.zeros((0, 1)), np.zeros((2, 2, 2)), np.zeros((8193, 1))):
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), inducing=bad)
    x = np.linspace(0, 1, 6)[:, None]
    with pytest.raises(ValueError):
        InducingSolver(_kernel(), inducing=np.zeros((3, 2))).compute(x, 0.1)   # inducing inputs of another dimension
    with pytest.raises(RuntimeError):
        InducingSolver(_kernel(), inducing=3).compute(np.zeros((6, 2)), 0.1)   # data of another dimension than the kernel
    assert InducingSolver(_kernel(), inducing=np.linspace(0, 1, 4)).inducing.shape == (4, 1)


# ------------------------------------------------------------------ C ABI
def test_abi_argument_checks():
    assert ctypes.sizeof(N.gh_inducing_opts) == 4 * 4
    for name in ("gh_inducing_create", "gh_inducing_destroy", "gh_inducing_info", "gh_inducing_compute", "gh_inducing_solve",
                 "gh_inducing_dot_solve", "gh_inducing_grad", "gh_inducing_predict"):
        assert name in N.SIGNATURES and hasattr(N.lib, name)
    assert len(N.SIGNATURES["gh_inducing_compute"][1]) == 10 and len(N.SIGNATURES["gh_inducing_predict"][1]) == 8
    o, h = N.gh_inducing_opts(), N._vp()
    for method, strip in ((2, 0), (-1, 0), (1, -128)):
        o.method, o.strip_points = method, strip
        assert N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)) == N.GH_ERR_BAD_ARG
        with pytest.raises(ValueError):
            N.check(N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)))
    assert N.lib.gh_inducing_create(None, ctypes.byref(h)) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_info(None) == 0
    N.lib.gh_inducing_destroy(None)
    buf, out = np.zeros(4), ctypes.c_double(0.0)
    assert N.lib.gh_inducing_compute(None, None, N.ptr(buf), 4, 1, N.ptr(buf), N.ptr(buf), 1, 0.0, ctypes.byref(out)) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_solve(None, N.ptr(buf), 1, N.ptr(buf)) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_dot_solve(None, N.ptr(buf), ctypes.byref(out)) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_grad(None, None, None, N.ptr(buf), N.ptr(buf), None, None) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_predict(None, None, N.ptr(buf), N.ptr(buf), 1, N.ptr(buf), None, None) == N.GH_ERR_BAD_ARG
    if george_amd.device_count() == 0:
        o.method, o.strip_points = 1, 0
        with pytest.raises(RuntimeError):
            N.check(N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)))
        with pytest.raises(RuntimeError):
            InducingSolver(_kernel(), inducing=3).compute(np.linspace(0, 1, 6)[:, None], 0.1)
