"""``InducingSolver``'s variational bound and its gradient with respect to the inducing inputs, without a device: the NumPy
restatement (tests/inducing_u_ref.py) against central differences and against the explicit N x N matrix, the two properties of
the bound, the bound of the device tests against every wrong result of ``inducing_u_ref.DEFECTS``, refused inputs, pickling and
the host checks of the C ABI."""
import ctypes
import pickle

import numpy as np
import pytest

import george_amd
from george_amd import GP, BasicSolver, kernels
from george_amd import _native as N
from george_amd.solvers import InducingSolver
from george_amd.solvers.inducing import inducing_points

import inducing_cases as IC
import inducing_u_cases as UC
import inducing_u_ref as UR
import vecchia_ref
from oracle import solver_np
from test_solver_protocol_host import OPTIONAL

OBJECTIVE = pytest.mark.parametrize("objective", UR.OBJECTIVES)


def _mixed_problem(n=40, m=6):
    """a kernel with a stationary and a dot-product part, whose diagonal depends on the input; u are no data points"""
    kernel = 1.3 * kernels.Matern32Kernel(0.6, ndim=2) + 0.4 * kernels.DotProductKernel(ndim=2)
    rng = np.random.RandomState(11)
    x = rng.uniform(-1, 1, (n, 2))
    return kernel, x, 0.1 + 0.05 * rng.rand(n), np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n), rng.uniform(-1, 1, (m, 2))


# ------------------------------------------------------------------ the restatement
@OBJECTIVE
def test_both_routes_match_central_differences(objective):
    """N = 40, m = 6: the gradients of both routes in the kernel parameters, in ``s_i = yerr_i^2`` (``1/2 diagA_i``) and in every
    coordinate of ``u`` against central differences of ``F`` (step 1e-5, bound 1e-6 of the scale, the absolute jitter held)."""
    kernel, x, yerr, r, u = _mixed_problem()
    p0, jitter = kernel.get_parameter_vector(), 1e-9

    def F(p=p0, s=yerr ** 2, uu=u):
        kernel.set_parameter_vector(p)
        return UR.model(kernel, x, np.sqrt(s), uu, jitter, objective, r).F

    def central(arg, a0, index):
        h = 1e-5 * max(1.0, abs(a0[index]))
        up, dn = a0.copy(), a0.copy()
        up[index] += h
        dn[index] -= h
        return (F(**{arg: up}) - F(**{arg: dn})) / (2 * h)

    try:
        for route in (UR.model, UR.dense):
            got = route(kernel, x, yerr, u, jitter, objective, r)
            assert got.kgrad.shape == p0.shape and got.ugrad.shape == u.shape
            for a in range(len(p0)):
                fd = central("p", p0, a)
                assert abs(fd - got.kgrad[a]) <= 1e-6 * max(1.0, abs(fd)), (route.__name__, "parameter", a, fd, got.kgrad[a])
            for i in (0, 17, 39):
                fd = central("s", yerr ** 2, i)
                assert abs(fd - 0.5 * got.diagA[i]) <= 1e-6 * max(1.0, abs(fd)), (route.__name__, "s", i, fd, 0.5 * got.diagA[i])
            for j in np.ndindex(*u.shape):
                fd = central("uu", u, j)
                assert abs(fd - got.ugrad[j]) <= 1e-6 * max(1.0, abs(fd)), (route.__name__, "u", j, fd, got.ugrad[j])
    finally:
        kernel.set_parameter_vector(p0)


@OBJECTIVE
@pytest.mark.parametrize("name", ["m32_1d_m129", "comp_3d_m65", "dot"])
def test_restatement_against_the_explicit_matrix(name, objective):
    """The two routes on problems of the device tests.  Observed at N = 777: 1e-18 .. 2e-12; asserted with three orders of margin."""
    kernel, x, yerr, r, u, _ = UC.case(name)
    jitter, ref, _ = UC.bounds(name, objective)
    g = UR.gaps(kernel, x, yerr, u, jitter, objective, r)[0]
    print(g)
    assert max(g.values()) <= 1e-9
    assert ref.tau >= 0.0 and (ref.tau > 0.0) == (objective == "vfe")
    assert ref.F == ref.ref.log_likelihood() - 0.5 * ref.tau


def test_the_bound_is_below_the_dense_likelihood_and_grows_with_nested_inducing_sets():
    """m32_3d, N = 300: ``F`` at the nested max-min sets m = 10 / 20 / 40 does not decrease (up to the tolerance of the
    log-likelihood, 1000 x 4 eps of its size) and stays below the dense log-likelihood; DTC's own value is no bound."""
    kernel, x, yerr, r, _ = IC._problem("m32_3d", 300)
    d = vecchia_ref.dense(kernel, x, yerr, r)
    ll = -0.5 * (d["quad"] + d["logdet"] + 300 * np.log(2 * np.pi))
    idx = inducing_points(x, 40)
    F = []
    for m in (10, 20, 40):
        u = x[idx[:m]]
        jitter = 1e-10 * np.mean(solver_np.kernel_matrix(kernel, u, diag=True))
        F.append(UR.model(kernel, x, yerr, u, jitter, "vfe", r).F)
    slack = 4000 * IC.EPS * abs(ll)
    print(F, ll)
    assert F[0] <= F[1] + slack and F[1] <= F[2] + slack and F[2] <= ll + slack
    assert F[2] - F[0] > 1.0                     # (the sets differ: the bound moves by far more than the slack)


# ------------------------------------------------------------------ the bound of the device tests
def _applies(defect, objective):
    if defect == "omega_dropped":
        return objective != "dtc"
    return defect != "tau_diaga_dropped" or objective == "vfe"


@OBJECTIVE
@pytest.mark.parametrize("name", UC.MATERN)
def test_the_bound_of_the_device_tests_rejects_every_defect(name, objective):
    """The Matern problems of the device tests (N = 777) with the bounds those tests use -- 1000 x the gap of the two CPU
    routes, ``ugrad`` over ``S_u``: every wrong result of ``inducing_u_ref.DEFECTS`` is further from the restatement than that.
    A defect that cannot change a result (``_applies``) leaves every bit of it."""
    kernel, x, yerr, r, u, _ = UC.case(name)
    jitter, ref, tol = UC.bounds(name, objective)
    for defect in UR.DEFECTS:
        bad = UR.model(kernel, x, yerr, u, jitter, objective, r, defect=defect)
        if defect == "tau_diaga_dropped":
            key, err = "diagA", UR.rel(bad.diagA, ref.diagA)
            same = np.array_equal(bad.diagA, ref.diagA) and np.array_equal(bad.ugrad, ref.ugrad)
        else:
            key, err = "ugrad", UR.over(bad.ugrad - ref.ugrad, ref.S_u)
            same = np.array_equal(bad.ugrad, ref.ugrad) and np.array_equal(bad.kgrad, ref.kgrad)
        print("%-20s %s error %.3g  bound %.3g" % (defect, key, err, tol[key]))
        if _applies(defect, objective):
            assert err > tol[key], (defect, err, tol[key])
        else:
            assert same, defect
    with pytest.raises(ValueError):
        UR.model(kernel, x, yerr, u, jitter, objective, r, defect="none")
    with pytest.raises(ValueError):
        UR.model(kernel, x, yerr, u, jitter, "vfe2", r)


def test_every_case_of_the_device_tests_keeps_the_gap_cap():
    """``bounds`` asserts ``GAP_CAP`` for every problem and objective the device tests run; one data point under FITC is the
    one degenerate pair (``C = k(x, x) + s`` whatever ``u``: ``Z`` cancels to rounding, and ``S_u`` with it)."""
    for name in list(UC.CASES) + ["dot"]:
        for objective in UR.OBJECTIVES:
            if (name, objective) == ("n1_m3", "fitc"):
                kernel, x, yerr, r, u, _ = UC.case(name)
                ref = UR.model(kernel, x, yerr, u, 1e-10, objective, r)
                assert np.all(np.abs(ref.ugrad) <= 4000 * IC.EPS * ref.S_u_terms) and np.all(ref.S_u_terms > 1e3 * ref.S_u)
            else:
                UC.bounds(name, objective)
    ref = UC.bounds("axes02_3d_m65", "vfe")[1]
    assert np.all(ref.ugrad[:, 1] == 0.0) and np.all(ref.S_u[:, 1] == 0.0) and np.all(ref.S_u[:, [0, 2]] > 0.0)


# ------------------------------------------------------------------ the Python surface, without a device
def _kernel():
    return 1.3 * kernels.Matern32Kernel(0.6, ndim=2)


def test_refused_inputs():
    for method in ("fitc", "vfe"):
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), method=method, variational=True)
    s = InducingSolver(_kernel(), inducing=4, method="dtc", variational=True)
    assert s.variational is True and s.trace_term == 0.0 and s._options_key() == (0, 0, 0, 1)
    assert InducingSolver(_kernel(), inducing=4, method="dtc")._options_key() == (0, 0, 0)
    assert InducingSolver(_kernel(), method="dtc", variational=1).variational is True
    with pytest.raises(RuntimeError):
        s.grad_inducing(np.zeros(3))
    assert {name for name in OPTIONAL if callable(getattr(InducingSolver, name, None))} == {"predict", "grad"}
    assert "grad_inducing" not in OPTIONAL and callable(InducingSolver.grad_inducing)


def test_gp_refuses_solvers_without_inducing_inputs():
    gp = GP(_kernel(), solver=BasicSolver)
    y = np.zeros(5)
    for call in (lambda: gp.inducing_inputs, lambda: gp.grad_log_likelihood_inducing(y), lambda: gp.nll_and_grad_inducing(np.zeros(9), y)):
        with pytest.raises(NotImplementedError, match="BasicSolver"):
            call()
    gp = GP(_kernel(), solver=InducingSolver, inducing=3, method="dtc", variational=True)
    with pytest.raises(RuntimeError):
        gp.nll_and_grad_inducing(np.zeros(len(gp) + 6), y)                 # not computed yet: no data recorded
    gp._x, gp._yerr2 = np.zeros((5, 2)), np.zeros(5)
    for bad in (np.zeros(len(gp)), np.zeros(len(gp) + 3), np.zeros((len(gp) + 4, 1))):
        with pytest.raises(ValueError):
            gp.nll_and_grad_inducing(bad, y)


def test_pickle_round_trip_keeps_the_option():
    s = pickle.loads(pickle.dumps(InducingSolver(_kernel(), inducing=np.zeros((3, 2)), method="dtc", variational=True, strip_points=128)))
    assert s.variational is True and s.method == "dtc" and s._options_key() == (0, 0, 128, 1) and not s.computed
    assert s._native_opts().variational == 1 and s._native_opts().strip_points == 128
    t = pickle.loads(pickle.dumps(InducingSolver(_kernel(), inducing=3)))
    assert t.variational is False and t._native_opts().variational == 0 and t._native_opts().method == 1


# ------------------------------------------------------------------ C ABI
def test_abi_argument_checks():
    assert ctypes.sizeof(N.gh_inducing_opts) == 4 * 4
    assert [f[0] for f in N.gh_inducing_opts._fields_] == ["device", "method", "strip_points", "variational"]
    for name, nargs in (("gh_inducing_trace_term", 2), ("gh_inducing_grad_u", 8)):
        assert name in N.SIGNATURES and hasattr(N.lib, name) and len(N.SIGNATURES[name][1]) == nargs
    o, h = N.gh_inducing_opts(), N._vp()
    for method, variational in ((0, 2), (0, -1), (1, 1), (2, 0), (2, 1)):
        o.method, o.variational = method, variational
        assert N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)) == N.GH_ERR_BAD_ARG
        with pytest.raises(ValueError):
            N.check(N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)))
    buf, out = np.zeros(4), ctypes.c_double(7.0)
    assert N.lib.gh_inducing_trace_term(None, ctypes.byref(out)) == N.GH_ERR_BAD_ARG and out.value == 7.0
    assert N.lib.gh_inducing_grad_u(None, None, None, N.ptr(buf), None, None, None, N.ptr(buf)) == N.GH_ERR_BAD_ARG
    if george_amd.device_count() == 0:
        o.method, o.variational = 0, 1
        with pytest.raises(RuntimeError):
            N.check(N.lib.gh_inducing_create(ctypes.byref(o), ctypes.byref(h)))
