"""``InducingSolver.grad_inducing`` -- the gradient of DTC, FITC and the variational bound with respect to the inducing inputs
(``gh_inducing_grad_u``: the weighted input-gradient reduction ``gh_launch_wxgrad`` of george_amd/csrc/gh_predgrad.hip on the
strips of ``Z^T`` and on ``-(W + W^T)``) -- against the NumPy restatement (tests/inducing_u_ref.py), and through ``GP``.

Tolerances: the rule of tests/inducing_cases.py on the two CPU routes of tests/inducing_u_ref.py (``inducing_u_cases.bounds``):
1000 x their gap on the test's own inputs, at least 4 eps, ``ugrad`` over ``S_u`` and ``kgrad`` over ``S``.
tests/test_inducing_vfe_host.py shows that the bound on ``ugrad`` rejects every wrong result of ``inducing_u_ref.DEFECTS`` on
the Matern problems.  The one exception is a single data point under FITC: ``C = k(x, x) + s`` whatever ``u``, the exact
gradient is 0, ``Z`` cancels to rounding and ``S_u`` with it; there the error is measured over ``S_u_terms``, the same sums
with the two parts of ``Z`` taken separately, at the rule's floor of 1000 x 4 eps.

``ugrad`` is one row of ``Z`` and ``W`` per inducing input, so it sees what the kernel gradient does not: the strips ``Z_J^T`` and
the ``W`` of ``gh_inducing_grad`` are products with the explicit inverse factors and carry an element-wise relative error of
eps cond(K_uu) (2e-6 on expsq_1d_m60, cond 1e9), which sums over ``j`` against derivatives smooth in ``u_j`` cancel (the kernel
gradient passes at 1e-17 of ``S``).  Fed to the reduction, they gave ``ugrad`` errors of 3e-8 .. 5e-8 of ``S_u`` on expsq_1d_m60
and 3.1e-12 on m32_1d_m129 (cond 1e5) under FITC, against bounds of 8.9e-13 and 2.0e-12; a NumPy emulation of the device's
formulas reproduced the 3.5e-8.  ``gh_inducing_grad_u`` therefore takes ``Z = P (alpha alpha^T - C^-1 - diag(omega))`` and
``W = -1/2 Z P^T`` from ``P`` itself, after a pass of its own for ``H Lambda^-1 P^T`` and ``P alpha``.  Largest error / bound seen
on one MI355X with that form: ``ugrad`` 0.017 (5.4e-14 of ``S_u`` against 3.1e-12, m52_2d_m65 under FITC; expsq_1d_m60 at most
6.6e-16 against 8.9e-13), ``kgrad`` 0.0061.  66 tests of this module and tests/test_gpu_inducing_vfe.py in 18 s, the CPU
restatement included.

Shapes: N = 777 in strips of 256 (four strips, the last ragged; 7 row tiles of 128 in one strip, the last of 9 rows) and in one
strip; m = 1 / 63 / 64 / 65 / 129 / 300 (the column tile is 64); the fast forms in 1-D, 2-D and 3-D, the interpreter (comp_3d
with one parameter frozen, a 5-D kernel), a metric on two of three axes, a kernel without parameters whose diagonal depends on
``u`` (m = 2), N = 1, and N = 100 under m = 129 inducing inputs that are no data points.
"""
import ctypes

import numpy as np
import pytest
import scipy.optimize

from george_amd import GP, InducingSolver
from george_amd import _native as N

import inducing_cases as IC
import inducing_u_cases as UC
import inducing_u_ref as UR
from inducing_cases import _check

pytestmark = pytest.mark.gpu

OBJECTIVE = pytest.mark.parametrize("objective", UR.OBJECTIVES)


def _solver(name, objective, strip):
    kernel, x, yerr, r, u, rel_jitter = UC.case(name)
    s = InducingSolver(kernel, inducing=u, method=UR.METHOD[objective], variational=objective == "vfe", jitter=rel_jitter, strip_points=strip)
    s.compute(x, yerr)
    return s


def _check_all(s, kernel, r, ref, tol, ugrad_scale=None):
    """grad_inducing against the restatement; ``grad`` gives the bits of its first three results, a second call and a call
    without ``which`` the same ``ugrad``"""
    mask = kernel.unfrozen_mask
    which = mask.astype(np.uint32)
    g, alpha, diagA, ugrad = s.grad_inducing(r, which)
    assert ugrad.shape == s.u.shape and len(g) == len(mask) and np.all(g[~mask] == 0.0)
    if mask.any():
        _check("kgrad", g[mask], ref.kgrad[mask], tol["kgrad"], scale=ref.S[mask])
    _check("alpha", alpha, ref.alpha, tol["alpha"])
    _check("diagA", diagA, ref.diagA, tol["diagA"])
    scale = ref.S_u if ugrad_scale is None else ugrad_scale
    assert np.all(ugrad[scale == 0.0] == 0.0)
    _check("ugrad", ugrad[scale > 0.0], ref.ugrad[scale > 0.0], tol["ugrad"], scale=scale[scale > 0.0])
    for a, b in zip(s.grad(r, which), (g, alpha, diagA)):
        assert np.array_equal(a, b)
    for a, b in zip(s.grad_inducing(r, which), (g, alpha, diagA, ugrad)):
        assert np.array_equal(a, b)
    g0, alpha0, diagA0, ugrad0 = s.grad_inducing(r)
    assert g0 is None and np.array_equal(alpha0, alpha) and np.array_equal(diagA0, diagA) and np.array_equal(ugrad0, ugrad)
    return ugrad


@OBJECTIVE
@pytest.mark.parametrize("name", list(UC.CASES) + ["dot"])
def test_against_the_restatement(name, objective):
    kernel, x, yerr, r, u, _ = UC.case(name)
    scale = None
    if (name, objective) == ("n1_m3", "fitc"):           # (the module docstring: the one degenerate pair)
        ref = UR.model(kernel, x, yerr, u, UC.bounds(name, "dtc")[0], objective, r)
        tol = {key: 4000 * IC.EPS for key in ("kgrad", "alpha", "diagA", "ugrad")}
        scale = ref.S_u_terms
        ref.S = np.full_like(ref.S, np.max(np.abs(ref.kgrad)))        # (kgrad: one term survives; over the gradient's own size)
    else:
        _, ref, tol = UC.bounds(name, objective)
    runs = []
    for strip in (256, 0):
        print("strip_points", strip)
        runs.append(_check_all(_solver(name, objective, strip), kernel, r, ref, tol, scale))
    s_u = ref.S_u if scale is None else scale
    _check("strips of 256 against one strip", runs[0][s_u > 0.0], runs[1][s_u > 0.0], tol["ugrad"], scale=s_u[s_u > 0.0])
    if name == "axes02_3d_m65":
        assert np.all(runs[0][:, 1] == 0.0) and np.all(runs[1][:, 1] == 0.0) and np.all(runs[0][:, [0, 2]] != 0.0)


def test_device_pointers_give_the_host_route_bits():
    """``r`` and the four array results as host memory, as device memory (``r`` also at an odd element offset) and mixed: the
    same status and the same bits, nothing written outside an output (tests/devptr.py)."""
    import devptr
    name = "m32_3d_m129"
    kernel, x, yerr, r, u, _ = UC.case(name)
    s = _solver(name, "vfe", 256)
    h, k, n = s._handle, s._dk.handle, len(x)
    which = np.ones(len(kernel), dtype=np.uint32)
    outs = dict(grad=devptr.Out((len(which),), np.float64), alpha=devptr.Out((n,), np.float64), diagA=devptr.Out((n,), np.float64),
                ugrad=devptr.Out(u.shape, np.float64))
    res = devptr.check_routes("gh_inducing_grad_u", lambda p: N.lib.gh_inducing_grad_u(h, k, N.ptr(which), p["r"], p["grad"], p["alpha"], p["diagA"],
                                                                                      p["ugrad"]), dict(r=r), outs, odd=("r",))
    assert res["host"][0] == N.GH_OK
    for a, b in zip(s.grad_inducing(r, which), (res["host"][1][key] for key in ("grad", "alpha", "diagA", "ugrad"))):
        assert np.array_equal(a, b)
    out = ctypes.c_double(-1.0)
    assert N.lib.gh_inducing_trace_term(h, ctypes.byref(out)) == N.GH_OK and out.value == s.trace_term > 0.0
    # the host checks, on a live handle: nothing is written
    ug = np.full(u.shape, 7.0)
    assert N.lib.gh_inducing_grad_u(h, k, N.ptr(which), N.ptr(r), None, None, None, N.ptr(ug)) == N.GH_ERR_BAD_ARG
    assert N.lib.gh_inducing_grad_u(h, k, None, N.ptr(r), None, None, None, None) == N.GH_ERR_BAD_ARG and np.all(ug == 7.0)


# ------------------------------------------------------------------ through GP
def _gp(name, n, m, objective, **kwargs):
    kernel, x, yerr, r, _ = IC._problem(name, n)
    gp = GP(kernel, solver=InducingSolver, inducing=m, method=UR.METHOD[objective], variational=objective == "vfe", **kwargs)
    gp.compute(x, yerr)
    return gp, x, yerr, r + 0.2


@OBJECTIVE
def test_through_gp_against_central_differences(objective):
    """``nll_and_grad_inducing`` -- constant mean, white noise, kernel parameters and every coordinate of ``u`` -- against central
    differences of ``GP.log_likelihood`` with a stationary kernel (step 1e-5: a truncation error of 1e-10 and a rounding error
    of eps |ll| / h = 1e-8 of the scale, bound 1e-6, as tests/test_gpu_inducing.py::test_through_gp), and what one call costs."""
    gp, x, yerr, y = _gp("m32_3d", 777, 12, objective, mean=0.2, fit_mean=True, white_noise=np.log(0.01), fit_white_noise=True)
    u0 = gp.inducing_inputs
    assert u0.shape == (12, 3) and np.array_equal(u0, gp.solver.u)
    v0 = np.concatenate([gp.get_parameter_vector(), u0.ravel()])
    npar = len(gp)

    def ll(v):
        gp.set_parameter_vector(v[:npar])
        gp.solver_kwargs["inducing"] = v[npar:].reshape(-1, 3).copy()
        gp.compute(x, yerr)
        return gp.log_likelihood(y)

    calls = []
    originals = {name: getattr(InducingSolver, name) for name in ("compute", "dot_solve", "grad_inducing", "grad", "apply_inverse")}
    try:
        for name, fn in originals.items():
            setattr(InducingSolver, name, (lambda fn, name: lambda self, *a, **k: (calls.append(name), fn(self, *a, **k))[1])(fn, name))
        nll, grad = gp.nll_and_grad_inducing(v0, y)
    finally:
        for name, fn in originals.items():
            setattr(InducingSolver, name, fn)
    assert sorted(calls) == ["compute", "dot_solve", "grad_inducing"]
    assert grad.shape == v0.shape and np.array_equal(gp.solver_kwargs["inducing"], u0)
    assert abs(nll + ll(v0)) <= 1e-12 * abs(nll)
    assert np.array_equal(-grad[npar:].reshape(-1, 3), gp.grad_log_likelihood_inducing(y))
    assert np.array_equal(-grad[:npar], gp.grad_log_likelihood(y))
    for a in range(len(v0)):
        h = 1e-5 * max(1.0, abs(v0[a]))
        up, dn = v0.copy(), v0.copy()
        up[a] += h
        dn[a] -= h
        fd = -(ll(up) - ll(dn)) / (2 * h)
        print("entry %d: gradient %.10g  central difference %.10g" % (a, grad[a], fd))
        assert abs(fd - grad[a]) <= 1e-6 * max(1.0, abs(grad[a])), (a, fd, grad[a])


def test_twenty_lbfgs_iterations_lower_the_objective():
    """N = 400, m = 8 in 1-D under the bound: hyper-parameters and inducing inputs jointly, ``jac=True``"""
    gp, x, yerr, y = _gp("m32_1d", 400, 8, "vfe")
    v0 = np.concatenate([gp.get_parameter_vector(), gp.inducing_inputs.ravel()])
    f0 = gp.nll_and_grad_inducing(v0, y)[0]
    res = scipy.optimize.minimize(gp.nll_and_grad_inducing, v0, jac=True, args=(y,), method="L-BFGS-B", options=dict(maxiter=20))
    print("objective %.6f -> %.6f in %d iterations, %d evaluations" % (f0, res.fun, res.nit, res.nfev))
    assert res.nit >= 1 and np.isfinite(res.fun) and res.fun < f0
    assert gp.nll_and_grad_inducing(res.x, y)[0] == res.fun and gp.inducing_inputs.shape == (8, 1)
