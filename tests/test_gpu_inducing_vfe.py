"""``InducingSolver(variational=True)`` on the device against the NumPy restatement (tests/inducing_u_ref.py): the trace term, the
``log_determinant`` that carries it, the bound ``F``, and the gradient of ``F`` in the kernel parameters and the error bars.

Tolerances: the rule of tests/inducing_cases.py on the two CPU routes of tests/inducing_u_ref.py (``inducing_u_cases.bounds``),
nothing else: 1000 x their gap on the test's own inputs, a gap of at least 4 eps, ``kgrad`` over ``S``, ``tau`` over
``tau_scale``; tests/test_inducing_vfe_host.py shows that these bounds reject each wrong result of ``inducing_u_ref.DEFECTS``.
Shapes: N = 777 in strips of 256 (four strips, the last ragged) and in one strip, m = 1 .. 300, the fast forms in 1-D, 2-D and
3-D and the interpreter.
"""
import numpy as np
import pytest

from george_amd import GP, BasicSolver, InducingSolver

import inducing_cases as IC
import inducing_u_cases as UC
import inducing_u_ref as UR
from inducing_cases import _check

pytestmark = pytest.mark.gpu

LOG2PI = np.log(2.0 * np.pi)


def _solver(name, objective, strip):
    kernel, x, yerr, r, u, rel_jitter = UC.case(name)
    s = InducingSolver(kernel, inducing=u, method=UR.METHOD[objective], variational=objective == "vfe", jitter=rel_jitter, strip_points=strip)
    s.compute(x, yerr)
    return s


@pytest.mark.parametrize("name", ["m32_3d_m129", "m32_3d_m300", "m32_1d_m129", "expsq_1d_m60", "m32_3d_m1", "m32_3d_m64", "m52_2d_m65",
                                  "comp_3d_m65", "m32_5d_m65", "n1_m3", "n100_m129", "dot"])
def test_the_bound_and_its_gradient(name):
    kernel, x, yerr, r, u, _ = UC.case(name)
    _, ref, tol = UC.bounds(name, "vfe")
    n, mask = len(x), kernel.unfrozen_mask
    for strip in (256, 0):
        print("strip_points", strip)
        s = _solver(name, "vfe", strip)
        assert s.trace_term >= 0.0
        _check("trace_term", s.trace_term, ref.tau, tol["tau"], scale=ref.tau_scale)
        _check("log_determinant", s.log_determinant, ref.logdet + ref.tau, tol["logdet"])
        _check("F", -0.5 * (s.dot_solve(r) + s.log_determinant + n * LOG2PI), ref.F, tol["ll"])
        g, alpha, diagA = s.grad(r, mask.astype(np.uint32))
        assert len(g) == len(mask) and np.all(g[~mask] == 0.0)
        if mask.any():
            _check("grad: kernel", g[mask], ref.kgrad[mask], tol["kgrad"], scale=ref.S[mask])
        _check("grad: alpha", alpha, ref.alpha, tol["alpha"])
        _check("grad: diagA", diagA, ref.diagA, tol["diagA"])
        g2, alpha2, diagA2 = s.grad(r, mask.astype(np.uint32))
        assert np.array_equal(g, g2) and np.array_equal(alpha, alpha2) and np.array_equal(diagA, diagA2)
        t = _solver(name, "vfe", strip)
        assert t.trace_term == s.trace_term and t.log_determinant == s.log_determinant


@pytest.mark.parametrize("name", ["m32_3d_m129", "comp_3d_m65"])
def test_everything_but_the_objective_is_dtc(name):
    """``solve``, ``dot_solve`` and ``predict`` are untouched: DTC's bits; DTC and FITC keep ``log|C|`` and a trace term of 0."""
    kernel, x, yerr, r, u, _ = UC.case(name)
    xs = np.random.RandomState(3).uniform(0, 2, (130, x.shape[1]))
    v, d, f = (_solver(name, objective, 256) for objective in ("vfe", "dtc", "fitc"))
    assert d.trace_term == 0.0 and f.trace_term == 0.0 and v.trace_term > 0.0
    assert v.log_determinant == d.log_determinant + v.trace_term
    for objective, s in (("dtc", d), ("fitc", f)):
        _check("log_determinant " + objective, s.log_determinant, UC.bounds(name, objective)[1].logdet, UC.bounds(name, objective)[2]["logdet"])
    assert v.dot_solve(r) == d.dot_solve(r) and np.array_equal(v.apply_inverse(r), d.apply_inverse(r))
    for a, b in zip(v.predict(kernel, r, xs, return_var=True)[:2], d.predict(kernel, r, xs, return_var=True)[:2]):
        assert np.array_equal(a, b)
    assert np.array_equal(v.grad(r, kernel.unfrozen_mask.astype(np.uint32))[1], d.grad(r, kernel.unfrozen_mask.astype(np.uint32))[1])


def test_the_bound_stays_below_the_dense_likelihood():
    """N = 300 against ``BasicSolver``, through ``GP``: ``log_likelihood`` IS the bound, at m = 10 / 20 / 40 nested max-min
    points non-decreasing and below the dense value (slack: the log-likelihood's tolerance, 4000 eps of its size)."""
    kernel, x, yerr, r, _ = IC._problem("m32_3d", 300)
    dense = GP(kernel, solver=BasicSolver)
    dense.compute(x, yerr)
    ll = dense.log_likelihood(r)
    F = []
    for m in (10, 20, 40):
        gp = GP(kernel, solver=InducingSolver, inducing=m, method="dtc", variational=True)
        gp.compute(x, yerr)
        F.append(gp.log_likelihood(r))
        assert gp.solver.trace_term > 0.0 and gp.inducing_inputs.shape == (m, 3)
    print(F, ll)
    slack = 4000 * IC.EPS * abs(ll)
    assert F[0] <= F[1] + slack and F[1] <= F[2] + slack and F[2] <= ll + slack and F[2] - F[0] > 1.0


def test_a_zero_error_bar_fails_as_under_dtc():
    kernel, x, yerr, r, u, _ = UC.case("m32_3d_m64")
    yerr = yerr.copy()
    yerr[5] = 0.0
    outcome = []
    for variational in (False, True):
        s = InducingSolver(kernel, inducing=u, method="dtc", variational=variational)
        try:
            s.compute(x, yerr)
            outcome.append((None, bool(np.isfinite(s.log_determinant))))
        except Exception as e:                   # noqa: BLE001  (whatever DTC raises is what the bound must raise)
            outcome.append((type(e), s.failed_factor))
    print(outcome)
    assert outcome[0] == outcome[1] and outcome[0] != (None, True)
