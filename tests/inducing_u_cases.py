"""What tests/test_inducing_vfe_host.py, tests/test_gpu_inducing_vfe.py and tests/test_gpu_inducing_ugrad.py share: the problems
and the tolerance rule.  Nothing here touches a device.

The rule is that of tests/inducing_cases.py: per compared quantity 1000 x the gap between the two CPU routes of
tests/inducing_u_ref.py (``model`` and ``dense``) on the test's own inputs, a gap counting as at least 4 eps, the log-determinant
and the log-likelihood no looser than ``inducing_cases.CAPS``, ``kgrad`` over ``S``, ``ugrad`` over ``S_u``; and no gap may
exceed ``GAP_CAP`` (``bounds`` asserts it: a problem that does is replaced, not the cap).
Test helper only: not a conftest.
"""
import functools

import numpy as np

from george_amd import kernels
from george_amd.solvers.inducing import inducing_points

import inducing_cases as IC
import inducing_u_ref as UR
from oracle import solver_np

N_MAIN = 777             # four strips of 256, the last ragged: 7 row tiles of 128, the last of 9 rows

# name -> (problem, N, m, inducing, relative jitter).  problem: a name of inducing_cases._problem or one of ``_extra``.
CASES = {
    "m32_3d_m129": ("m32_3d", N_MAIN, 129, "maxmin", 1e-10),
    "m32_3d_m300": ("m32_3d", N_MAIN, 300, "maxmin", 1e-10),
    "m32_1d_m129": ("m32_1d", N_MAIN, 129, "maxmin", 1e-10),
    "expsq_1d_m60": ("expsq_1d", N_MAIN, 60, "maxmin", 1e-8),        # cancels to 3e-9 of S_u: a conditioning probe
    "m32_3d_m1": ("m32_3d", N_MAIN, 1, "maxmin", 1e-10),
    "m32_3d_m63": ("m32_3d", N_MAIN, 63, "maxmin", 1e-10),
    "m32_3d_m64": ("m32_3d", N_MAIN, 64, "maxmin", 1e-10),
    "m32_3d_m65": ("m32_3d", N_MAIN, 65, "maxmin", 1e-10),
    "m52_2d_m65": ("m52_2d", N_MAIN, 65, "maxmin", 1e-10),           # the fast form in 2-D
    "comp_3d_m65": ("comp_3d", N_MAIN, 65, "maxmin", 1e-10),         # the interpreter; one parameter frozen
    "m32_5d_m65": ("m32_5d", N_MAIN, 65, "maxmin", 1e-10),           # the interpreter: more than 3 dimensions
    "axes02_3d_m65": ("axes02_3d", N_MAIN, 65, "random", 1e-10),     # a metric on axes 0 and 2 of 3: ugrad on axis 1 exactly 0
    "n1_m3": ("m32_3d", 1, 3, "random", 1e-10),
    "n100_m129": ("m32_3d", 100, 129, "random", 1e-10),              # more inducing inputs than data; none of them a data point
}
MATERN = ("m32_3d_m129", "m32_3d_m300", "m32_1d_m129")              # the problems the defects are judged on


@functools.lru_cache(maxsize=None)
def _extra(name, n):
    """(kernel, x, yerr, r) of the problems inducing_cases has not"""
    if name == "m52_2d":
        kernel, ndim, amp = 1.1 * kernels.Matern52Kernel(0.7, ndim=2), 2, np.sqrt(1.1)
    elif name == "m32_5d":
        kernel, ndim, amp = 0.9 * kernels.Matern32Kernel(1.5, ndim=5), 5, np.sqrt(0.9)
    else:
        kernel, ndim, amp = 1.2 * kernels.Matern32Kernel([0.6, 0.9], ndim=3, axes=[0, 2]), 3, np.sqrt(1.2)
    rng = np.random.RandomState(100 * ndim + n)
    x = rng.uniform(0, 2, (n, ndim))
    return kernel, x, amp * (0.1 + 0.05 * rng.rand(n)), amp * (np.sin(3.0 * x.sum(axis=1)) + 0.3 * rng.randn(n))


@functools.lru_cache(maxsize=None)
def case(name):
    """(kernel, x, yerr, r, u, relative jitter)"""
    if name == "dot":
        kernel, x, yerr, r, _, u = IC.dot_problem()
        return kernel, x, yerr, r, u, 1e-10
    problem, n, m, inducing, rel_jitter = CASES[name]
    kernel, x, yerr, r = (IC._problem(problem, n)[:4] if problem in ("m32_3d", "m32_1d", "expsq_1d", "comp_3d") else _extra(problem, n))
    if inducing == "maxmin":
        u = np.ascontiguousarray(x[inducing_points(x, m)])
    else:
        u = np.random.RandomState(m).uniform(0, 2, (m, x.shape[1]))
    return kernel, x, yerr, r, u, rel_jitter


@functools.lru_cache(maxsize=None)
def bounds(name, objective):
    """(absolute jitter, the restatement, tolerances) of ``case(name)`` under one objective of ``inducing_u_ref.OBJECTIVES``"""
    kernel, x, yerr, r, u, rel_jitter = case(name)
    jitter = rel_jitter * float(np.mean(solver_np.kernel_matrix(kernel, u, diag=True)))
    g, ref = UR.gaps(kernel, x, yerr, u, jitter, objective, r)
    print("gaps", name, objective, {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= IC.GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return jitter, ref, IC.tolerances(g)
