"""The gradient reference of tests/grad_ref.py, checked on the CPU: its accuracy against a 50-digit evaluation, the
power of its tolerance rule to reject a wrong reduction, the parameter counts of the GPU test problems, and the NumPy
kernel port against the reference's compiled evaluator on the 16-dimensional kernels.  (No GPU needed.)"""
import functools

import mpmath
import numpy as np
import pytest

import grad_ref as R
from george_amd import kernels as K
from george_amd.program import DeviceKernel
from oracle import kernels_np, ref_loader, solver_np


# ------------------------------------------------------------------ accuracy against mpmath
def _mp_gradient(kernel, x, yerr, r):
    """g, alpha and diag(A) from the same fp64 K and dK, with the Cholesky factor, the inverse and the contraction
    carried out in 50-digit arithmetic."""
    mp = mpmath.mp
    n = len(x)
    Kf = np.array(solver_np.kernel_matrix(kernel, x), dtype=np.float64)
    Kf[np.diag_indices(n)] += yerr ** 2
    G = kernels_np.gradient_general(kernel, x, x)
    with mpmath.workdps(50):
        Km = [[mp.mpf(float(Kf[i, j])) for j in range(n)] for i in range(n)]
        L = [[mp.mpf(0)] * n for _ in range(n)]
        for j in range(n):
            L[j][j] = mp.sqrt(Km[j][j] - mp.fsum(L[j][k] ** 2 for k in range(j)))
            for i in range(j + 1, n):
                L[i][j] = (Km[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
        Li = [[mp.mpf(0)] * n for _ in range(n)]
        for i in range(n):
            Li[i][i] = 1 / L[i][i]
            for j in range(i):
                Li[i][j] = -mp.fsum(L[i][k] * Li[k][j] for k in range(j, i)) / L[i][i]
        Kinv = [[mp.fsum(Li[k][i] * Li[k][j] for k in range(max(i, j), n)) for j in range(n)] for i in range(n)]
        rm = [mp.mpf(float(v)) for v in r]
        al = [mp.fsum(Kinv[i][j] * rm[j] for j in range(n)) for i in range(n)]
        A = [[al[i] * al[j] - Kinv[i][j] for j in range(n)] for i in range(n)]
        g = [mp.fsum(A[i][j] * mp.mpf(float(G[i, j, p])) for i in range(n) for j in range(n)) / 2
             for p in range(G.shape[2])]
        return (np.array([float(v) for v in g]), np.array([float(v) for v in al]),
                np.array([float(A[i][i]) for i in range(n)]))


MP_CASES = {
    "stationary_1d": (lambda: K.ConstantKernel(log_constant=0.2) * K.ExpSquaredKernel(0.7), 1),
    "product_of_sums": (lambda: R.kernel_p5(K), 2),
    "general_metric_3d": (lambda: K.ConstantKernel(log_constant=0.1, ndim=3) * K.Matern52Kernel(R._spd(3, 5, 1.0), ndim=3), 3),
}


@pytest.mark.parametrize("n", [17, 48])
@pytest.mark.parametrize("name", sorted(MP_CASES))
def test_reference_matches_50_digit_evaluation(name, n):
    make, ndim = MP_CASES[name]
    kernel = make()
    rng = np.random.RandomState(n + ndim)
    x = rng.uniform(0.0, 2.0, (n, ndim))
    yerr = 0.1 + 0.05 * rng.rand(n)
    r = rng.randn(n)
    ref = R.reference(kernel, x, yerr, r)
    g, alpha, diagA = _mp_gradient(kernel, x, yerr, r)
    assert ref.kappa <= 1e6
    assert np.all(ref.S >= np.abs(ref.g)) and np.all(ref.S > 0)
    assert ref.ratio_grad(g) < 1e-3, (ref.g, g)
    assert ref.ratio_alpha(alpha) < 1e-3
    assert ref.ratio_diagA(diagA) < 1e-3


# ------------------------------------------------------------------ the tolerance tells right from wrong
DISC_N = 129         # three tile rows of the device reduction, the last one ragged (a single row)
FAMILIES = sorted(R.PCASES) + ["depth8"]


@functools.lru_cache(maxsize=None)
def _disc_problem(family):
    if family == "depth8":
        kernel = R.deep_kernel(K, 8)
        rng = np.random.RandomState(8)
        x = rng.uniform(0.0, 2.0, (DISC_N, 16))
        return kernel, x, 0.1 + 0.05 * rng.rand(DISC_N), rng.randn(DISC_N)
    return R.problem(family, DISC_N)


def _has_product(spec):
    if bool(spec.is_kernel):
        return False
    return int(spec.operator_type) == 1 or _has_product(spec.k1) or _has_product(spec.k2)


@functools.lru_cache(maxsize=None)
def _disc_reference(family):
    return R.reference(*_disc_problem(family))


def _applicable(family, defect):
    kernel = _disc_problem(family)[0]
    if defect.startswith("swap"):
        return kernels_np.full_size(kernel) >= 2
    if defect == "product_wrong_operand":
        return _has_product(kernel)
    return True


@pytest.mark.parametrize("family,defect", [(f, d) for f in FAMILIES for d in R.DEFECTS if _applicable(f, d)])
def test_tolerance_rejects_a_defective_reduction(family, defect):
    kernel, x, yerr, r = _disc_problem(family)
    ref = _disc_reference(family)
    assert ref.kappa <= 1e6
    assert ref.ratio_grad(ref.g) == 0.0
    bad = R.reference(kernel, x, yerr, r, defect=defect)
    assert ref.ratio_grad(bad.g) >= 10.0, (family, defect, ref.ratio_grad(bad.g))


def test_every_family_meets_every_defect():
    # only the swaps of a one-parameter kernel and the product rule of a product-free one are left out
    missing = [(f, d) for f in FAMILIES for d in R.DEFECTS if not _applicable(f, d)]
    assert missing == [(1, "swap_first_pair"), (1, "swap_last_pair"), (1, "product_wrong_operand")]


# ------------------------------------------------------------------ construction guards
def _stack_depth(spec):
    if bool(spec.is_kernel):
        return 1
    return max(_stack_depth(spec.k1), 1 + _stack_depth(spec.k2))


def test_gpu_test_problems_have_their_intended_size():
    # the parameter-count matrix of tests/test_gpu_grad_reference.py: both sides of every instance boundary
    assert sorted(R.PCASES) == [1, 4, 5, 16, 17, 37, 64]
    for P, (make, ndim) in R.PCASES.items():
        kernel = make(K)
        assert kernels_np.full_size(kernel) == P
        assert len(kernel.get_parameter_vector(include_frozen=True)) == P
        assert kernel.ndim == ndim
        assert DeviceKernel(kernel).size == P
    assert {R.instance(P) for P in (1, 4)} == {4}
    assert {R.instance(P) for P in (5, 16)} == {16}
    assert {R.instance(P) for P in (17, 37, 64)} == {64}
    for P in (5, 17, 64):
        assert P in R.PCASES
    # the 16-dimensional kernels use every input axis and at most 8 active axes per leaf
    assert R.PCASES[64][0](K).ndim == 16
    # the stack-depth cases: exactly 8 operands at once, and one more
    k8, k9 = R.deep_kernel(K, 8), R.deep_kernel(K, 9)
    assert _stack_depth(k8) == 8 and _stack_depth(k9) == 9
    assert k8.ndim == 16 and kernels_np.full_size(k8) == 20 and R.instance(20) == 64
    # the parameter limit: 64 is the largest program, one more constant makes 65
    k65 = R.kernel_p64(K) + K.ConstantKernel(log_constant=0.0, ndim=16, axes=1)
    assert kernels_np.full_size(k65) == 65


def test_device_kernel_refuses_depth_9_and_65_parameters():
    # host-side validation in gh_kernel_create: nothing reaches a device
    DeviceKernel(R.deep_kernel(K, 8))
    with pytest.raises(ValueError, match="too deep"):
        DeviceKernel(R.deep_kernel(K, 9))
    with pytest.raises(ValueError, match="too many kernel parameters"):
        DeviceKernel(R.kernel_p64(K) + K.ConstantKernel(log_constant=0.0, ndim=16, axes=1))


# ------------------------------------------------------------------ NumPy port against the compiled reference
@pytest.mark.parametrize("name", ["p37", "p64", "depth8"])
def test_port_matches_compiled_evaluator_at_16_dimensions(name):
    KI = ref_loader.load_kernel_interface()
    if KI is None:
        pytest.skip("oracle/_ref not built")
    kernel = {"p37": lambda: R.kernel_p37(K), "p64": lambda: R.kernel_p64(K), "depth8": lambda: R.deep_kernel(K, 8)}[name]()
    rng = np.random.RandomState(16)
    x1 = rng.uniform(0.0, 2.0, (65, 16))
    x2 = rng.uniform(0.0, 2.0, (33, 16))
    P = kernels_np.full_size(kernel)
    ki = KI(kernel)
    v, vref = kernels_np.value_general(kernel, x1, x2), ki.value_general(x1, x2)
    assert np.max(np.abs(v - vref)) <= 1e-13 * np.max(np.abs(vref))
    g, gref = kernels_np.gradient_general(kernel, x1, x2), ki.gradient_general(np.ones(P, dtype=np.uint32), x1, x2)
    assert g.shape == gref.shape == (65, 33, P)
    assert np.max(np.abs(g - gref)) <= 1e-13 * np.max(np.abs(gref))
    gs, gsref = kernels_np.gradient_symmetric(kernel, x1), ki.gradient_symmetric(np.ones(P, dtype=np.uint32), x1)
    assert np.max(np.abs(gs - gsref)) <= 1e-13 * np.max(np.abs(gsref))
