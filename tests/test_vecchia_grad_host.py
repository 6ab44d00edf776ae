"""The host side of tests/test_gpu_vecchia_grad.py: the restatement of ``vecchia_grad_kernel``'s LDS size against the table of
that module and against the constants of the sources, the problems of tests/vecchia_cases.py inside ``GAP_CAP``, and the bound
of the device tests against deliberately wrong gradients on those very problems.  No device is touched.

The wrong gradients model what the device reduction could get wrong without a fault (``kgrad(..., defect=)``; the block is the
one of the last point, which has all ``m`` neighbours):

================  =====================================================================================================
``drop_pair``     one off-diagonal pair of the block left out: the point and its last neighbour
``short_chunk``   the second half of the last 64-entry chunk of the block's packed triangle left out: a wrong ``nact``
``shifted_slot``  slot p of the block read from slot p + 1 (the last one from past the row: 0): a pitch off by one
``weight_one``    off-diagonal entries weighted 1 instead of 2, in every block
================  =====================================================================================================

Observed on the CPU, error over ``S`` against a bound of 8.9e-13 (4000 eps: the two CPU routes differ by 1e-17 .. 5e-16 of
``S``); every test prints them.  The weakest is ``drop_pair`` at P = 5, m = 7, 5.3e-6 in its worst slot; ``shifted_slot`` is at
least 4.3e-8 in every slot, and ``weight_one`` at least 2.5e-3 in its worst.
"""
import functools
import os
import re

import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve

import vecchia_cases as VC
import vecchia_ref
from oracle import kernels_np, solver_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFECTS = ("drop_pair", "short_chunk", "shifted_slot", "weight_one")

# case -> (parameters, dimension, LDS bytes of the gradient kernel at m = 64, at m = 7)
TABLE = {1: (1, 1, 29232, 10312), 4: (4, 3, 32320, 12488), 5: (5, 2, 31800, 12424), 16: (16, 4, 38984, 18696),
         17: (17, 4, 38984, 18696), "deep8": (20, 16, 47272, 21512), 37: (37, 16, 55464, 29704), 64: (64, 16, 69800, 44040)}


# ------------------------------------------------------------------ the LDS size
def test_lds_bytes_of_the_table():
    assert set(TABLE) == set(VC.PCASE_NAMES)
    for name, (P, ndim, big, small) in TABLE.items():
        kernel, x, yerr, r, xs = VC.pcase(name)
        assert kernels_np.full_size(kernel) == len(kernel) == P and x.shape == (300, ndim) and xs.shape == (7, ndim)
        assert np.all(np.diff(x[:, 0]) >= 0)
        assert VC.grad_lds_bytes(64, ndim, P) == big and VC.grad_lds_bytes(7, ndim, P) == small, name
    # P = 16 and 17 share one pitch; P = 64 leaves the evaluator GH_EVAL_WS + 1 doubles
    assert (16 + VC.GH_EVAL_WS) | 1 == (17 + VC.GH_EVAL_WS) | 1 == 33 and ((64 + VC.GH_EVAL_WS) | 1) - 64 == VC.GH_EVAL_WS + 1
    # the switch of group b: m = 57 the largest at or below 64 KB, m = 58 the smallest above, everything inside the raised limit
    assert VC.grad_lds_bytes(57, 16, 64) == 65240 and VC.grad_lds_bytes(58, 16, 64) == 65864
    assert VC.grad_lds_bytes(57, 16, 64) <= 65536 < VC.grad_lds_bytes(58, 16, 64) <= 96 * 1024
    sizes = [VC.grad_lds_bytes(m, 16, 64) for m in range(1, 65)]
    assert sizes == sorted(sizes) and sizes[-1] == 69800 <= VC.V_GRAD_LDS


def _source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_restatement_reads_the_constants_of_the_sources():
    hip = _source("george_amd", "csrc", "gh_vecchia.hip")
    impl = _source("george_amd", "csrc", "gh_vecchia_impl.h")
    ev = _source("george_amd", "csrc", "gh_eval.h")
    abi = _source("include", "george_amd.h")
    assert re.search(r"#define V_GRAD_LDS \((\d+) \* 1024\)", hip).group(1) == str(VC.V_GRAD_LDS // 1024)
    assert int(re.search(r"#define VM_MAX (\d+)\b", impl).group(1)) == VC.VM_MAX
    assert re.search(r"#define GH_EVAL_WS \(2 \* GH_MAX_AXES\)", ev)
    assert 2 * int(re.search(r"#define GH_MAX_AXES\s+(\d+)\b", abi).group(1)) == VC.GH_EVAL_WS
    assert int(re.search(r"#define GH_MAX_GRAD\s+(\d+)\b", abi).group(1)) == 64 == max(p for p, _, _, _ in TABLE.values())
    assert int(re.search(r"#define GH_MAX_NDIM\s+(\d+)\b", abi).group(1)) == 16 == max(d for _, d, _, _ in TABLE.values())
    # the formula and the pitch as the restatement has them, and the switch at 64 KB
    squeezed = re.sub(r"\s+", " ", hip)
    assert ("return (size_t)(m + 1) * nd + (m + 1) + v_tri(m + 1) + VM_MAX + 2 * (m + 1) + VM_MAX + (size_t)VM_MAX * gp + (m + 3) / 2;"
            in squeezed)
    assert "const int gp = (P + GH_EVAL_WS) | 1;" in squeezed and "if (lds > 64 * 1024) {" in squeezed


# ------------------------------------------------------------------ the problems and their bounds
@pytest.mark.parametrize("case", VC.PCASE_NAMES)
def test_the_restatement_stays_inside_every_bound(case):
    """the two CPU routes on the first 150 points: every gap within ``GAP_CAP`` (``gaps`` asserts it) and within its own bound"""
    g, tol = VC.gaps(case), VC.tolerances(case)
    assert set(g) == set(tol) == {"logdet", "quad", "ll", "alpha", "Kinv", "kgrad", "diagA", "mu", "var", "cov"}
    for key in g:
        assert g[key] <= VC.GAP_CAP and g[key] <= tol[key] <= max(1000.0 * g[key], 4000.0 * VC.EPS), key
    assert tol["logdet"] <= 1e-10 and tol["quad"] <= 1e-9 and tol["ll"] <= 1e-9
    # every conditional is well determined: a block's f is its error bar squared at the least
    ref = VC.reference(case, 300, 64)[0]
    assert ref.f.min() >= 1e-2


@pytest.mark.parametrize("n", [1, 2])
def test_the_smallest_problems(n):
    """N = 1 and 2 of the P = 64 kernel (and N = 1 of P = 1): the restatement, the table and the rule at their edge"""
    for case in (64, 1)[:3 - n]:
        kernel, x, yerr, r, xs = VC.pcase(case, n)
        ref, nbr = VC.reference(case, n, 64)
        assert nbr.shape == (n, 64) and np.array_equal(nbr[:, 1:], np.full((n, 63), -1)) and nbr[0, 0] == -1
        tol = VC.tolerances(case, n)
        assert ref.kgrad.shape == ref.S.shape == (len(kernel),) and ref.alpha.shape == ref.diagA.shape == (n,)
        if case == 64 and n == 1:
            assert np.sum(ref.S == 0.0) == 61 and np.all(ref.kgrad[ref.S == 0.0] == 0.0)
        d = vecchia_ref.dense(kernel, x, yerr, r)
        assert VC._over(ref.kgrad - d["kgrad"], d["S"]) <= tol["kgrad"]


def test_a_zero_scale_asks_for_an_exact_zero():
    logged = len(VC.LOG)
    VC._check("zero scale", [0.0, 1.0], [0.0, 1.0 + 1e-13], 1e-12, scale=np.array([0.0, 1.0]))
    VC._check("negative zero", [-0.0], [0.0], 1e-12, scale=np.array([0.0]))
    with pytest.raises(AssertionError):
        VC._check("zero scale", [1e-300, 1.0], [0.0, 1.0], 1e-12, scale=np.array([0.0, 1.0]))
    with pytest.raises(AssertionError):
        VC._check("beyond", [0.0, 1.0], [0.0, 1.0 + 1e-11], 1e-12, scale=np.array([0.0, 1.0]))
    with pytest.raises(AssertionError):
        VC._check("not finite", [0.0, np.nan], [0.0, 1.0], 1e-12, scale=np.array([0.0, 1.0]))
    del VC.LOG[logged:]


# ------------------------------------------------------------------ wrong gradients
class _Parts(object):
    """``kgrad``: the kernel gradient of ``vecchia_ref.reference``, added block by block in its order; ``lower``: the same with
    the triangle the device walks -- diagonal once, off-diagonal entries once; ``W`` and ``dA`` of the block ``block``"""


@functools.lru_cache(maxsize=None)
def _parts(case, m):
    kernel, x, yerr, r, xs = VC.pcase(case)
    ref, nbr = VC.reference(case, 300, m)
    n, out = len(x), _Parts()
    out.block, out.kgrad, out.lower = n - 1, None, None
    for lo in range(0, n, vecchia_ref.CHUNK):
        hi = min(n, lo + vecchia_ref.CHUNK)
        rows = nbr[lo:hi]
        pts = np.unique(np.concatenate([rows[rows >= 0], np.arange(lo, hi)]))
        Ku = solver_np.kernel_matrix(kernel, x[pts])
        Ku[np.diag_indices_from(Ku)] += yerr[pts] ** 2
        dKu = solver_np.kernel_gradient(kernel, x[pts])
        for i in range(lo, hi):
            c = nbr[i][nbr[i] >= 0]
            blk = np.searchsorted(pts, np.concatenate([c, [i]]))
            A, nc = Ku[np.ix_(blk, blk)], len(c)
            b = z = np.zeros(0)
            if nc:
                cf = cho_factor(A[:nc, :nc], lower=True)
                b, z = cho_solve(cf, A[:nc, nc]), cho_solve(cf, r[c])
            f = A[nc, nc] - np.dot(A[:nc, nc], b)
            e = r[i] - np.dot(b, r[c])
            u, ze = np.concatenate([-b, [1.0]]), np.concatenate([z, [0.0]])
            W = 0.5 * (e * e / (f * f) - 1.0 / f) * np.outer(u, u) + 0.5 * (e / f) * (np.outer(ze, u) + np.outer(u, ze))
            dA = dKu[np.ix_(blk, blk)]
            g, low = np.einsum("jk,jkp->p", W, dA), np.einsum("jk,jkp->p", np.tril(W), dA)
            out.kgrad = g if out.kgrad is None else out.kgrad + g
            out.lower = low if out.lower is None else out.lower + low
            if i == out.block:
                out.W, out.dA = W, dA
    return out


def kgrad(case, m, defect=None):
    """the restatement's kernel gradient of ``pcase(case)`` with ``m`` neighbours; ``defect``: one of ``DEFECTS``"""
    p = _parts(case, m)
    if defect is None:
        return p.kgrad
    if defect == "weight_one":
        return p.lower
    if defect not in DEFECTS:
        raise ValueError(defect)
    W, nb = p.W.copy(), len(p.W)
    good = np.einsum("jk,jkp->p", W, p.dA)
    if defect == "drop_pair":
        W[nb - 1, nb - 2] = W[nb - 2, nb - 1] = 0.0
    if defect == "short_chunk":
        T = nb * (nb + 1) // 2
        t0 = 64 * ((T - 1) // 64)
        nact = T - t0
        for t in range(t0 + nact - max(1, nact // 2), T):
            j = int((np.sqrt(8.0 * t + 1.0) - 1.0) / 2.0)
            j += (j + 1) * (j + 2) // 2 <= t
            k = t - j * (j + 1) // 2
            assert 0 <= k <= j < nb
            W[j, k] = W[k, j] = 0.0
    bad = np.einsum("jk,jkp->p", W, p.dA)
    if defect == "shifted_slot":
        bad = np.concatenate([good[1:], [0.0]])
    return p.kgrad - good + bad


@pytest.mark.parametrize("m", [7, 64])
@pytest.mark.parametrize("case", [5, 17, 64])
def test_the_bound_of_the_device_tests_rejects_every_defect(case, m):
    ref = VC.reference(case, 300, m)[0]
    tol = VC.tolerances(case)["kgrad"]
    assert np.array_equal(kgrad(case, m), ref.kgrad) and np.all(ref.S > 0.0)
    assert (ref.nbr[-1] >= 0).sum() == m
    with pytest.raises(ValueError):
        kgrad(case, m, defect="none")
    for defect in DEFECTS:
        err = np.abs(kgrad(case, m, defect) - ref.kgrad) / ref.S
        print("%-13s error over S %.3g .. %.3g  bound %.3g" % (defect, err.min(), err.max(), tol))
        assert err.max() > tol, (defect, err.max(), tol)
        if defect == "shifted_slot":
            assert err.min() > tol, (defect, err.min(), tol)
