"""NumPy restatement of ``VecchiaSolver.loo_blocks`` (gh_vecchia_loo, george_amd/csrc/gh_vecchia.hip): a plain loop over points on
top of ``vecchia_ref.reference``, and the tolerance rule of the tests that use it.

The Vecchia density is the Gaussian with precision ``Q = sum_i u_i u_i^T / f_i``, ``u_i = [-b_i; 1]`` on the block
``S_i = c(i) + {i}``.  Its leave-one-out quantities, exact for that density:

    c_j   = Q_jj = 1/f_j + sum over the rows i with j in c(i) of b_ij^2 / f_i,        alpha = Q r,
    resid = alpha / c,    var = 1 / c,    lpd = 1/2 log c - 1/2 alpha^2 / c - 1/2 log 2 pi,    L = sum_j lpd_j,

and with ``w = 1/2 (1 + alpha^2 / c) / c``, ``a = alpha / c``, ``M = diag(w) - 1/2 (a r^T + r a^T)`` restricted to ``S_i``:

    g = M u,    h = A^-1 g,    W(i) = (u.g / f^2) u u^T - (1/f) (h u^T + u h^T),
    kgrad = sum_i sum_jk W(i)_jk dA_jk/dtheta,    v = Q a  (= dL/dmean),    diagB_j = sum_{blocks with j} W_jj  (= dL/dK_jj),

the layout of ``BasicSolver.loo``, so that ``GP._assemble_grad(v, diagB, kgrad, diag_weight=1.0)`` applies unchanged; with every
predecessor in ``c`` these are the dense values (tests/loo_ref.py).  ``S[p]`` is the same sum over absolute values: the scale a
gradient error is measured against.  In the gradient pass ``u / f`` is the last column of ``A^-1`` and ``h`` a solve with the
WHOLE block ``A``, both from one SciPy Cholesky factor (the device takes ``b`` and ``f`` from the factor of ``K_cc`` and ``h`` by
the partitioned inverse on that factor alone); kernel values and gradients come from ``oracle.solver_np`` as in ``vecchia_ref``.

The tolerance rule is that of tests/vecchia_cases.py, nothing new: per quantity ``1000 x`` the gap between this restatement with
every predecessor in the conditioning set and the dense leave-one-out by LAPACK (``loo_ref.reference``) on the test's own first
``GAP_N`` points, a gap counting as at least ``4 eps``, vectors over their largest entry, the gradient over ``S``, no bound looser
than ``CAP`` = 1e-9, and no gap above ``GAP_CAP`` (``gaps`` asserts it: an ill-conditioned problem fails loudly instead of
widening its own bound).  Test helper only: not a conftest.
"""
import functools

import numpy as np
from scipy.linalg import cho_factor, cho_solve

import loo_ref
import vecchia_ref
from inducing_cases import EPS, GAP_CAP
from oracle import solver_np
from vecchia_cases import _over

GAP_N = 150
CAP = 1e-9
VECTORS = ("c", "resid", "var", "lpd", "v", "diagB")
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


class VecchiaLooRef(object):
    """``base`` (the ``VecchiaRef`` with ``B``, ``f``, ``alpha``), ``c``, ``L``, ``resid``, ``var``, ``lpd`` and, with
    ``want_grad``, ``kgrad``, ``S`` (P,), ``v``, ``diagB``"""

    def outputs(self):
        """the tuple ``loo_blocks`` returns with a mask of ones"""
        return self.L, self.resid, self.var, self.lpd, self.kgrad, self.v, self.diagB


def values(base, r):
    """``(c, alpha, resid, var, lpd)`` from the factors ``B``, ``f`` of ``vecchia_ref.reference``"""
    c = 1.0 / base.f
    for i, cols in enumerate(base.lists()):
        if len(cols):
            np.add.at(c, cols, base.B[i, base.nbr[i] >= 0] ** 2 / base.f[i])
    alpha = base.apply_q(r)
    resid = alpha / c
    return c, alpha, resid, 1.0 / c, 0.5 * np.log(c) - 0.5 * alpha * resid - HALF_LOG_2PI


def reference(spec, x, yerr, nbr, r, want_grad=True, block_spec=None):
    """``block_spec``: another kernel for the blocks of the gradient pass (``b``, ``f``, ``A`` and ``dA`` from it; ``c``,
    ``alpha``, ``w`` and ``a`` stay those of ``spec``, as a handle computed with ``spec`` keeps them); a block that does not
    factor under it adds nothing, and ``failed`` lists those points."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    x = x[:, None] if x.ndim == 1 else x
    r = np.ascontiguousarray(r, dtype=np.float64)
    n = len(x)
    yerr = np.zeros(n) + yerr
    base = vecchia_ref.reference(spec, x, yerr, nbr, r=r)
    out = VecchiaLooRef()
    out.base = base
    out.c, alpha, out.resid, out.var, out.lpd = values(base, r)
    out.L = float(np.sum(out.lpd))
    out.kgrad = out.S = out.v = out.diagB = None
    if not want_grad:
        return out
    w, a = 0.5 * (1.0 + alpha * out.resid) / out.c, out.resid
    out.v = base.apply_q(a)
    out.diagB = np.zeros(n)
    out.failed = []
    bspec = spec if block_spec is None else block_spec
    for lo in range(0, n, vecchia_ref.CHUNK):
        hi = min(n, lo + vecchia_ref.CHUNK)
        rows = base.nbr[lo:hi]
        pts = np.unique(np.concatenate([rows[rows >= 0], np.arange(lo, hi)]))      # index-sorted: lower index first
        Ku = solver_np.kernel_matrix(bspec, x[pts])
        Ku[np.diag_indices_from(Ku)] += yerr[pts] ** 2
        dKu = solver_np.kernel_gradient(bspec, x[pts])
        for i in range(lo, hi):
            slots = base.nbr[i] >= 0
            idx = np.concatenate([base.nbr[i][slots], [i]])
            blk = np.searchsorted(pts, idx)
            A, dA = Ku[np.ix_(blk, blk)], dKu[np.ix_(blk, blk)]
            try:
                cf = cho_factor(A, lower=True)
            except (np.linalg.LinAlgError, ValueError):                             # (ValueError: an entry that is not finite)
                out.failed.append(i)
                continue
            p = cho_solve(cf, np.eye(len(idx))[-1])                                 # A^-1 e_last = u / f
            f = 1.0 / p[-1]
            u = p * f
            g = w[idx] * u - 0.5 * (a[idx] * np.dot(r[idx], u) + r[idx] * np.dot(a[idx], u))
            h = cho_solve(cf, g)
            W = (np.dot(u, g) / (f * f)) * np.outer(u, u) - (np.outer(h, u) + np.outer(u, h)) / f
            kg, s = np.einsum("jk,jkp->p", W, dA), np.einsum("jk,jkp->p", np.abs(W), np.abs(dA))
            out.kgrad = kg if out.kgrad is None else out.kgrad + kg
            out.S = s if out.S is None else out.S + s
            np.add.at(out.diagB, idx, np.diag(W))
    return out


def full_table(n):
    """every predecessor in the conditioning set"""
    tab = np.full((n, max(n - 1, 1)), -1, dtype=np.int32)
    for i in range(1, n):
        tab[i, :i] = np.arange(i)
    return tab


def gaps(spec, x, yerr, r):
    """What two float64 routes on the CPU differ by on these inputs: this restatement with every predecessor in the conditioning
    set against the dense leave-one-out by LAPACK, per quantity.  Returns ``(gaps, restatement, dense)``."""
    ref = reference(spec, x, yerr, full_table(len(x)), r)
    d = loo_ref.reference(spec, x, yerr, r)
    g = dict(L=vecchia_ref.rel(ref.L, d.L), c=vecchia_ref.rel(ref.c, d.c), resid=vecchia_ref.rel(ref.resid, d.resid),
             var=vecchia_ref.rel(ref.var, d.var), lpd=vecchia_ref.rel(ref.lpd, d.lpd), v=vecchia_ref.rel(ref.v, d.v),
             diagB=vecchia_ref.rel(ref.diagB, d.diagB), kgrad=_over(ref.kgrad - d.g, ref.S))
    return g, ref, d


def tolerances(spec, x, yerr, r):
    """the bound per quantity from the first ``GAP_N`` points of the test's own inputs"""
    k = min(len(x), GAP_N)
    g = gaps(spec, x[:k], (np.zeros(len(x)) + yerr)[:k], r[:k])[0]
    print("gaps", {key: "%.1e" % v for key, v in g.items()})
    assert max(g.values()) <= GAP_CAP, "the problem is too ill-conditioned for these tests: replace it"
    return {key: min(1000.0 * max(v, 4 * EPS), CAP) for key, v in g.items()}


def check(what, got, want, tol, log=None):
    """the seven outputs ``got`` of ``loo_blocks`` against the restatement ``want``, each printed before it is asserted; without
    a gradient in ``got`` only the values"""
    import vecchia_cases
    L, resid, var, lpd, kgrad, v, diagB = got
    vecchia_cases._check(what + ": L", L, want.L, tol["L"])
    for name, val in (("resid", resid), ("var", var), ("lpd", lpd)):
        vecchia_cases._check(what + ": " + name, val, getattr(want, name), tol[name])
    if kgrad is None:
        assert v is None and diagB is None
        return
    vecchia_cases._check(what + ": kgrad", kgrad, want.kgrad, tol["kgrad"], scale=want.S)
    vecchia_cases._check(what + ": v", v, want.v, tol["v"])
    vecchia_cases._check(what + ": diagB", diagB, want.diagB, tol["diagB"])


@functools.lru_cache(maxsize=None)
def irregular_table(n, m):
    """A table in which point 0 is a neighbour of EVERY later row (the longest gather column: n - 1 entries) and the points
    ``j = 2 mod 3`` are nobody's neighbour (empty gather columns); rows with 1 .. m entries, not in ascending order, padding in
    the middle of every fifth row."""
    rng = np.random.RandomState(78)
    tab = np.full((n, m), -1, dtype=np.int32)
    for i in range(1, n):
        pool = np.array([j for j in range(1, i) if j % 3 != 2], dtype=np.int64)
        k = min(len(pool), rng.randint(0, m))
        near = pool[len(pool) - k // 2:] if k // 2 else pool[:0]
        far = rng.choice(pool, size=k, replace=False) if k else pool[:0]
        c = np.unique(np.concatenate([near, far]))[:k]
        c = rng.permutation(np.concatenate([[0], c]))
        slots = np.sort(rng.choice(m, size=len(c), replace=False)) if i % 5 == 0 else np.arange(len(c))
        tab[i, slots] = c
    return tab
