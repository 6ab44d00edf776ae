"""Device-side sampling (needs an MI355X): the batched pivoted Cholesky ``gh_dev_pstrf`` through torch device pointers, the
solver entry ``BasicSolver.sample_conditional``, and ``GP.sample_conditional`` / ``GP.sample`` / ``GP.sample_conditional_batch``
with ``factor="cholesky"``.

The two bounds are those of tests/test_sample_host.py, derived there: reconstruction ``max|A - L L^T| <= 2 tol`` with ``tol``
the stop threshold actually used, and the affine law ``|draws - (mean + z[:, :rank] fac[:, :rank]^T)| <=
8 M eps (|z[:, :rank]| |fac[:, :rank]|^T + |mean|)`` entrywise."""
import numpy as np
import pytest

from sample_ref import EPS, affine_law, check_factor, default_tol, low_rank

pytestmark = pytest.mark.gpu


def pstrf(mats, tol=-1.0, pad=3):
    """gh_dev_pstrf on a list of equally sized matrices, lda = m + pad: (L (B, m, m), piv (B, m), rank (B), resid (B))"""
    import torch
    from george_amd import _native as N
    B, m = len(mats), len(mats[0])
    lda = m + pad
    a = np.full((B, m, lda), 7.5)                                       # (what lies between the rows is not the matrix)
    for b, mat in enumerate(mats):
        a[b, :, :m] = mat
    ad = torch.from_numpy(a).cuda()
    ld = torch.full((B, m, lda), -3.25, dtype=torch.float64, device="cuda")
    piv = torch.zeros((B, m), dtype=torch.int64, device="cuda")
    rank = torch.zeros(B, dtype=torch.int64, device="cuda")
    resid = torch.zeros(B, dtype=torch.float64, device="cuda")
    N.check(N.lib.gh_dev_pstrf(ad.data_ptr(), lda, m * lda, m, B, float(tol), ld.data_ptr(), lda, m * lda, piv.data_ptr(),
                               rank.data_ptr(), resid.data_ptr(), None))
    torch.cuda.synchronize()
    lh = ld.cpu().numpy()
    assert np.all(lh[:, :, m:] == -3.25)                                # nothing is written outside m x m
    return lh[:, :, :m].copy(), piv.cpu().numpy(), rank.cpu().numpy(), resid.cpu().numpy()


# (m, k): the edges of a 128-pivot panel and of the GEMM's 128-tiles; m > 512 takes the panel path
LOW_RANK = [(1, 1), (5, 3), (127, 37), (128, 128), (129, 37), (300, 64), (515, 129)]


@pytest.mark.parametrize("m,k", LOW_RANK)
def test_pstrf_low_rank(m, k):
    from george_amd.utils import pivoted_cholesky
    a = low_rank(m, k)
    tol = default_tol(a)
    L, piv, rank, resid = pstrf([a])
    assert rank[0] == k
    check_factor(a, L[0], piv[0], k, tol)
    assert np.all(piv[0, k:] == -1)
    assert resid[0] <= tol and (resid[0] == 0.0 or k < m)
    # the restatement takes the same pivots on these inputs (the remaining diagonal is 40x below the threshold at the end,
    # and the leading pivots are well separated); where it does, the factors agree to rounding
    Lr, pr, rr = pivoted_cholesky(a)
    assert rr == k
    if np.array_equal(pr, piv[0]):
        assert np.max(np.abs(Lr - L[0])) <= 1e-9 * np.sqrt(np.max(np.diagonal(a)))
    # two calls give the same bits
    L2, piv2, rank2, resid2 = pstrf([a])
    assert np.array_equal(L, L2) and np.array_equal(piv, piv2) and np.array_equal(rank, rank2) and np.array_equal(resid, resid2)


@pytest.mark.parametrize("m", [1, 5, 127, 128, 129, 300, 515])
def test_pstrf_exact_cases(m):
    rng = np.random.default_rng(7)
    v = rng.permutation(np.arange(1.0, m + 1.0)) / 7.0                  # distinct
    for at, val in ((514, 100.0), (128, 99.0), (127, 98.0)):            # the largest entries across workgroup-sized strides
        if at < m:
            v[at] = val
    L, piv, rank, resid = pstrf([np.diag(v)], tol=0.0)
    assert rank[0] == m and np.array_equal(piv[0], np.argsort(-v)) and resid[0] == 0.0
    want = np.zeros((m, m))
    want[piv[0], np.arange(m)] = np.sqrt(v[piv[0]])                     # diag(sqrt(v)) in pivot order: no swaps are made
    assert np.array_equal(L[0], want)                                   # bit for bit
    thr = float(np.median(v))
    L, piv, rank, resid = pstrf([np.diag(v)], tol=thr)
    assert rank[0] == np.sum(v > thr)
    if rank[0] < m:
        assert resid[0] == np.max(v[v <= thr])
    # the tie rule, the zero matrix, a negative diagonal entry
    L, piv, rank, resid = pstrf([np.eye(m), np.zeros((m, m)), np.diag(np.where(np.arange(m) % 2 == 1, -1.0, 2.0))], tol=0.0)
    assert rank[0] == m and np.array_equal(piv[0], np.arange(m)) and np.array_equal(L[0], np.eye(m))
    assert rank[1] == 0 and np.all(L[1] == 0) and np.all(piv[1] == -1) and resid[1] == 0.0
    assert rank[2] == (m + 1) // 2 and np.all(piv[2, :rank[2]] % 2 == 0) and np.all(L[2][1::2] == 0)
    assert resid[2] == (-1.0 if m > 1 else 0.0)


def test_pstrf_batch_and_nan_member():
    a0, a1, a2 = low_rank(129, 37), low_rank(129, 129) + np.eye(129), np.zeros((129, 129))
    L, piv, rank, resid = pstrf([a0, a1, a2])
    assert rank.tolist() == [37, 129, 0]
    check_factor(a0, L[0], piv[0], 37, default_tol(a0))
    check_factor(a1, L[1], piv[1], 129, default_tol(a1))
    assert np.all(L[2] == 0)
    # a NaN member between two good ones leaves the good ones right, bit for bit
    bad = a1.copy()
    bad[64, 64] = np.nan
    Ln, pn, rn, resn = pstrf([a0, bad, a1])
    assert rn.tolist() == [37, -1, 129] and np.all(np.isnan(Ln[1])) and np.isnan(resn[1])
    assert np.array_equal(Ln[0], L[0]) and np.array_equal(Ln[2], L[1])
    assert np.array_equal(pn[0], piv[0]) and np.array_equal(pn[2], piv[1])
    # the same on the panel path (m > 512)
    b0 = low_rank(515, 129)
    bad = b0.copy()
    bad[514, 514] = np.inf
    Lp, pp, rp, resp = pstrf([b0, bad, b0 + np.eye(515)])
    assert rp.tolist() == [129, -1, 515] and np.all(np.isnan(Lp[1]))
    check_factor(b0, Lp[0], pp[0], 129, default_tol(b0))
    check_factor(b0 + np.eye(515), Lp[2], pp[2], 515, default_tol(b0 + np.eye(515)))


def _cond_cases():
    from george_amd import kernels
    rng = np.random.RandomState(11)
    x = np.sort(rng.uniform(0, 10, 200))
    t = np.sort(np.concatenate([x[:150], rng.uniform(0, 10, 150)]))
    yield "expsq_N200_M300", kernels.ExpSquaredKernel(1.0), x, np.sin(x), t, 1e-3
    x = np.sort(rng.uniform(0, 10, 468))
    yield "expsq_N468_M250", kernels.ExpSquaredKernel(1.0), x, np.sin(x), np.linspace(0, 10, 250), 0.1
    x3 = rng.uniform(0, 3, (300, 3))
    yield ("m32_axis_N300_M129", kernels.Matern32Kernel(metric=[1.0, 0.1, 10.0], ndim=3), x3, np.sin(x3.sum(axis=1)),
           rng.uniform(0, 3, (129, 3)), 0.05)


@pytest.mark.parametrize("case", range(3))
def test_solver_sample_conditional(case):
    from george_amd import GP
    name, kernel, x, y, t, yerr = list(_cond_cases())[case]
    gp = GP(kernel, mean=0.25)
    gp.compute(x, yerr)
    mu, cov = gp.predict(y, t)
    xs = np.ascontiguousarray(gp.parse_samples(t), dtype=np.float64)
    m = len(xs)
    z = np.random.default_rng(case).standard_normal((7, m))
    draws, smu, fac, rank = gp.solver.sample_conditional(gp.kernel, gp._residual(y), xs, z, return_factor=True)
    tol = m * EPS * np.max(kernel.get_value(xs, diag=True))
    assert 0 < rank <= m
    for a in (draws, smu, fac):
        assert np.all(np.isfinite(a))
    assert np.array_equal(smu + gp._call_mean(xs), mu)                 # the launches of predict
    err = np.max(np.abs(cov - fac @ fac.T))
    print("\n[%s] rank %d of %d, max|cov - L L^T| = %.3g, tol = %.3g" % (name, rank, m, err, tol))
    assert err <= 2 * tol
    assert np.all(fac[:, rank:] == 0.0)
    affine_law(draws, smu, z, fac, rank, m)
    # an explicit threshold is used as given; two calls give the same bits
    d2, m2, f2, r2 = gp.solver.sample_conditional(gp.kernel, gp._residual(y), xs, z, tol=tol, return_factor=True)
    assert r2 == rank and np.array_equal(d2, draws) and np.array_equal(f2, fac)
    d3, _, r3 = gp.solver.sample_conditional(gp.kernel, gp._residual(y), xs, z[:1])
    assert r3 == rank and d3.shape == (1, m)
    affine_law(d3, smu, z[:1], fac, rank, m)
    assert gp.computed and np.array_equal(gp.predict(y, t)[0], mu)     # the factor is untouched


def test_gp_sample_conditional_and_sample_end_to_end():
    from george_amd import GP, kernels
    from george_amd.gp import TINY
    rng = np.random.RandomState(2)
    x = np.sort(rng.uniform(0, 10, 200))
    y = np.sin(x) + 0.1 * rng.randn(200)
    kernel = 0.8 * kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel, mean=-0.5)
    gp.compute(x, 0.1)
    t = np.linspace(0, 10, 500)
    m = 500
    mu, cov = gp.predict(y, t)
    xs = gp.parse_samples(t)
    _, smu, fac, rank = gp.solver.sample_conditional(gp.kernel, gp._residual(y), xs, np.zeros((1, m)), return_factor=True)
    for size in (1, 3):
        np.random.seed(31)
        got = gp.sample_conditional(y, t, size, factor="cholesky")
        assert got.shape == ((m,) if size == 1 else (size, m)) and np.all(np.isfinite(got))
        np.random.seed(31)
        z = np.random.standard_normal((size, m))
        affine_law(np.atleast_2d(got), mu, z, fac, rank, m)
    # the SVD path is today's, draw for draw
    from george_amd.utils import multivariate_gaussian_samples
    np.random.seed(4)
    want = multivariate_gaussian_samples(cov, 2, mean=mu)
    np.random.seed(4)
    assert np.array_equal(gp.sample_conditional(y, t, 2), want)
    # prior draws at t: K(t, t) + TINY I
    k = gp.get_matrix(t)
    k[np.diag_indices_from(k)] += TINY
    z0 = np.random.default_rng(0).standard_normal((3, m))
    d0, pfac, prank = gp.kernel.kernel.sample(xs, z0, jitter=TINY, return_factor=True)
    ptol = default_tol(k)
    assert 0 < prank <= m and np.max(np.abs(k - pfac @ pfac.T)) <= 2 * ptol and np.all(pfac[:, prank:] == 0)
    affine_law(d0, np.zeros(m), z0, pfac, prank, m)
    for size in (1, 3):
        np.random.seed(32)
        got = gp.sample(t, size, factor="cholesky")
        assert got.shape == ((m,) if size == 1 else (size, m)) and np.all(np.isfinite(got))
        np.random.seed(32)
        z = np.random.standard_normal((size, m))
        affine_law(np.atleast_2d(got), np.full(m, -0.5), z, pfac, prank, m)
    with pytest.raises(ValueError, match="factor"):
        gp.sample(t, factor="lu")


def test_gp_sample_conditional_batch(monkeypatch):
    from george_amd import GP, BasicSolver, kernels
    rng = np.random.RandomState(5)
    x = np.sort(rng.uniform(0, 10, 200))
    y = np.sin(x) + 0.1 * rng.randn(200)
    gp = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8), mean=0.1, white_noise=np.log(0.02), fit_white_noise=True)
    gp.compute(x, 0.0)
    t = np.linspace(0, 10, 129)
    m, size = 129, 5
    p0 = gp.get_parameter_vector()
    vec = p0 + 1e-2 * rng.randn(4, len(p0))
    names = gp.get_parameter_names()
    vec[2, names.index("white_noise:value")] = -300.0                   # numerically singular: not positive definite
    vec[2, names.index("kernel:k2:metric:log_M_0_0")] = np.log(1e8)
    solver, ll = gp.solver, gp.log_likelihood(y)
    np.random.seed(77)
    got = gp.sample_conditional_batch(vec, y, t, size=size, quiet=True, factor="cholesky")
    assert got.shape == (4, size, m)
    assert np.all(np.isnan(got[2])) and np.all(np.isfinite(got[[0, 1, 3]]))
    # the GP is what it was
    assert np.array_equal(gp.get_parameter_vector(), p0) and gp.computed and gp.solver is solver and gp.log_likelihood(y) == ll
    with pytest.raises(np.linalg.LinAlgError, match="member 2"):
        gp.sample_conditional_batch(vec, y, t, size=size, factor="cholesky")
    # the good members obey the affine law against their own predict_batch covariance and the solver's factor of it
    np.random.seed(77)
    z = np.random.standard_normal((4, size, m))                         # one call; the failed member's block is discarded
    mu, cov = gp.predict_batch(vec, y, t, quiet=True)
    kp, sigma, r, ok, mean_t = gp._batch_inputs(vec, y, True, t=gp.parse_samples(t))
    s = BasicSolver(gp.kernel)
    draws, smu, fac, rank, info = s.sample_conditional_batch(kp, gp._x, sigma, r, gp.parse_samples(t), z, return_factor=True)
    assert info[2] != 0 and rank[2] == -1 and np.all(np.isnan(draws[2])) and np.all(info[[0, 1, 3]] == 0)
    for b in (0, 1, 3):
        assert np.array_equal(smu[b] + mean_t[b], mu[b])
        # member b's prior scale: its own constant times the unit-variance ExpSquared
        gp_b = GP(kernels.ConstantKernel(0.3) * kernels.ExpSquaredKernel(0.8))
        gp_b.kernel.set_parameter_vector(kp[b], include_frozen=True)
        tol = m * EPS * np.max(gp_b.kernel.get_value(gp.parse_samples(t), diag=True))
        assert 0 < rank[b] <= m and np.max(np.abs(cov[b] - fac[b] @ fac[b].T)) <= 2 * tol
        assert np.all(fac[b][:, rank[b]:] == 0.0)
        affine_law(got[b], mu[b], z[b], fac[b], rank[b], m)
        assert np.array_equal(draws[b] + mean_t[b][None, :], got[b])
    np.random.seed(77)
    one = gp.sample_conditional_batch(vec[[0, 1, 3]], y, t, factor="cholesky")
    assert one.shape == (3, m)
    # the loop path (larger N, other solvers): the same random-number rule, the same formula
    monkeypatch.setattr(BasicSolver, "BATCH_MAX_N", 0)
    np.random.seed(77)
    loop = gp.sample_conditional_batch(vec, y, t, size=size, quiet=True, factor="cholesky")
    assert np.all(np.isnan(loop[2]))
    for b in (0, 1, 3):
        mu_b, fac_b, rank_b = _member_factor(gp, vec[b], y, t)
        affine_law(loop[b], mu_b, z[b], fac_b, rank_b, m)
    assert np.array_equal(gp.get_parameter_vector(), p0) and gp.computed


def _member_factor(gp, v, y, t):
    with gp._state_kept():
        gp.set_parameter_vector(v)
        gp.recompute()
        xs = np.ascontiguousarray(gp.parse_samples(t), dtype=np.float64)
        _, mu, fac, rank = gp.solver.sample_conditional(gp.kernel, gp._residual(y), xs, np.zeros((1, len(xs))), return_factor=True)
        return mu + gp._call_mean(xs), fac, rank
