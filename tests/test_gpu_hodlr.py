"""Parity of the HIP HODLR solver.

The oracle is the reference's own ``include/george/hodlr.h``, compiled unmodified against
``oracle/mini_eigen`` (``oracle/_ref/_hodlr``): its log-determinants, solves and per-node ranks on
``zoo.hodlr_configs`` are committed as ``tests/golden/hodlr.npz`` and -- the shared object travels
to the GPU box -- recomputed live here.  The HIP solver draws its pivot rows from a different
generator (one stream per node instead of one mt19937 threaded through the pre-order
construction), so ranks are compared as a distribution and values within the accuracy the
tolerance gives; on top of that the reference's own HODLR tests (tests/test_solvers.py:61-75,
tests/test_gp.py HODLR parametrisations, tests/test_tutorial.py:39-43: agreement with the dense
answer within allclose) and the published N=100 value."""
import numpy as np
import pytest

import zoo
import os

from oracle import solver_np, hodlr_np, ref_loader
from george_amd import kernels, GP, BasicSolver, HODLRSolver
from george_amd import _native as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HCONF = zoo.hodlr_configs(kernels)


@pytest.fixture(scope="module")
def golden_hodlr():
    return np.load(os.path.join(ROOT, "tests", "golden", "hodlr.npz"))


def _level_max(nodes):
    out = {}
    for lvl, _, _, r in nodes:
        out[int(lvl)] = max(out.get(int(lvl), 0), int(r))
    return out


@pytest.mark.parametrize("name", list(HCONF))
def test_against_reference_hodlr(name, golden_hodlr):
    """a17-a19 against the pinned oracle: log-determinant, K^-1 y, y^T K^-1 y and the rank profile."""
    g = golden_hodlr
    kernel, x, yerr, y, kw = HCONF[name]
    X = np.ascontiguousarray(x.reshape(len(x), -1))
    s = HODLRSolver(kernel, **kw)
    s.compute(X, yerr)
    ld = float(g[name + "/logdet"])
    # Both are approximations of the dense answer at the same tolerance, from different pivot rows:
    # the HIP solver must be as close to the exact (dense HIP solver, itself pinned to the reference's
    # LAPACK path) as the reference's HODLR is -- within a factor 10, or at rounding level.
    d = BasicSolver(kernel)
    d.compute(X, yerr)
    ld_d, a_d, q_d = d.log_determinant, d.apply_inverse(y), d.dot_solve(y)
    a0 = g[name + "/alpha"]
    tol, n = kw["tol"], len(x)
    # (a loose tolerance leaves O(tol) per block to chance -- which rows were drawn: allow that much)
    assert abs(s.log_determinant - ld_d) <= max(10 * abs(ld - ld_d), 1e-9 * abs(ld_d), 0.02 * tol * n), (s.log_determinant, ld, ld_d)
    if tol <= 1e-3:          # (at tol = 0.1 a rank-1..2 block model is as good as its luck with the rows: values unconstrained)
        scale = np.abs(a_d).max()
        assert np.abs(s.apply_inverse(y) - a_d).max() <= max(10 * np.abs(a0 - a_d).max(), 1e-7 * scale, 10 * tol * scale)
        assert abs(s.dot_solve(y) - q_d) <= max(10 * abs(float(g[name + "/dot"]) - q_d), 1e-9 * abs(q_d), tol * abs(q_d))
    # the live reference build, when the shared object travelled with the snapshot: same numbers as the golden
    H = ref_loader.load_hodlr()
    if H is not None:
        h = H()
        h.compute(kernel, X, yerr, **kw)
        assert h.log_determinant == ld
    # rank profile: same tree, and per level the largest rank within a few of the reference's --
    # except where the reference ran out of rows and took its exact rank-min(rows, cols) fallback
    # (hodlr.h:160-176); the HIP solver keeps the converged low-rank factors there
    ref_nodes = g[name + "/nodes"]
    mine = s.ranks()
    assert len(mine) == len(ref_nodes)
    ref_lv = _level_max(ref_nodes)
    order = np.lexsort((ref_nodes[:, 1], ref_nodes[:, 0]))             # breadth-first = our level order
    my_lv = {}
    for (lvl, _, _, _), r in zip(ref_nodes[order], mine):
        my_lv[int(lvl)] = max(my_lv.get(int(lvl), 0), int(r))
    for lvl, r_ref in ref_lv.items():
        fallback = any(r == sz // 2 for l2, _, sz, r in ref_nodes if l2 == lvl)
        if fallback:
            assert my_lv[lvl] <= r_ref
        else:
            assert abs(my_lv[lvl] - r_ref) <= max(3, r_ref // 5), (name, lvl, my_lv[lvl], r_ref)


def test_exhausted_rows_keep_low_rank_factors(golden_hodlr):
    """Matern-3/2 on sorted 1-D inputs has exactly rank-2 off-diagonal blocks.  The reference runs out
    of rows (all residuals < 1e-14) and returns rank = block size (golden: 600 at the root); the HIP
    solver stops with the rank-2..3 factors -- and the answers agree."""
    kernel, x, yerr, y, kw = HCONF["m32_exhausted"]
    s = HODLRSolver(kernel, **kw)
    s.compute(x[:, None], yerr)
    assert max(s.ranks()) <= 4 and int(golden_hodlr["m32_exhausted/nodes"][0, 3]) == 600
    assert abs(s.log_determinant - float(golden_hodlr["m32_exhausted/logdet"])) <= 1e-9 * abs(s.log_determinant)
    np.testing.assert_allclose(s.apply_inverse(y), golden_hodlr["m32_exhausted/alpha"], rtol=1e-6, atol=1e-7)


def test_rank_grows_past_256_and_cap_is_loud():
    """hodlr.h:147 lets the rank grow to min(rows, cols).  3-D inputs need it (docs/user/solvers.rst:40-42):
    the scratch is regrown and the result must still agree with the dense solver; a rank the solver
    cannot hold is an error, never a silently truncated factorisation."""
    x, yerr, y = zoo.bench_data(4096, ndim=3)
    kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
    s = HODLRSolver(kernel, tol=1e-7, min_size=100)                       # reference build: rank 400 at the root
    s.compute(x, yerr)                                                    # (values: test_against_reference_hodlr[c5like3d_4096_rank400])
    assert 256 < max(s.ranks()) <= 1024
    with pytest.raises(ValueError):                                       # explicit cap too small for the tolerance
        HODLRSolver(kernel, tol=1e-7, min_size=100, max_rank=64).compute(x, yerr)
    # a loose tolerance under the same cap is fine
    HODLRSolver(kernel, tol=0.1, min_size=100, max_rank=64).compute(x, yerr)
    # a block that needs more than the ACA's 1024 columns (hodlr.h:147 allows min(rows, cols) = 3000 here): the
    # solver answers with the exact dense device factorisation -- every tolerance is met -- and says so
    x2, yerr2, y2 = zoo.bench_data(6000, ndim=3)
    s2 = HODLRSolver(kernel, tol=1e-12, min_size=100)
    with pytest.warns(RuntimeWarning):
        s2.compute(x2, yerr2)
    assert s2.computed and s2.dense_fallback and s2.ranks() == []
    d = BasicSolver(kernel)
    d.compute(x2, yerr2)
    assert s2.log_determinant == d.log_determinant
    assert np.array_equal(s2.apply_inverse(y2), d.apply_inverse(y2)) and s2.dot_solve(y2) == d.dot_solve(y2)
    with pytest.raises(NotImplementedError):
        s2.apply_sqrt(y2)                                                 # (hodlr.py:62-64 either way)
    # the same solver object goes back to the HODLR path when the next problem is low-rank again
    s2.tol = 1e-6
    s2.compute(x, yerr)
    assert not s2.dense_fallback and max(s2.ranks()) > 0
    # through GP: log-likelihood against the dense solver
    gp = GP(kernel, solver=HODLRSolver, tol=1e-12)
    with pytest.warns(RuntimeWarning):
        gp.compute(x2, yerr2)
    gd = GP(kernel)
    gd.compute(x2, yerr2)
    assert gp.log_likelihood(y2) == gd.log_likelihood(y2)
    # beyond the size where a dense matrix is reasonable, and with an explicit cap, it stays an error
    old = HODLRSolver.DENSE_FALLBACK_MAX_N
    HODLRSolver.DENSE_FALLBACK_MAX_N = 1000
    try:
        with pytest.raises(ValueError):
            HODLRSolver(kernel, tol=1e-12, min_size=100).compute(x2, yerr2)
    finally:
        HODLRSolver.DENSE_FALLBACK_MAX_N = old


@pytest.mark.parametrize("N", [300, 1000, 417])
def test_hodlr_solver(N, seed=1234):                                  # tests/test_solvers.py:29-62
    kernel = 1.0 * kernels.ExpSquaredKernel(1.0)
    solver = HODLRSolver(kernel, tol=1e-10)
    np.random.seed(seed)
    x = np.atleast_2d(np.sort(10 * np.random.randn(N))).T
    yerr = np.ones(N)
    solver.compute(x, yerr)
    K = kernel.get_value(x)
    K[np.diag_indices_from(K)] += yerr ** 2
    sgn, lndet = np.linalg.slogdet(K)
    assert sgn == 1.0
    assert np.allclose(solver.log_determinant, lndet), (solver.log_determinant, lndet)
    y = np.sin(x[:, 0])
    b0 = np.linalg.solve(K, y)
    assert np.allclose(solver.apply_inverse(y).flatten(), b0)
    assert np.allclose(solver.apply_inverse(K), np.eye(N)), "Incorrect inverse"
    assert np.allclose(solver.get_inverse(), np.linalg.inv(K))
    assert np.allclose(solver.dot_solve(y), y @ b0)


def test_strange_hodlr_bug():                                         # tests/test_solvers.py:64-75
    x, yerr, y, amp = zoo.scaling_data(200)
    gp = GP(amp * kernels.ExpSquaredKernel(1.0), solver=HODLRSolver, seed=42)
    gp.compute(x, yerr)
    ll = gp.log_likelihood(y)
    ref = solver_np.gp_log_likelihood(solver_np.DenseOracle(amp * kernels.ExpSquaredKernel(1.0)), x[:, None], yerr, y)
    assert np.isfinite(ll) and abs(ll - ref) < 0.5         # default tol = 0.1: loose by construction
    gp.compute(x, yerr)                                    # "re-using HODLR factorizations" (HISTORY.rst:14)
    assert np.isclose(gp.log_likelihood(y), ll, rtol=1e-12)


def test_published_golden_single_leaf():
    """N=100 < 2*min_size: one exact leaf -> the published 133.946394912 (scaling.rst:91)."""
    kernel, x, yerr, y = zoo.gp_configs(kernels)["scaling100"]
    gp = GP(kernel, solver=HODLRSolver)
    gp.compute(x, yerr)
    assert abs(gp.log_likelihood(y) - 133.946394912) < 5e-9


@pytest.mark.parametrize("white_noise", [None, 0.1])
def test_gradient_hodlr(white_noise, seed=123, N=305, ndim=3, eps=1.32e-3):   # tests/test_gp.py:16-56
    np.random.seed(seed)
    kernel = 1.0 * kernels.ExpSquaredKernel(0.5, ndim=ndim)
    kwargs = dict(tol=1e-8)
    if white_noise is not None:
        kwargs.update(white_noise=white_noise, fit_white_noise=True)
    gp = GP(kernel, solver=HODLRSolver, **kwargs)
    x = np.random.rand(N, ndim)
    x = x[np.argsort(x[:, 0])]
    y = gp.sample(x)
    gp.compute(x, yerr=0.1)
    grad0 = gp.grad_log_likelihood(y)
    vector = gp.get_parameter_vector()
    for i, v in enumerate(vector):
        vector[i] = v + eps
        gp.set_parameter_vector(vector)
        lp = gp.log_likelihood(y)
        vector[i] = v - eps
        gp.set_parameter_vector(vector)
        lm = gp.log_likelihood(y)
        vector[i] = v
        gp.set_parameter_vector(vector)
        assert np.abs(0.5 * (lp - lm) / eps - grad0[i]) < 5 * eps


def test_prediction_and_apply_inverse_hodlr(seed=42):                 # tests/test_gp.py:59-83,123-171
    np.random.seed(seed)
    kernel = kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel, solver=HODLRSolver, white_noise=0.0, tol=1e-8)
    x0 = np.linspace(-10, 10, 500)
    x = np.sort(np.random.uniform(-10, 10, 300))
    gp.compute(x)
    y = np.sin(x)
    mu, cov = gp.predict(y, x0)
    Kstar = gp.get_matrix(x0, x)
    K = gp.get_matrix(x)
    K[np.diag_indices_from(K)] += 1.0
    assert np.allclose(mu, np.dot(Kstar, np.linalg.solve(K, y)))
    gp2 = GP(1.0 * kernels.ExpSquaredKernel(0.5), solver=HODLRSolver, tol=1e-10)
    xs = np.sort(np.random.rand(201))
    ys = gp2.sample(xs)
    gp2.compute(xs, yerr=0.1)
    K2 = gp2.get_matrix(xs)
    K2[np.diag_indices_from(K2)] += 0.01
    assert np.allclose(np.linalg.solve(K2, ys), gp2.apply_inverse(ys))
    Y5 = gp2.sample(xs, size=5).T
    assert np.allclose(np.linalg.solve(K2, Y5), gp2.apply_inverse(Y5))
    mu0, var0 = gp2.predict(ys, [0.0], return_var=True)
    mu1, var1 = gp2.predict(ys, [0.0, 1.0], return_var=True)
    assert np.allclose(mu0, mu1[0]) and np.allclose(var0, var1[0])


def test_tutorial_default_tolerance():                                # tests/test_tutorial.py:39-43
    rng = np.random.RandomState(1)
    x = np.sort(rng.uniform(0, 30, 50))
    y = np.sin(x) + 0.1 * rng.randn(50)
    kernel = 2.0 * kernels.Matern32Kernel(3.0) + 0.001
    a = GP(kernel, solver=BasicSolver)
    a.compute(x, 0.1)
    b = GP(kernel, solver=HODLRSolver)
    b.compute(x, 0.1)
    assert np.allclose(a.log_likelihood(y), b.log_likelihood(y))


@pytest.mark.parametrize("n,min_size", [(8192, 100), (5000, 64), (3001, 200)])
def test_mid_size_vs_dense_and_numpy_restatement(n, min_size):
    """Unbalanced trees (odd sizes, leaves at different depths) against the dense HIP solver and
    the NumPy restatement of hodlr.h at tol = 1e-10."""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    h = GP(kernel, solver=HODLRSolver, tol=1e-10, min_size=min_size)
    h.compute(x, yerr)
    d = GP(kernel, solver=BasicSolver)
    d.compute(x, yerr)
    ll_h, ll_d = h.log_likelihood(y), d.log_likelihood(y)
    assert abs(ll_h - ll_d) <= 1e-7 * abs(ll_d), (ll_h, ll_d)
    assert np.allclose(h.apply_inverse(y), d.apply_inverse(y), rtol=1e-5, atol=1e-7)
    if n <= 5000:
        o = hodlr_np.HODLROracle(kernel, tol=1e-10, min_size=min_size)
        ll_o = solver_np.gp_log_likelihood(o, x[:, None], yerr, y)
        assert abs(ll_h - ll_o) <= 1e-7 * abs(ll_o)
        # ranks are of the same order as the restatement's (different RNG streams -> not identical)
        assert max(h.solver.ranks()) <= 2 * max(max(v) for v in o.root.ranks().values()) + 8


@pytest.mark.parametrize("n", [65536, 262144])
def test_c4_shape_properties(n):
    """BASELINE config C4 (N=262144, tol=1e-10) and a quarter of it: residual of the solve against
    an independent device mat-vec on a row sample, determinism."""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    gp = GP(kernel, solver=HODLRSolver, tol=1e-10)
    gp.compute(x, yerr)
    alpha = gp.apply_inverse(y)
    X = x[:, None]
    rows = np.random.RandomState(0).choice(n, 512, replace=False)
    Kr = kernel.get_value(X[rows], X)
    Kr[np.arange(512), rows] += yerr[rows] ** 2
    assert np.abs(Kr @ alpha - y[rows]).max() < 1e-6
    ll = gp.log_likelihood(y)
    gp2 = GP(kernel, solver=HODLRSolver, tol=1e-10)
    gp2.compute(x, yerr)
    assert gp2.log_likelihood(y) == ll


@pytest.mark.parametrize("leaf_gj", [False, True])
def test_hodlr_not_positive_definite_leaf(leaf_gj):
    """A leaf block that is not positive definite must surface as LinAlgError (what GP.compute
    catches, gp.py:356) from the batched-Cholesky leaf path; the Gauss-Jordan path (general leaves)
    only fails on exactly singular blocks, so there the answer just has to be finite or an error."""
    n = 512 if not leaf_gj else 600                      # leaves of 128 rows / 150 rows (2 x 2 blocked Cholesky, or Gauss-Jordan on request)
    x = np.linspace(0, 3, n)[:, None]
    k = kernels.CosineKernel(log_period=0.0)             # rank-2 kernel: every leaf is singular
    for env in ([None] if not leaf_gj else [None, "1"]):
        if env:
            N.lib.gh_debug_set_hodlr_leaf_gj(1)
        try:
            s = HODLRSolver(k, tol=1e-10)
            if env is None:
                with pytest.raises(np.linalg.LinAlgError):
                    s.compute(x, np.zeros(n))
                assert not s.computed
            else:
                try:
                    s.compute(x, np.zeros(n))
                except (np.linalg.LinAlgError, RuntimeError):
                    assert not s.computed
        finally:
            N.lib.gh_debug_set_hodlr_leaf_gj(0)


@pytest.mark.parametrize("n", [3000, 1560, 10000])
def test_blocked_cholesky_leaves_match_gauss_jordan_and_dense(n):
    """leaves of 129 .. 256 rows (n = 3000: 187 / 188 rows; 1560: 195; 10000: 156 / 157): the 2 x 2 blocked Cholesky path on
    256 x 256 slots (round 5) against the pivoted Gauss-Jordan it replaces (gh_debug_set_hodlr_leaf_gj(1)) and the dense solver"""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    X = x[:, None]
    got = {}
    for env in (None, "1"):
        if env:
            N.lib.gh_debug_set_hodlr_leaf_gj(1)
        try:
            s = HODLRSolver(kernel, tol=1e-12)
            s.compute(X, yerr)
            wide = np.stack([np.cos((q + 1) * x) for q in range(20)], axis=1)      # 20 right-hand sides: the tile-kernel path, leaf pitch 256
            got[env] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(np.stack([y, np.cos(x)], axis=1)), s.apply_inverse(wide))
        finally:
            N.lib.gh_debug_set_hodlr_leaf_gj(0)
    a, b = got[None], got["1"]
    assert abs(a[0] - b[0]) <= 1e-11 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-9 * abs(b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=0, atol=1e-8 * np.abs(b[2]).max())
    np.testing.assert_allclose(a[3], b[3], rtol=0, atol=1e-8 * np.abs(b[3]).max())
    np.testing.assert_allclose(a[3][:, 0], s.apply_inverse(np.cos(x)), rtol=0, atol=1e-8 * np.abs(a[3][:, 0]).max())   # wide against narrow
    if n <= 3000:
        d = BasicSolver(kernel)
        d.compute(X, yerr)
        assert abs(a[0] - d.log_determinant) <= 1e-9 * abs(d.log_determinant)
        assert abs(a[1] - d.dot_solve(y)) <= 1e-7 * abs(d.dot_solve(y))


@pytest.mark.parametrize("n", [4096, 16384, 3000])
def test_shared_passes_match_separate_launches(n):
    """gh_debug_set_hodlr_passes: the sweep's update + next level's reduce in one pass (and the deepest level's reduce inside the
    leaf product) multiply the same doubles in the same order as the separate launches -- the log-determinant and the factors
    are IDENTICAL; the narrow solve's passes change the order of a few sums -- agreement to rounding.  n = 4096, 16384: leaves
    of 128 rows, every pass shared; n = 3000: chunks differ from level to level, the sweep falls back to separate launches."""
    from george_amd import _native as N
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    got = {}
    try:
        for mask in (0, 2, 1, 3):
            N.lib.gh_debug_set_hodlr_passes(mask)
            s = HODLRSolver(kernel, tol=1e-10)
            s.compute(x[:, None], yerr)
            got[mask] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y))
    finally:
        N.lib.gh_debug_set_hodlr_passes(-1)
    assert got[2][0] == got[0][0] and got[3][0] == got[0][0] and got[1][0] == got[0][0]
    assert got[2][1] == got[0][1] and np.array_equal(got[2][2], got[0][2])            # the sweep: same bits
    for m in (1, 3):
        assert abs(got[m][1] - got[0][1]) <= 1e-10 * abs(got[0][1])
        np.testing.assert_allclose(got[m][2], got[0][2], rtol=0, atol=1e-9 * np.abs(got[0][2]).max())


@pytest.mark.parametrize("case", ["c4_4096", "c4_16384", "c4_65536", "min50", "ragged_3000", "default_tol", "interp_sum", "overflow_3d", "matern_tight"])
def test_wave_per_node_aca_gives_the_same_bits(case):
    """hodlr_aca_wave_kernel (one wavefront per node for blocks of <= 256 x 256 -- 64 / 128 / 256: one, two, four entries per lane;
    min50: 64 x 64 blocks -- four nodes per workgroup, no workgroup barrier)
    against the one-workgroup-per-node kernel (gh_debug_set_hodlr_wave_aca(0)): same generator, same draws, the workgroup
    kernel's reduction trees -- ranks, log-determinant, solves IDENTICAL.  overflow_3d / matern_tight: deep blocks that need more
    than the wavefront kernel's eight (six for 256 x 256 blocks) columns -- the level is redone with the workgroup kernel (and on the handle's second
    compute() goes there directly): still identical."""
    if case == "overflow_3d":
        x, yerr, y = zoo.bench_data(3000, ndim=3)
        kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
        X, kw = np.ascontiguousarray(x), dict(tol=1e-6)
    else:
        n = {"c4_4096": 4096, "c4_16384": 16384, "c4_65536": 65536, "min50": 4096, "ragged_3000": 3000, "default_tol": 10000, "interp_sum": 5000, "matern_tight": 6000}[case]
        x, yerr, y = zoo.bench_data(n)
        X = x[:, None]
        if case == "interp_sum":
            kernel = 0.3 * kernels.ExpSquaredKernel(1.0) + 0.2 * kernels.Matern32Kernel(2.0)      # two stationary leaves: the interpreter
        elif case == "matern_tight":
            kernel = np.var(y) * kernels.Matern32Kernel(1.0)
        else:
            kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
        kw = dict(tol=0.1) if case == "default_tol" else dict(tol=1e-10, min_size=50) if case == "min50" else dict(tol=1e-10)
    got = {}
    try:
        for mode in (0, 1):
            N.lib.gh_debug_set_hodlr_wave_aca(mode)
            s = HODLRSolver(kernel, **kw)
            s.compute(X, yerr)
            first = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y), list(s.ranks()))
            s.compute(X, yerr)                                     # (second compute() of the handle: overflowed levels remembered)
            assert s.log_determinant == first[0] and s.dot_solve(y) == first[1]
            got[mode] = first
    finally:
        N.lib.gh_debug_set_hodlr_wave_aca(1)
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1]
    assert np.array_equal(got[1][2], got[0][2])
    assert got[1][3] == got[0][3]


@pytest.mark.parametrize("n, tol", [(4096, 1e-10), (16384, 1e-10), (65536, 1e-10), (5000, 1e-8), (20000, 1e-3)])
def test_leaf_product_from_the_level_major_copy_gives_the_same_bits(n, tol):
    """Round 6: the compaction writes the level-major copy V only; the factorisation's leaf product reads a leaf's rows from it
    (a contiguous piece per level) and writes the row-major U for the first time (gh_debug_set_hodlr_u_from_v; LeafSrc in
    gh_hodlr_impl.h).  The LDS image the product multiplies from holds the same doubles: identical ranks, log-determinant and solves.
    n = 5000: ragged leaves (rows past a leaf's end are zeros in the image); tol = 1e-3: few columns, levels of rank zero."""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    got = {}
    try:
        for mode in (0, 1):
            N.lib.gh_debug_set_hodlr_u_from_v(mode)
            s = HODLRSolver(kernel, tol=tol, min_size=64 if n != 5000 else 40)
            s.compute(x[:, None], yerr)
            got[mode] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y), list(s.ranks()))
            del s
    finally:
        N.lib.gh_debug_set_hodlr_u_from_v(1)
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1] and got[1][3] == got[0][3]
    assert np.array_equal(got[1][2], got[0][2])


@pytest.mark.parametrize("n, tol, min_size", [(8192, 1e-10, 64), (65536, 1e-10, 64), (20000, 1e-6, 64), (30000, 1e-12, 40), (12000, 1e-3, 64)])
def test_fused_core_launch_gives_the_same_bits(n, tol, min_size):
    """Round 6: for the levels with many small nodes, the sum of the chunk partials, the core's pivoted Gauss-Jordan and the core
    product are ONE launch with a workgroup per node (hodlr_core_kernel) instead of three (gh_debug_set_hodlr_core_fused(0)): the
    same doubles through the same operations in the same order -- ranks, log-determinant and solves IDENTICAL.  tol = 1e-12: cores
    of up to 32 rows (all three instantiations); min_size = 40: ragged chunks; tol = 1e-3: levels of rank zero or one."""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    got = {}
    try:
        for mode in (0, 1):
            N.lib.gh_debug_set_hodlr_core_fused(mode)
            s = HODLRSolver(kernel, tol=tol, min_size=min_size)
            s.compute(x[:, None], yerr)
            got[mode] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y), list(s.ranks()))
            s.compute(x[:, None], yerr)
            assert s.log_determinant == got[mode][0]
            del s
    finally:
        N.lib.gh_debug_set_hodlr_core_fused(1)
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1] and got[1][3] == got[0][3]
    assert np.array_equal(got[1][2], got[0][2])


@pytest.mark.parametrize("n", [65536, 131072])
def test_phase_one_packing_gives_the_same_bits(n):
    """Round 6, late: WHO GETS A CU WHEN in the ACA phase -- the clusters below the root at half the even-load width
    (gh_debug_set_hodlr_coop_lower), a second level of one-workgroup nodes inside the cooperative launch, the one-workgroup launch
    longest first by the durations the nodes reported in the handle's previous compute() (gh_debug_set_hodlr_lpt), one barrier for
    all the block sums of an ACA step -- changes no arithmetic: ranks, log-determinant and solves IDENTICAL in every arm, and from
    the first compute() of a handle (tree order) to its third (sorted by the second's durations)."""
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    got = {}
    try:
        for lower, lpt in ((1, 0), (2, 0), (2, 1), (4, 1)):
            N.lib.gh_debug_set_hodlr_coop_lower(lower)
            N.lib.gh_debug_set_hodlr_lpt(lpt)
            s = HODLRSolver(kernel, tol=1e-10)
            res = []
            for rep in range(3):
                s.compute(x[:, None], yerr)
                res.append((s.log_determinant, s.dot_solve(y), list(s.ranks())))
            assert res[1] == res[0] and res[2] == res[0]
            got[(lower, lpt)] = (res[0], s.apply_inverse(y))
            del s
    finally:
        N.lib.gh_debug_set_hodlr_coop_lower(-1)
        N.lib.gh_debug_set_hodlr_lpt(1)
    ref = got[(1, 0)]
    for key, val in got.items():
        assert val[0] == ref[0], key
        assert np.array_equal(val[1], ref[1]), key


@pytest.mark.parametrize("n,ndim", [(4096, 1), (5000, 1), (6000, 3)])
def test_leaf_blocks_evaluated_inside_the_factorisation_kernel(n, ndim):
    """Round 6: 128-row leaves of fast-form kernels are evaluated inside potf2_kinv_kernel (no build launch, nothing written but
    K_leaf^-1); with gh_debug_set_hodlr_leaf_fused(0) the build launch writes the blocks first.  Same evaluator, same ordered
    arguments: identical log-determinant and solves.  n = 5000: ragged leaves (identity padding inside the kernel); 3-D inputs."""
    x, yerr, y = zoo.bench_data(n, ndim=ndim)
    X = x[:, None] if ndim == 1 else np.ascontiguousarray(x)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0) if ndim == 1 else 0.7 * kernels.Matern32Kernel(0.5, ndim=3)
    got = {}
    try:
        for mode in (0, 1):
            N.lib.gh_debug_set_hodlr_leaf_fused(mode)
            s = HODLRSolver(kernel, tol=1e-8, min_size=64 if n != 5000 else 40)
            s.compute(X, yerr)
            got[mode] = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y))
    finally:
        N.lib.gh_debug_set_hodlr_leaf_fused(1)
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1] and np.array_equal(got[1][2], got[0][2])
    d = BasicSolver(kernel)
    d.compute(X, yerr)
    assert abs(got[1][0] - d.log_determinant) <= 1e-6 * abs(d.log_determinant)


def test_parked_handles_are_bounded_and_reused():
    """A dropped HODLRSolver parks its native handle for the next solver with the same options (GP makes a new solver
    per compute, gp.py:327): at most two per option set and four in all, oldest option set evicted first."""
    kernel, x, yerr, y, kw = HCONF["solver1000"]
    HODLRSolver.release_pool()
    X = x[:, None]
    want = None
    for tol in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8):
        for _ in range(3):
            s = HODLRSolver(kernel, min_size=100, tol=tol, seed=42)
            s.compute(X, yerr)
            del s
    parked = sum(len(v) for v in HODLRSolver._HPOOL.values())
    assert 1 <= parked <= HODLRSolver._HPOOL_TOTAL
    assert all(len(v) <= HODLRSolver._HPOOL_MAX for v in HODLRSolver._HPOOL.values())
    assert 1e-3 not in [k[4] for k in HODLRSolver._HPOOL]            # the oldest option set went first
    # a parked handle answers like a fresh one
    a = HODLRSolver(kernel, min_size=100, tol=1e-8, seed=42)
    before = sum(len(v) for v in HODLRSolver._HPOOL.values())
    a.compute(X, yerr)
    assert sum(len(v) for v in HODLRSolver._HPOOL.values()) == before - 1
    HODLRSolver.release_pool()
    b = HODLRSolver(kernel, min_size=100, tol=1e-8, seed=42)
    b.compute(X, yerr)
    assert a.log_determinant == b.log_determinant and a.ranks() == b.ranks()

