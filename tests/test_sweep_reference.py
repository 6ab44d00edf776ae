"""The criteria of ``tests/sweep_ref.py`` on the CPU, no device involved: a correct answer passes each of them with a
headroom of at least 16, a subtly wrong one fails at least one of them by a factor of at least 10.

The correct answers are SciPy's: ``cho_solve`` on the lower factor for the backward errors and the exact properties, and
-- since an answer compared with itself shows nothing -- an LU solve of the same matrix (``lu_factor`` / ``lu_solve``, another
algorithm with a backward error of its own) for the forward bounds.  ``apply_sqrt``'s product is formed a second time with
the summation order reversed.

Measured (x86-64, longdouble eps 1.08e-19; u = 2^-53), the largest over the checked columns:

    N      kind    kappa_inf  cond_2   eta / u (nrhs 1, 300)    gram / u   bound n u / u
    128    m32     209.9      98.2     0.102, 0.119             0.76       128
    1024   expsq   339.1      133.9    0.075, 0.128             1.42       1024
    1152   m32     240.4      112.4    0.080, 0.133             1.62       1152
    1300   expsq   356.3      136.9    0.086, 0.122             2.25       1300
    2100   m32     261.7      124.9    0.085, 0.119             1.78       2100

SciPy's inverse sits at 1.3e-6 .. 1.3e-5 of its forward bound and at 1.7e-5 .. 2.1e-4 of its right-residual bound.  So
the headroom is 10^3 and more everywhere.  The mutations below miss by 4e8 .. 6e12, but for (a), which the backward error
sees by a factor of 48 .. 78 and the forward bound by 6 .. 9 only, and (e), which nothing but the exact symmetry sees.

The wrong answers imitate what ``trsm_multi`` and its callers can get wrong at N = 1300 (1408 padded, 11 tiles: one super-
block of 8 and a partial one of 3) with 300 right-hand sides (three column tiles, the last one partial):

(a) one 128 x 128 tile of the solution multiplied by ``1 + 1e-9``;
(b) the solution from a factor in which an off-diagonal tile of the partial last super-block is zero (a dropped K step);
(c) the far update of the first super-block left out for columns 128 .. 255 (a clipped column range);
(d) ``apply_sqrt`` with one K tile too many for one tile of columns: the sum runs on into what lies right of the diagonal
    in the factor's storage, taken here as ``K``'s own entries;
(e) ``get_inverse`` with the tile at rows 1024 .. 1151, columns 0 .. 127 read from the transposed place of the product
    before it is mirrored, where nothing was computed: zeros.  The true entries there are below 1e-20, so only the exact
    symmetry can see it.
"""
import numpy as np
import pytest
from scipy.linalg import cho_solve, lu_factor, lu_solve, solve_triangular

import sweep_ref as R
from sweep_ref import T

CPU_SIZES = [n for n in R.SIZES if n <= 2100]      # (8400 costs SciPy several seconds: it is the GPU suite's alone)
HEADROOM = 16.0
MISS = 10.0
N_MUT, NRHS_MUT = 1300, 300


def _passes(checks):
    for c in checks:
        assert c.ratio * HEADROOM <= 1.0, c


def _fails(checks):
    worst = max(checks, key=lambda c: c.ratio)
    assert worst.ratio >= MISS, checks
    return worst


@pytest.fixture(scope="module")
def lu():
    made = {}

    def get(n):
        if n not in made:
            made[n] = lu_factor(R.problem(n, R.kind_of(n)).K)
        return made[n]
    return get


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


def test_checked_cols_reach_every_tile():
    for ncols in (1, 2, 127, 128, 129, 300, 1300, 2100):
        cols = R.checked_cols(ncols)
        assert cols[0] == 0 and cols[-1] == ncols - 1 and len(set(cols)) == len(cols)
        assert {c // T for c in cols} == set(range(-(-ncols // T)))
        for b in range(T, ncols, T):
            assert b - 1 in cols and b in cols


def test_kinds_alternate_and_condition_is_flat():
    assert [R.kind_of(n) for n in R.SIZES] == ["m32", "expsq"] * 3
    for n in CPU_SIZES:
        p = R.problem(n, R.kind_of(n))
        assert 50.0 < p.kappa < 1000.0, (n, p.kappa)
        assert not p.K.flags.writeable and not p.L.flags.writeable and not p.Kinv.flags.writeable


@pytest.mark.parametrize("n", CPU_SIZES)
@pytest.mark.parametrize("nrhs", [1, 129, 300])
def test_scipy_solve_passes(n, nrhs, lu):
    case = R.solve_case(n, nrhs)
    _passes(R.check_solve(case, case.X))                       # the backward error of cho_solve
    _passes(R.check_solve(case, lu_solve(lu(n), case.B)))      # ... and of another algorithm, within the forward bound


@pytest.mark.parametrize("n", CPU_SIZES)
def test_scipy_inverse_passes(n, lu):
    p = R.problem(n, R.kind_of(n))
    for X in (p.Kinv, lu_solve(lu(n), np.eye(n))):
        X = np.tril(X) + np.tril(X, -1).T                      # (one triangle mirrored, as the device does)
        _passes(R.check_inverse(p, X))


@pytest.mark.parametrize("n", [128, 1152, 1300, 2100])
def test_scipy_sqrt_passes(n):
    p = R.problem(n, R.kind_of(n))
    for nrows in (1, 200):
        case = R.sqrt_case(n, nrows)
        _passes(R.check_sqrt(case, np.dot(case.r[:, ::-1], p.L.T[::-1])))
    idx = R.unit_rows(n)
    assert idx == [i for i in (0, 127, 128, 1023, 1024) if i < n - 1] + [n - 1]
    _passes(R.check_sqrt_units(p, idx, np.dot(np.eye(n)[idx], p.L.T)))
    _passes(R.check_sqrt_gram(p, p.L.T, idx))


def test_rows_of_the_factor_do_not_reproduce_K():
    """why check_sqrt_gram takes the columns of ``U``: ``e_i @ U`` is a ROW of ``U``, and ``(U U^T)_ij`` is not ``K_ij``"""
    p = R.problem(1152, R.kind_of(1152))
    Uf = p.L.T
    assert abs(np.dot(Uf[1151], Uf[1151]) - p.K[1151, 1151]) > 0.1 * p.K[1151, 1151]
    assert abs(np.dot(Uf[:, 1151], Uf[:, 1151]) - p.K[1151, 1151]) <= 1152 * R.U * p.K[1151, 1151]


@pytest.mark.parametrize("n,m", [(1152, 1), (1300, 129), (2100, 300)])
def test_scipy_predict_passes(n, m, lu):
    case = R.predict_case(n, m)
    p = case.p
    from oracle import kernels_np
    Ks = kernels_np.value_general(p.kernel, case.xs, p.x)
    Kss = kernels_np.value_general(p.kernel, case.xs, case.xs)
    cov = Kss - np.dot(Ks, lu_solve(lu(n), Ks.T))
    _passes(R.check_predict(case, np.dot(Ks, lu_solve(lu(n), case.y)), np.diag(cov).copy(), cov))


# ---------------------------------------------------------------- the mutations
@pytest.fixture(scope="module")
def mut():
    return R.solve_case(N_MUT, NRHS_MUT)


def test_mutation_a_one_tile_scaled(mut):
    for ti, tj in ((0, 0), (9, 1), (10, 2), (4, 2)):
        X = mut.X.copy()
        X[ti * T:(ti + 1) * T, tj * T:(tj + 1) * T] *= 1.0 + 1e-9
        worst = _fails(R.check_solve(mut, X))
        assert "tile column %d " % tj in worst.where, worst


def test_mutation_b_dropped_tile_of_the_factor(mut):
    L = mut.p.L.copy()
    L[9 * T:10 * T, 8 * T:9 * T] = 0.0
    _fails(R.check_solve(mut, cho_solve((L, True), mut.B)))


def test_mutation_c_far_update_clipped_to_some_columns(mut):
    L, B = mut.p.L, mut.B
    top = R.SB * T                                             # rows of the first super-block: 1024
    Z = np.empty_like(B)
    Z[:top] = solve_triangular(L[:top, :top], B[:top], lower=True)
    low = B[top:] - np.dot(L[top:, :top], Z[:top])
    good = solve_triangular(L[top:, top:], low, lower=True)
    low[:, T:2 * T] = B[top:, T:2 * T]                         # the update of everything below never reached these columns
    Z[top:] = solve_triangular(L[top:, top:], low, lower=True)
    full = Z.copy()
    full[top:] = good
    _passes(R.check_solve(mut, solve_triangular(L, full, lower=True, trans="T")))       # (the blocked sweep itself is right)
    worst = _fails(R.check_solve(mut, solve_triangular(L, Z, lower=True, trans="T")))
    assert "tile column 1 " in worst.where, worst


def test_mutation_d_sqrt_one_k_tile_too_many():
    p = R.problem(N_MUT, R.kind_of(N_MUT))
    idx = R.unit_rows(N_MUT)

    def wrong(r, tj):
        out = np.dot(r, p.L.T)
        out[:, tj * T:(tj + 1) * T] += np.dot(r[:, (tj + 1) * T:(tj + 2) * T], p.K[tj * T:(tj + 1) * T, (tj + 1) * T:(tj + 2) * T].T)
        return out
    for tj in (0, 3, 9):
        for nrows in (1, 200):
            case = R.sqrt_case(N_MUT, nrows)
            _fails(R.check_sqrt(case, wrong(case.r, tj)))
    # the unit row 128 lies in the K tile that column tile 0 must not reach: its entries left of the diagonal show it
    checks = R.check_sqrt_units(p, idx, wrong(np.eye(N_MUT)[idx], 0))
    assert checks[0].name.startswith("non-zeros left") and checks[0].ratio == np.inf, checks
    checks = R.check_sqrt_gram(p, wrong(np.eye(N_MUT), 0), idx)
    assert checks[0].ratio == np.inf and checks[1].ratio >= MISS, checks


def test_mutation_e_inverse_tile_from_the_unmirrored_place():
    p = R.problem(N_MUT, R.kind_of(N_MUT))
    product = np.tril(p.Kinv)                                  # the product as it is formed: lower triangle only
    X = product + np.tril(product, -1).T
    _passes(R.check_inverse(p, X))
    assert 0.0 < np.max(np.abs(X[8 * T:9 * T, :T])) < 1e-20
    X[8 * T:9 * T, :T] = product[:T, 8 * T:9 * T].T
    worst = _fails(R.check_inverse(p, X))
    assert worst.name == "asymmetric entries" and "tile row" in worst.where, worst
    # a tile next to the diagonal, where the entries are not small, fails the forward bound and the residual as well
    X = product + np.tril(product, -1).T
    X[9 * T:10 * T, 8 * T:9 * T] = product[8 * T:9 * T, 9 * T:10 * T].T
    assert sum(c.ratio >= MISS for c in R.check_inverse(p, X)) == 3
