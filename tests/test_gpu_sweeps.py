"""The dense solver's solve-side entry points -- ``apply_inverse``, ``get_inverse``, ``apply_sqrt``, ``predict`` of
``BasicSolver`` -- held element by element to the criteria of ``tests/sweep_ref.py`` (SciPy on the same matrix, residuals in
longdouble) at the smallest sizes that reach each edge of ``trsm_multi``: one tile (N = 128), exactly one super-block of 8
tiles (1024), one super-block and a tile (1152), a ragged N with a partial super-block (1300), two super-blocks and a tile
(2100), and for the single-right-hand-side chain and ``predict``'s column reduction 66 tiles (8400).  Right-hand sides and
test points cross the 128-column border of the padded width (1, 2, 127, 128, 129, 300).  Every bound is derived in
``sweep_ref.py`` and shown to pass on SciPy's answers with a headroom of 16 and more, and to fail on five kinds of subtly
wrong answers, by ``tests/test_sweep_reference.py``; none is taken from what the device gives.

A failure prints the ``Check`` that missed: its value, its bound and the 128 x 128 tile (tile row, tile column) of the worst
entry -- a far update, a clipped column range and a diagonal step go wrong in different tiles.

``apply_sqrt`` returns ``r @ U`` with ``U^T U = K``, so the unit row ``e_i`` returns ROW ``i`` of ``U``, which is exactly zero
left of column ``i``; ``K_ij`` is the product of COLUMNS ``i`` and ``j`` of ``U`` (``tests/test_sweep_reference.py::
test_rows_of_the_factor_do_not_reproduce_K``).  ``test_apply_sqrt_unit_rows`` therefore also applies all the unit rows at
once -- the identity, N rows -- and holds the columns of the result to ``|K_ij - U_:i . U_:j| <= n u |U_:i| |U_:j|`` for i, j in
the listed rows; the listed rows on their own must come back with the very bits of those rows of the identity's result
(every product is ``0 * l`` or ``1 * l`` and every sum adds zeros: exact in any order).

Measured on an MI355X, the largest over the cases of a size (u = 2^-53 = 1.11e-16).  The backward error ``eta`` against its
bound ``n u``, with SciPy's ``cho_solve`` on the same inputs beside it (``tests/test_sweep_reference.py``):

    N       device eta / u    SciPy eta / u    n u / u
    128     0.93              0.12             128
    1024    0.72              0.13             1024
    1152    1.11              0.13             1152
    1300    0.58              0.12             1300
    2100    0.80              0.12             2100
    8400    0.39 (nrhs 1)     --               8400

and value / bound of every other criterion (SciPy's inverse: 1.3e-6 .. 1.3e-5 forward, 1.7e-5 .. 2.1e-4 right residual; its
factor's gram 0.76 .. 2.25 u):

    N       apply_inverse   get_inverse   get_inverse      apply_sqrt   apply_sqrt      predict
            forward         forward       right residual   forward      gram (in u)     mu       var      cov
    128     8.6e-4          5.9e-4        7.0e-4           2.1e-4       1.2e-2 (1.6)    --       --       --
    1024    8.6e-5          6.2e-5        1.7e-4           --           --              --       --       --
    1152    1.6e-4          1.2e-4        2.0e-4           3.0e-5       3.1e-3 (3.6)    4.7e-6   1.3e-5   2.7e-5
    1300    5.8e-5          6.0e-5        1.7e-4           1.5e-5       9.5e-3 (12.4)   2.3e-6   5.4e-6   1.1e-5
    2100    8.3e-5          6.4e-5        8.9e-5           1.7e-5       3.8e-3 (7.9)    2.4e-6   7.2e-6   1.3e-5
    8400    8.3e-6          --            --               --           --              2.2e-7   7.8e-7   1.3e-6

``var`` against ``diag(cov)`` is at most 1.8e-5 of its bound; the inverse is symmetric bit for bit and nothing but zeros lies
left of the diagonal, at every size.  The device's backward error is about ten times SciPy's (it multiplies by explicit
inverses of the 128 x 128 diagonal blocks) and a thousand times and more below ``n u``: no bound is scaled by a condition
number of the blocks.
"""
import functools

import numpy as np
import pytest

import sweep_ref as R
from george_amd import BasicSolver

pytestmark = pytest.mark.gpu

SWEEP_SIZES = [n for n in R.SIZES if n <= 2100]
NRHS = [1, 2, 127, 128, 129, 300]
SOLVE_CASES = [(n, k) for n in SWEEP_SIZES for k in NRHS] + [(8400, 1)]
SQRT_SIZES = [128, 1152, 1300, 2100]
NROWS = [1, 128, 129, 200]
PREDICT_CASES = [(n, m) for n in (1152, 1300, 2100) for m in (1, 128, 129, 300)] + [(8400, 129)]


@functools.lru_cache(maxsize=None)
def _solver(n):
    """the factor of size ``n``, computed once"""
    p = R.problem(n, R.kind_of(n))
    s = BasicSolver(p.kernel)
    s.compute(p.x, p.yerr)
    return s


@pytest.fixture(scope="module", autouse=True)
def _factors_freed_afterwards():
    """the six factors (and the work arrays their handles grew) go back when the module is done"""
    yield
    _solver.cache_clear()


def _hold(what, checks):
    for c in checks:
        print("SWEEP %-28s %-30s value %.3e bound %.3e ratio %.3e  %s" % (what, c.name, c.value, c.bound, c.ratio, c.where))
    for c in checks:
        assert c.value <= c.bound, (what, c)


@pytest.mark.parametrize("n,nrhs", SOLVE_CASES, ids=["%d-%d" % c for c in SOLVE_CASES])
def test_apply_inverse(n, nrhs):
    case = R.solve_case(n, nrhs)
    b = case.B.copy()
    X = _solver(n).apply_inverse(b, in_place=False)
    assert X is not b and not np.shares_memory(X, b) and np.array_equal(b, case.B)
    _hold("apply_inverse %d x %d" % (n, nrhs), R.check_solve(case, X))


@pytest.mark.parametrize("n", SWEEP_SIZES)
def test_get_inverse(n):
    _hold("get_inverse %d" % n, R.check_inverse(R.problem(n, R.kind_of(n)), _solver(n).get_inverse()))


@pytest.mark.parametrize("n", SQRT_SIZES)
@pytest.mark.parametrize("nrows", NROWS)
def test_apply_sqrt_random_rows(n, nrows):
    case = R.sqrt_case(n, nrows)
    r = case.r.copy()
    out = _solver(n).apply_sqrt(r)
    assert np.array_equal(r, case.r)
    _hold("apply_sqrt %d rows of %d" % (nrows, n), R.check_sqrt(case, out))


@pytest.mark.parametrize("n", SQRT_SIZES)
def test_apply_sqrt_unit_rows(n):
    p = R.problem(n, R.kind_of(n))
    idx = R.unit_rows(n)
    s = _solver(n)
    eye = np.eye(n)
    rows = s.apply_sqrt(eye[idx])
    _hold("apply_sqrt unit rows of %d" % n, R.check_sqrt_units(p, idx, rows))
    one = s.apply_sqrt(eye[idx[-1]])
    assert one.shape == (n,) and np.array_equal(one, rows[-1])
    G = s.apply_sqrt(eye)
    assert np.array_equal(G[idx], rows)
    _hold("apply_sqrt identity of %d" % n, R.check_sqrt_gram(p, G, idx))


@pytest.mark.parametrize("n,m", PREDICT_CASES, ids=["%d-%d" % c for c in PREDICT_CASES])
def test_predict(n, m):
    case = R.predict_case(n, m)
    s = _solver(n)
    mu, var, cov = s.predict(case.p.kernel, case.y.copy(), case.xs.copy(), return_var=True, return_cov=True)
    _hold("predict %d at %d" % (n, m), R.check_predict(case, mu, var, cov))
