"""The lifetime code and the protocol path the pooled solvers share (``NativeSolver`` and ``HandlePool`` in
``george_amd/solvers/protocol.py``), on the device: a dropped solver's native handle serves the next solver with the same
options and no other, ``in_place`` of the two solvers that copy back, and the residual length check of the dense solver's
fused calls.  300 points in 1-D throughout, the problem of ``test_gpu_solver_protocol.py``."""
import gc

import numpy as np
import pytest

from george_amd import BasicSolver, HODLRSolver, InducingSolver, VecchiaSolver
from test_gpu_solver_protocol import _kernel, _problem, _right_hand_sides

pytestmark = pytest.mark.gpu

N_PTS = 300

# class -> (its options, the same with one option changed: another pool key)
POOLED = {
    BasicSolver: (dict(), dict(lookahead=False)),
    HODLRSolver: (dict(min_size=32, tol=1e-8), dict(min_size=32, tol=1e-6)),
    VecchiaSolver: (dict(m=8), dict(m=9)),
    InducingSolver: (dict(inducing=16, method="fitc"), dict(inducing=16, method="dtc")),
}


@pytest.mark.parametrize("cls", list(POOLED), ids=lambda c: c.__name__)
def test_a_parked_handle_serves_the_same_options_only(cls):
    ref = _problem(N_PTS)
    same, other = POOLED[cls]
    cls.release_pool()
    a = cls(_kernel(), **same)
    a.compute(ref["x"], ref["yerr"])
    address = a._handle.value
    want = (a.log_determinant, a.dot_solve(ref["y"]))                  # (of a handle made after release_pool())
    assert address and np.all(np.isfinite(want))
    del a
    gc.collect()
    c = cls(_kernel(), **other)                                        # other options: the parked handle stays parked
    c.compute(ref["x"], ref["yerr"])
    assert c._handle.value != address
    b = cls(_kernel(), **same)
    b.compute(ref["x"], ref["yerr"])
    assert b._handle.value == address
    assert (b.log_determinant, b.dot_solve(ref["y"])) == want
    del b, c
    gc.collect()
    cls.release_pool()


def _shuffled(ref):
    """the problem's points in a fixed random order: ``(x, yerr, perm)`` with ``x = ref["x"][perm]``"""
    perm = np.random.RandomState(77).permutation(N_PTS)
    return np.ascontiguousarray(ref["x"][perm]), np.ascontiguousarray(ref["yerr"][perm]), perm


COPY_BACK = {
    "vecchia": lambda: VecchiaSolver(_kernel(), m=8, order="coordinate"),
    "inducing": lambda: InducingSolver(_kernel(), inducing=16),
}


@pytest.mark.parametrize("name", list(COPY_BACK))
def test_in_place_copies_back_into_every_writable_array(name):
    ref = _problem(N_PTS)
    x, yerr, perm = _shuffled(ref)                                     # (Vecchia's permutation is not the identity)
    s = COPY_BACK[name]()
    s.compute(x, yerr)
    if name == "vecchia":
        assert not np.array_equal(s._perm, np.arange(N_PTS))
    fresh = {}
    for rhs, (y, _) in _right_hand_sides(ref).items():
        keep = y.copy()
        out = s.apply_inverse(y)
        assert out is not y and not np.shares_memory(out, y) and np.array_equal(y, keep), rhs
        assert out.shape == y.shape and out.dtype == np.float64 and np.all(np.isfinite(out)), rhs
        back = s.apply_inverse(y, in_place=True)
        assert back is y and np.array_equal(y, out), rhs
        fresh[rhs] = out
    assert np.array_equal(fresh["fortran"], fresh["n_by_3"]) and np.array_equal(fresh["strided"], fresh["n_by_3"])
    # a read-only array: a fresh answer, the array as it was
    ro = ref["Y"].copy()
    ro.flags.writeable = False
    back = s.apply_inverse(ro, in_place=True)
    assert back is not ro and not np.shares_memory(back, ro) and back.flags.writeable
    assert np.array_equal(back, fresh["n_by_3"]) and np.array_equal(ro, ref["Y"])
    # an integer array: the values, cast
    yi = (np.arange(3 * N_PTS).reshape(N_PTS, 3) % 7 - 3).astype(np.int64)
    keep = yi.copy()
    out = s.apply_inverse(yi)
    assert out.dtype == np.float64 and np.array_equal(yi, keep)
    assert not np.array_equal(out.astype(np.int64), keep)
    back = s.apply_inverse(yi, in_place=True)
    assert back is yi and yi.dtype == np.int64 and np.array_equal(yi, out.astype(np.int64))


def test_vecchia_order_hooks_undo_the_permutation():
    """``order="coordinate"`` on shuffled points is the caller's order on the sorted points: vectors go in and come out
    through the permutation, with the same bits."""
    ref = _problem(N_PTS)
    x, yerr, perm = _shuffled(ref)
    s = VecchiaSolver(_kernel(), m=8, order="coordinate")
    s.compute(x, yerr)
    t = VecchiaSolver(_kernel(), m=8)
    t.compute(ref["x"], ref["yerr"])
    assert s.log_determinant == t.log_determinant
    assert s.dot_solve(ref["y"][perm]) == t.dot_solve(ref["y"])
    assert np.array_equal(s.apply_inverse(ref["y"][perm]), t.apply_inverse(ref["y"])[perm])
    assert np.array_equal(s.apply_inverse(ref["Y"][perm]), t.apply_inverse(ref["Y"])[perm])
    which = np.ones(len(_kernel().unfrozen_mask), dtype=np.uint32)
    (g, alpha, diagA), (g0, alpha0, diagA0) = s.grad(ref["y"][perm], which), t.grad(ref["y"], which)
    assert np.array_equal(g, g0) and np.array_equal(alpha, alpha0[perm]) and np.array_equal(diagA, diagA0[perm])
    xs = np.linspace(0.0, 10.0, 7)[:, None]
    for p, q in zip(s.predict(_kernel(), ref["y"][perm], xs, return_var=True)[:2], t.predict(_kernel(), ref["y"], xs, return_var=True)[:2]):
        assert np.array_equal(p, q)


def test_dense_fused_calls_check_the_residual_length():
    ref = _problem(N_PTS)
    s = BasicSolver(_kernel())
    s.compute(ref["x"], ref["yerr"])
    short = np.zeros(N_PTS - 1)
    with pytest.raises(ValueError, match="dimension mismatch"):
        s.grad(short, np.ones(len(_kernel().unfrozen_mask), dtype=np.uint32))
    with pytest.raises(ValueError, match="dimension mismatch"):
        s.predict(_kernel(), short, np.linspace(0.0, 10.0, 7)[:, None])
