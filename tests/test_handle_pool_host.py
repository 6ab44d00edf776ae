"""``HandlePool`` -- the parked native handles of a solver class -- with plain Python objects as handles and a recording
destroy function, and the solver classes' ``__del__`` on objects whose constructor never finished.  No device is touched."""
import gc
import sys

import pytest

from george_amd import kernels
from george_amd.solvers import BasicSolver, HODLRSolver, InducingSolver, VecchiaSolver
from george_amd.solvers.protocol import HandlePool


class Handle(object):
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "Handle(%r)" % (self.name,)


def _pool(*args, **kwargs):
    gone = []
    return HandlePool(gone.append, *args, **kwargs), gone


def test_take_from_an_empty_pool_or_an_unknown_key():
    pool, gone = _pool(2)
    assert pool.take("a") is None and not pool
    h = Handle(0)
    pool.park("a", h)
    assert pool.take("b") is None
    assert pool.take("a") is h and pool.take("a") is None
    assert gone == [] and isinstance(pool, dict)


def test_the_bound_of_a_key_evicts_its_oldest_handle():
    pool, gone = _pool(2)
    h = [Handle(i) for i in range(4)]
    for x in h:
        pool.park("a", x)
    assert pool["a"] == h[2:] and gone == h[:2]                        # oldest first, in the list and out of it
    assert pool.take("a") is h[3]                                      # the newest is taken first
    assert list(pool.values()) == [[h[2]]]


def test_the_total_bound_evicts_from_the_oldest_key():
    # the scenario of test_gpu_hodlr.py::test_parked_handles_are_bounded_and_reused: six option sets, three solvers each
    pool, gone = _pool(2, 4)
    made = []
    for key in range(6):
        for i in range(3):
            made.append(Handle((key, i)))
            pool.park(key, made[-1])
            assert sum(len(v) for v in pool.values()) <= 4 and all(len(v) <= 2 for v in pool.values())
    assert 0 not in pool and list(pool) == [4, 5]
    assert sum(len(v) for v in pool.values()) == 4
    parked = [x for v in pool.values() for x in v]
    assert sorted(gone + parked, key=id) == sorted(made, key=id) and len(set(map(id, gone))) == len(gone)
    # a key that is parked under again becomes the newest: the other one goes first
    pool.take(4)
    pool.park(4, Handle("again"))
    pool.park(4, Handle("and again"))
    pool.park(6, Handle("new"))
    assert list(pool) == [5, 4, 6] and [len(v) for v in pool.values()] == [1, 2, 1]


def test_an_emptied_key_disappears():
    pool, gone = _pool(2, 4)
    pool.park("a", Handle(0))
    pool.park("b", Handle(1))
    pool.take("a")
    assert list(pool) == ["b"] and "a" not in pool and pool.get("a") is None
    assert pool["a"] == [] and pool["never parked"] == [] and list(pool) == ["b"]        # (indexing reads, it does not insert)
    pool.take("b")
    assert not pool and len(pool) == 0 and gone == []


def test_admission():
    asked = []

    def refuse(h):
        asked.append(h)
        return False

    pool, gone = _pool(2, admit=refuse)
    h = Handle(0)
    pool.park("a", h)
    assert asked == [h] and gone == [h] and not pool                   # refused: destroyed, nothing parked, no empty key

    def trim(h):
        asked.append(h)
        assert not pool                                                # (asked before the handle is parked)
        h.name = "trimmed"
        return True

    del asked[:], gone[:]
    pool, gone = _pool(2, admit=trim)
    pool.park("a", h)
    assert asked == [h] and gone == [] and pool["a"] == [h] and h.name == "trimmed"


def test_release_destroys_everything_once():
    pool, gone = _pool(2, 4)
    made = [Handle(i) for i in range(4)]
    for i, h in enumerate(made):
        pool.park(i % 3, h)
    pool.release()
    assert not pool and list(pool.values()) == []
    assert sorted(gone, key=id) == sorted(made, key=id)
    pool.release()
    assert len(gone) == 4


def test_a_destroy_that_raises_does_not_stop_release():
    seen = []

    def destroy(h):
        seen.append(h)
        raise RuntimeError("no device")

    pool = HandlePool(destroy, 2)
    made = [Handle(i) for i in range(3)]
    pool.park("a", made[0])
    pool.park("a", made[1])
    pool.park("b", made[2])
    pool.release()
    assert not pool and sorted(seen, key=id) == sorted(made, key=id)
    pool.park("a", made[0])
    pool.park("a", made[1])
    pool.park("a", made[2])                                            # (nor an eviction)
    assert pool["a"] == made[1:]


def test_the_class_attributes_keep_their_values():
    assert (BasicSolver._POOL_MAX, BasicSolver._POOL_MAX_BYTES) == (2, 112 << 30)
    assert (HODLRSolver._HPOOL_MAX, HODLRSolver._HPOOL_TOTAL) == (2, 4)
    assert VecchiaSolver._HPOOL_MAX == 2 and InducingSolver._HPOOL_MAX == 2
    pools = [BasicSolver._POOL, HODLRSolver._HPOOL, VecchiaSolver._HPOOL, InducingSolver._HPOOL]
    assert all(isinstance(p, dict) for p in pools) and len(set(map(id, pools))) == 4
    for cls in (BasicSolver, HODLRSolver, VecchiaSolver, InducingSolver):
        assert callable(cls.release_pool)


def _kernel():
    return 1.0 * kernels.ExpSquaredKernel(1.0)


def _construct_and_fail(cls):
    """an object of ``cls`` whose constructor did not get to ``NativeSolver.__init__``: made, dropped and collected here"""
    if cls is VecchiaSolver:
        with pytest.raises(ValueError):
            VecchiaSolver(_kernel(), m=0)
    elif cls is InducingSolver:
        with pytest.raises(ValueError):
            InducingSolver(_kernel(), method="x")
    else:
        s = cls.__new__(cls)
        assert not hasattr(s, "_handle")
        del s
    gc.collect()


@pytest.mark.parametrize("cls", [BasicSolver, HODLRSolver, VecchiaSolver, InducingSolver], ids=lambda c: c.__name__)
def test_construct_and_drop(cls):
    pool = cls._POOL if cls is BasicSolver else cls._HPOOL
    before = {key: list(v) for key, v in pool.items()}
    unraisable = []
    old = sys.unraisablehook
    sys.unraisablehook = unraisable.append
    try:
        _construct_and_fail(cls)
    finally:
        sys.unraisablehook = old
    assert unraisable == []
    assert {key: list(v) for key, v in pool.items()} == before
