"""``NativeSolver`` -- what the solvers over the C ABI share: the reference's solver protocol
(``src/george/solvers/basic.py:25-121``) written once over a native handle the subclass owns.

The base knows no back end.  A subclass creates, parks and destroys its own handle (``_ensure_handle``) and
names the native function of each protocol call (``_SOLVE = "gh_chol_solve"`` ...); a call it cannot offer it
overrides.  Optional capabilities (``predict``, ``grad``, ``objective``, ``truncate`` ...) are methods a class
defines itself -- :class:`george_amd.GP` routes on ``callable(getattr(solver, name, None))`` -- and no solver
class inherits from another back end's class: a method that takes a native handle is only ever reachable on
the class that made the handle.
"""
import ctypes as C

import numpy as np

from .. import _native as N
from ..program import DeviceKernel

__all__ = ["NativeSolver", "rhs_matrix", "rhs_vector", "rhs_rows"]


def rhs_matrix(y, n):
    """The right-hand side of ``apply_inverse``, (n,) or (n, nrhs): ``(contiguous float64 array, nrhs)``."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim < 1 or y.ndim > 2 or y.shape[0] != n:
        raise ValueError("dimension mismatch")
    yc = np.ascontiguousarray(y)
    return yc, (1 if yc.ndim == 1 else yc.shape[1])


def rhs_vector(y, n):
    """The vector of ``dot_solve`` (and the residual of the fused calls): contiguous float64, n entries."""
    y = N.as_f64(y).reshape(-1)
    if len(y) != n:
        raise ValueError("dimension mismatch")
    return y


def rhs_rows(r, n):
    """The rows of ``apply_sqrt``, (n,) or (nrows, n): ``(contiguous float64 (nrows, n), was it one-dimensional)``."""
    r = N.as_f64(r)
    one_d = r.ndim == 1
    r2 = r.reshape(1, -1) if one_d else r
    if r2.ndim != 2 or r2.shape[1] != n:
        raise ValueError("dimension mismatch")
    return r2, one_d


class NativeSolver(object):

    # the native entry point of each protocol call: set by the subclass
    _SOLVE = _DOT_SOLVE = _GET_INVERSE = _APPLY_SQRT = None

    def __init__(self, kernel):
        self.kernel = kernel
        self._computed = False
        self._log_det = None
        self._handle = None
        self._dk = None

    # -- properties (basic.py:25-49)
    @property
    def computed(self):
        return self._computed

    @computed.setter
    def computed(self, v):
        self._computed = v

    @property
    def log_determinant(self):
        return self._log_det

    @log_determinant.setter
    def log_determinant(self, v):
        self._log_det = v

    def _need(self):
        if not self._computed or self._handle is None:
            raise RuntimeError("you must call 'compute' first")
        return self._handle

    def _check_inputs(self, x, yerr, r=None):
        """The start of a call that factors: the inputs coerced and checked (``r``: a residual, one entry per point), the
        solver no longer computed, a new device kernel.  Returns ``(x, yerr, r)``."""
        x = N.as_f64(x)
        if x.ndim != 2:
            raise ValueError("x must be (nsamples, ndim)")
        yerr = N.as_f64(np.zeros(len(x)) + yerr)
        if r is not None:
            r = rhs_vector(r, len(x))
        self._computed = False
        self._dk = DeviceKernel(self.kernel)
        if x.shape[1] != self._dk.ndim:
            raise RuntimeError("dimension mismatch")
        return x, yerr, r

    def _kernel_for(self, kernel):
        """the device kernel of ``compute`` when ``kernel`` is the solver's own, a new one otherwise"""
        return DeviceKernel(kernel) if kernel is not self.kernel else self._dk

    def _retry_without_parked_memory(self, call, ensure=None):
        """Run ``call(handle)``; on MemoryError give back what dead solvers left parked on the device
        (``_release_parked_memory``: the subclass's pools and the native block cache) and try ONCE more: a new pool key, a
        multi-GPU handle or the application's own allocations must not fail because of memory nobody uses.
        (``ensure``: where the handle comes from; the solver's own by default.)"""
        ensure = ensure or self._ensure_handle
        try:
            return call(ensure())
        except MemoryError:
            self._release_parked_memory()
            return call(ensure())

    # pickling drops the device-resident factor and flags the solver un-computed, as the reference's native solver does
    # (hodlr.py:69-76)
    def __getstate__(self):
        state = self.__dict__.copy()
        state["_handle"] = None
        state["_dk"] = None
        state["_computed"] = False
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    # -- the solver protocol
    def _solve_target(self, y, yc, in_place):
        """The ``in_place`` policy of ``apply_inverse`` for the caller's ``y`` and its contiguous form ``yc``: ``(out, back)``,
        the array the native solve writes and the array its values are then copied back to (and returned), or None.  Here:
        always a fresh array."""
        return np.empty_like(yc), None

    def apply_inverse(self, y, in_place=False):
        """basic.py:72-87 (``cho_solve``): ``y`` is (n,) or (n, nrhs)."""
        h = self._need()
        yc, nrhs = rhs_matrix(y, self._n)
        out, back = self._solve_target(y, yc, in_place)
        if nrhs > 0:
            N.check(getattr(N.lib, self._SOLVE)(h, N.ptr(yc), nrhs, N.ptr(out)))
        if back is not None:
            try:
                back[...] = out                    # honour overwrite_b for non-contiguous callers (gp.py:296-301)
                return back
            except (ValueError, TypeError):
                pass
        return out

    def dot_solve(self, y):
        """basic.py:89-102."""
        h = self._need()
        y = rhs_vector(y, self._n)
        out = C.c_double(0.0)
        N.check(getattr(N.lib, self._DOT_SOLVE)(h, N.ptr(y), C.byref(out)))
        return out.value

    def apply_sqrt(self, r):
        """basic.py:104-114: ``r @ U`` with ``U^T U = K``."""
        h = self._need()
        r2, one_d = rhs_rows(r, self._n)
        out = np.empty_like(r2)
        N.check(getattr(N.lib, self._APPLY_SQRT)(h, N.ptr(r2), r2.shape[0], N.ptr(out)))
        return out[0] if one_d else out

    def get_inverse(self):
        """basic.py:116-121."""
        h = self._need()
        out = np.empty((self._n, self._n), dtype=np.float64)
        N.check(getattr(N.lib, self._GET_INVERSE)(h, N.ptr(out)))
        return out
