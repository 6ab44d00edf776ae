"""``NativeSolver`` -- what the solvers over the C ABI share: the reference's solver protocol
(``src/george/solvers/basic.py:25-121``) and the lifetime of the native handle, both written once.

The base knows no back end.  A subclass names its native functions (``_CREATE = "gh_chol_create"``, ``_SOLVE =
"gh_chol_solve"`` ...), fills the options of a new handle (``_native_opts``) and says under which key a handle may be
shared (``_options_key``).  A protocol call without a name takes the generic route: ``get_inverse`` solves against the identity,
``apply_sqrt`` raises ``NotImplementedError``.  A solver that works in an order of its own (``VecchiaSolver``) overrides the two
order hooks ``_in`` and ``_out``; every vector of the protocol, of ``_grad`` and of ``_predict`` passes through them.

Handles of dropped solvers are parked in the class's :class:`HandlePool` (``_HPOOL``; none: the handle is destroyed with
the solver) under the key they were made with, and picked up by the next solver with that key: ``GP.compute`` makes a new
solver per call.  One mechanism, and per class a policy written as data: the bounds of the pool, an admission rule
(``BasicSolver``'s byte budget) and what ``_release_parked_memory`` gives back when the device runs out of memory.

Optional capabilities (``predict``, ``grad``, ``objective``, ``truncate`` ...) are methods a class defines itself --
:class:`george_amd.GP` routes on ``callable(getattr(solver, name, None))`` -- and no solver class inherits from another back
end's class: a method that takes a native handle is only ever reachable on the class that made the handle.
"""
import atexit
import ctypes as C

import numpy as np

from .. import _native as N
from ..program import DeviceKernel

__all__ = ["NativeSolver", "HandlePool", "rhs_matrix", "rhs_vector", "rhs_rows"]


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


class HandlePool(dict):
    """The parked native handles of one solver class: ``key -> [handle, ...]``, each list oldest first and the keys in the
    order they were last parked under, so that dict order means age; a key without handles is not kept (``pool[key]`` is then
    an empty list, as it was while the emptied lists stayed: "nothing is parked under this key").  ``destroy``: the
    name of the native function that frees a handle (or a callable).  At most ``per_key`` handles stay under one key and
    ``total`` in all (None: no bound), the oldest going first.  ``admit(handle)``, if given, is asked once before a handle
    is parked (it may shrink the handle); a handle it refuses is destroyed.  A ``destroy`` that raises is ignored: handles
    are freed from ``__del__`` and at interpreter exit, where the pool empties itself."""

    def __init__(self, destroy, per_key, total=None, admit=None):
        super(HandlePool, self).__init__()
        self._free, self.per_key, self.total, self._admit = destroy, per_key, total, admit
        atexit.register(self.release)

    def __missing__(self, key):
        return []

    def _destroy(self, h):
        try:
            (self._free if callable(self._free) else getattr(N.lib, self._free))(h)
        except Exception:
            pass

    def _evict_oldest(self, key):
        free = self[key]
        self._destroy(free.pop(0))
        if not free:
            del self[key]

    def take(self, key):
        """the newest handle parked under ``key``, or None"""
        free = self.get(key)
        if not free:
            return None
        h = free.pop()
        if not free:
            del self[key]
        return h

    def park(self, key, h):
        if self._admit is not None and not self._admit(h):
            self._destroy(h)
            return
        free = self.pop(key, [])                               # (re-inserted last: the newest key)
        free.append(h)
        self[key] = free
        if len(free) > self.per_key:
            self._evict_oldest(key)
        while self.total is not None and sum(len(v) for v in self.values()) > self.total:
            self._evict_oldest(next(iter(self)))

    def release(self):
        """destroy every parked handle (frees their device memory)"""
        while self:
            self._evict_oldest(next(iter(self)))


class NativeSolver(object):

    # the native functions of the handle's lifetime and of each protocol call: set by the subclass
    _CREATE = _DESTROY = None
    _SOLVE = _DOT_SOLVE = _GET_INVERSE = _APPLY_SQRT = None
    _NAME = None                # what error messages call the solver: the class's name unless set

    # -- lifetime: the policy of a class, as data
    _HPOOL = None               # its HandlePool; None: a handle is destroyed with its solver
    _HANDLES = ("_handle",)     # the attributes that hold a native handle; <attribute>_key remembers the key it was taken under
    _GIVES_BACK_OWN_HANDLE = True   # does _release_parked_memory destroy the solver's own handle ...
    _GIVES_BACK_POOLS = ()          # ... and which pools does it empty, before the native caches of the solver's device
    # (a pooled class keeps the options of its handle in ``self._opts``, the device ordinal under "device")

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

    def _options_key(self):
        """The options a native handle is made with, hashable: handles are shared among solvers with equal keys."""
        return None

    def _native_opts(self):
        """The filled options struct of ``_CREATE``."""
        raise NotImplementedError

    def _take_handle(self, attr, key):
        """The handle of ``attr``: as it is, else one parked under ``key``, else a new one."""
        h = getattr(self, attr, None)
        if h is None:
            h = self._HPOOL.take(key) if self._HPOOL is not None else None
            if h is None:
                o, h = self._native_opts(), N._vp()
                N.check(getattr(N.lib, self._CREATE)(C.byref(o), C.byref(h)))
            setattr(self, attr, h)
            setattr(self, attr + "_key", key)
        return h

    def _ensure_handle(self):
        return self._handle if self._handle is not None else self._take_handle("_handle", self._options_key())

    def _park_handle(self, attr="_handle"):
        """Give the handle of ``attr`` to the pool, under the key it was taken with (no pool: destroy it).  Also for an object
        whose constructor raised and at interpreter exit: nothing here fails, a native call that does is ignored."""
        h = getattr(self, attr, None)
        if h is None or not h.value:
            return
        setattr(self, attr, None)
        key, pool = getattr(self, attr + "_key", None), self._HPOOL
        try:
            if pool is None or key is None:
                getattr(N.lib, self._DESTROY)(h)
            else:
                pool.park(key, h)
        except Exception:
            pass

    def _destroy_handle(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None and h.value:
            getattr(N.lib, self._DESTROY)(h)

    def __del__(self):
        for attr in self._HANDLES:
            self._park_handle(attr)

    @classmethod
    def release_pool(cls):
        """Destroy every parked native handle (frees their device memory)."""
        if cls._HPOOL is not None:
            cls._HPOOL.release()

    def _release_parked_memory(self):
        """What ``_retry_without_parked_memory`` gives back, by the class's ``_GIVES_BACK_*``."""
        if self._GIVES_BACK_OWN_HANDLE:
            self._destroy_handle()
        for pool in self._GIVES_BACK_POOLS:
            pool.release()
        N.lib.gh_release_caches(self._opts["device"])

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
        (``_release_parked_memory``: the class's pools and the native block cache) and try ONCE more: a new pool key, a
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
    def _in(self, a):
        """A vector or matrix with one row per point, from the caller's order into the solver's.  Here: the same array."""
        return a

    def _out(self, a):
        """... and back."""
        return a

    def _solve_target(self, y, yc, in_place):
        """The ``in_place`` policy of ``apply_inverse`` for the caller's ``y`` and its contiguous form ``yc``: ``(out, back)``,
        the array the native solve writes and the array its values are then copied back to (and returned), or None.  Here:
        always a fresh array."""
        return np.empty_like(yc), None

    def apply_inverse(self, y, in_place=False):
        """basic.py:72-87 (``cho_solve``): ``y`` is (n,) or (n, nrhs)."""
        h = self._need()
        yc, nrhs = rhs_matrix(y, self._n)
        ys = self._in(yc)
        out, back = self._solve_target(y, ys, in_place)
        if nrhs > 0:
            N.check(getattr(N.lib, self._SOLVE)(h, N.ptr(ys), nrhs, N.ptr(out)))
        out = self._out(out)
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
        y = self._in(rhs_vector(y, self._n))
        out = C.c_double(0.0)
        N.check(getattr(N.lib, self._DOT_SOLVE)(h, N.ptr(y), C.byref(out)))
        return out.value

    def apply_sqrt(self, r):
        """basic.py:104-114: ``r @ U`` with ``U^T U = K``."""
        if self._APPLY_SQRT is None:
            raise NotImplementedError("apply_sqrt is not implemented for the " + (self._NAME or type(self).__name__))
        h = self._need()
        r2, one_d = rhs_rows(r, self._n)
        out = np.empty_like(r2)
        N.check(getattr(N.lib, self._APPLY_SQRT)(h, N.ptr(r2), r2.shape[0], N.ptr(out)))
        return out[0] if one_d else out

    def get_inverse(self):
        """basic.py:116-121; without a native form, ``apply_inverse`` of the identity (N^2 memory: meant for small N)."""
        h = self._need()
        if self._GET_INVERSE is None:
            return self.apply_inverse(np.eye(self._n))
        out = np.empty((self._n, self._n), dtype=np.float64)
        N.check(getattr(N.lib, self._GET_INVERSE)(h, N.ptr(out)))
        return out

    # -- the bodies of the optional ``grad`` and ``predict``, for the classes that offer them
    def _grad(self, entry, r, which):
        """``(grad over ALL kernel parameters (masked ones 0), alpha, diagA)`` from the native ``entry`` for residual ``r``."""
        h = self._need()
        r = self._in(rhs_vector(r, self._n))
        which = np.ascontiguousarray(which, dtype=np.uint32)
        g = np.zeros(max(self._dk.size, 1))
        alpha, diagA = np.empty(self._n), np.empty(self._n)
        N.check(getattr(N.lib, entry)(h, self._dk.handle, N.ptr(which), N.ptr(r), N.ptr(g), N.ptr(alpha), N.ptr(diagA)))
        return g[:self._dk.size], self._out(alpha), self._out(diagA)

    def _predict(self, entry, kernel, r, xs, return_var, return_cov):
        """``(mu, var | None, cov | None)`` at ``xs`` from the native ``entry`` for residual ``r``; ``return_var`` wins over
        ``return_cov``, and no test points make no call."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = self._in(rhs_vector(r, self._n)), N.as_f64(xs)
        want_var = bool(return_var)
        want_cov = bool(return_cov) and not want_var
        m = len(xs)
        mu = np.empty(m)
        var = np.empty(m) if want_var else None
        cov = np.empty((m, m)) if want_cov else None
        if m > 0:
            N.check(getattr(N.lib, entry)(h, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(var), N.ptr(cov)))
        return mu, var, cov
