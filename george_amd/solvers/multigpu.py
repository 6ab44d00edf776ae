"""``MultiGPUSolver`` -- the dense solver on several MI355X of ONE process, behind the C ABI.

``GP(kernel, solver=MultiGPUSolver, devices=[0, 1, 2, 3, 4, 5, 6, 7])`` shards the factorisation of
``BasicSolver`` (reference ``src/george/solvers/basic.py:51-121``) block-cyclically over the listed
devices (``gh_mgpu_*``, george_amd/csrc/gh_mgpu.hip: one host thread per device, RCCL over xGMI;
default grid ``len(devices) x 1``: whole tile rows per device in snake order).  The whole solver
protocol: ``compute`` / ``log_determinant`` / ``computed`` / ``dot_solve`` / ``apply_inverse`` /
``apply_sqrt`` / ``get_inverse``, plus the device-resident ``predict`` of ``george_amd.GP`` -- every
O(N^2 R) operation is a tile sweep on the sharded factor with all its right-hand sides together.  The
multi-PROCESS form (one rank per GPU under torch.distributed) is
``george_amd.distributed.DistributedBasicSolver``.
"""
import ctypes as C

import numpy as np

from .. import _native as N
from .protocol import NativeSolver, rhs_vector

__all__ = ["MultiGPUSolver", "MultiGPUHODLRSolver"]


class _MultiDeviceSolver(NativeSolver):
    """What the two solvers over several devices of one process share: the device list, a handle made on first use
    from the subclass's ``_split_opts()`` and destroyed with the solver (no pool), ``compute`` around one native call,
    an ``in_place`` that copies back, and NativeSolver's pickle without the factor."""

    _COMPUTE = None

    def __init__(self, kernel, devices):
        super(_MultiDeviceSolver, self).__init__(kernel)
        self.devices = [int(d) for d in devices]
        if not 1 <= len(self.devices) <= 16:
            raise ValueError("devices must list 1..16 device ordinals")

    def _native_opts(self):
        o = self._split_opts()
        o.n_dev = len(self.devices)
        for i, d in enumerate(self.devices):
            o.devices[i] = d
        return o

    def _compute(self, x, yerr):
        """``compute`` up to the ``computed`` flag, which the subclass sets; returns the coerced ``x``"""
        x, yerr, _ = self._check_inputs(x, yerr)
        h = self._ensure_handle()
        logdet = C.c_double(0.0)
        N.check(getattr(N.lib, self._COMPUTE)(h, self._dk.handle, N.ptr(x), len(x), x.shape[1], N.ptr(yerr), C.byref(logdet)))
        self._n = len(x)
        self.log_determinant = logdet.value
        return x

    def _solve_target(self, y, yc, in_place):
        """``in_place``: the values are copied back into the caller's float64 array"""
        return np.empty_like(yc), (y if in_place and isinstance(y, np.ndarray) and y.dtype == np.float64 else None)


class MultiGPUSolver(_MultiDeviceSolver):

    _CREATE, _DESTROY, _COMPUTE = "gh_mgpu_create", "gh_mgpu_destroy", "gh_mgpu_compute"
    _SOLVE, _DOT_SOLVE, _GET_INVERSE, _APPLY_SQRT = "gh_mgpu_solve", "gh_mgpu_dot_solve", "gh_mgpu_get_inverse", "gh_mgpu_apply_sqrt"

    def __init__(self, kernel, devices=None, nb=0, grid=None, transport="rccl", plain_cyclic=False, chain_only=False, trace=False,
                 one_comm=False):
        if devices is None:
            devices = list(range(max(int(N.lib.gh_device_count()), 1)))
        super(MultiGPUSolver, self).__init__(kernel, devices)
        if transport not in ("rccl", "copy"):
            raise ValueError("transport must be 'rccl' or 'copy'")
        self.nb = int(nb)
        self.grid = tuple(grid) if grid is not None else (0, 0)
        self.transport = transport
        self.flags = ((N.GH_MGPU_PLAIN_CYCLIC if plain_cyclic else 0) | (N.GH_MGPU_CHAIN_ONLY if chain_only else 0) |
                      (N.GH_MGPU_TRACE if trace else 0) | (N.GH_MGPU_ONE_COMM if one_comm else 0))

    def _split_opts(self):
        o = N.gh_mgpu_opts()
        o.pr, o.pc = int(self.grid[0]), int(self.grid[1])
        o.nb = self.nb
        o.transport = N.GH_MGPU_RCCL if self.transport == "rccl" else N.GH_MGPU_COPY
        o.flags = self.flags
        return o

    def grid_shape(self):
        pr, pc, nb = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        N.check(N.lib.gh_mgpu_grid(self._ensure_handle(), C.byref(pr), C.byref(pc), C.byref(nb)))
        return pr.value, pc.value, nb.value

    def comm_mode(self):
        """2: chain and bulk gather on their own RCCL communicators; 1: one communicator (``one_comm=True``, or chosen by
        gh_mgpu_create because two streams of a rank did not dispatch independently); 0: transport "copy" """
        return int(N.lib.gh_mgpu_comm_mode(self._ensure_handle()))

    def compute(self, x, yerr):
        """basic.py:51-70.  ``yerr`` already contains the white noise (gp.py:330)."""
        self._x_host = self._compute(x, yerr)
        self.computed = not (self.flags & N.GH_MGPU_CHAIN_ONLY)       # (a chain-only run is a timing aid: nothing to solve with)

    def owner(self, tile_row, tile_col):
        """rank (index into ``devices``) that holds tile (I, J)"""
        return int(N.lib.gh_mgpu_owner(self._ensure_handle(), int(tile_row), int(tile_col)))

    def trace(self):
        """``trace=True``: array of (rank, step, phase, milliseconds, flops or bytes) rows of the last compute()
        (phases: include/george_amd.h, gh_mgpu_get_trace)"""
        h = self._ensure_handle()
        cnt = C.c_int64(0)
        N.check(N.lib.gh_mgpu_get_trace(h, None, 0, C.byref(cnt)))
        out = np.zeros((max(cnt.value, 1), 5))
        N.check(N.lib.gh_mgpu_get_trace(h, N.ptr(out), cnt.value, C.byref(cnt)))
        return out[:cnt.value]

    def predict(self, kernel, r, xs, return_var=False, return_cov=False):
        """mean / variance / covariance terms of gp.py:532-545 on the sharded factor (as ``BasicSolver.predict``)."""
        h = self._need()
        dk = self._kernel_for(kernel)
        r, xs = rhs_vector(r, self._n), N.as_f64(xs)
        m = len(xs)
        mu = np.empty(m)
        var = np.empty(m) if return_var else None
        if return_cov and m > 2048:
            # the device call offers the full covariance up to 2048 test points: beyond it, the mean from the device and
            # gp.py:543-545 as written, on the sharded solves
            N.check(N.lib.gh_mgpu_predict(h, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), None, None))
            Kxs = kernel.get_value(xs, self._x_host)
            cov = kernel.get_value(xs) - np.dot(Kxs, self.apply_inverse(np.ascontiguousarray(Kxs.T)))
            if var is not None:
                var[:] = np.diag(cov)
            return mu, var, cov
        cov = np.empty((m, m)) if return_cov else None
        N.check(N.lib.gh_mgpu_predict(h, dk.handle, N.ptr(r), N.ptr(xs), m, N.ptr(mu), N.ptr(var), N.ptr(cov)))
        return mu, var, cov


class MultiGPUHODLRSolver(_MultiDeviceSolver):
    """The HODLR solver with its tree split over several MI355X of one process (``gh_hodlr_mgpu_*``,
    george_amd/csrc/gh_hodlr_mgpu.hip): the top log2(len(devices)) levels are shared, each device owns one
    sub-tree.  Same keywords as ``HODLRSolver`` (reference ``src/george/solvers/hodlr.py:13-76``:
    ``min_size=100, tol=0.1, seed=42``) plus ``devices``; same node-by-node random streams as the
    single-GPU solver, so ranks and answers agree with it to rounding.  ``len(devices)`` must be a power
    of two and ``N / len(devices) >= 2 * min_size``.  ``apply_sqrt`` raises ``NotImplementedError``
    (hodlr.py:62-64); pickling drops the factor (:69-76).  The device-resident ``predict`` / ``grad`` of the
    single-GPU ``HODLRSolver`` (``gh_hodlr_predict`` / ``gh_hodlr_grad``) are not offered on the split: the class
    defines neither, so ``GP`` takes its generic branch on ``apply_inverse`` / ``get_inverse`` here."""

    _CREATE, _DESTROY, _COMPUTE = "gh_hodlr_mgpu_create", "gh_hodlr_mgpu_destroy", "gh_hodlr_mgpu_compute"
    # (no native get_inverse: hodlr.h / _hodlr.cpp:194-199 solve against the identity, and so does the base)
    _SOLVE, _DOT_SOLVE = "gh_hodlr_mgpu_solve", "gh_hodlr_mgpu_dot_solve"
    _NAME = "HODLRSolver"

    def __init__(self, kernel, min_size=100, tol=0.1, seed=42, devices=None, max_rank=0):
        if devices is None:                                  # all visible devices, cut down to a power of two (3, 6, 7 GPUs: 2, 4, 4)
            have = max(int(N.lib.gh_device_count()), 1)
            devices = list(range(1 << (min(have, 16).bit_length() - 1)))
        super(MultiGPUHODLRSolver, self).__init__(kernel, devices)
        n = len(self.devices)
        if n & (n - 1):
            raise ValueError("the HODLR tree is split over 1, 2, 4, 8 or 16 devices (got %d)" % n)
        self.min_size, self.tol, self.seed, self.max_rank = min_size, tol, seed, int(max_rank)

    def _split_opts(self):
        o = N.gh_hodlr_mgpu_opts()
        o.min_size, o.seed, o.max_rank, o.tol = int(self.min_size), int(self.seed), self.max_rank, float(self.tol)
        return o

    def _options_key(self):
        """(no pool: what ``compute`` compares to see that the options were changed on the instance)"""
        return (tuple(self.devices), int(self.min_size), int(self.seed), self.max_rank, float(self.tol))

    def grid_shape(self):
        raise NotImplementedError("the HODLR split has no process grid: see rows()")

    def compute(self, x, yerr):
        """hodlr.h:75-103 over the split tree.  ``yerr`` already contains the white noise (gp.py:330)."""
        if self._handle is not None and self._handle_key != self._options_key():
            self._destroy_handle()                             # options were changed on the instance
        self._compute(x, yerr)
        self.computed = True

    def rows(self):
        """[(first row, number of rows)] of every device's sub-tree (after compute())."""
        n = len(self.devices)
        r0, nr = (C.c_int64 * n)(), (C.c_int64 * n)()
        N.check(N.lib.gh_hodlr_mgpu_rows(self._need(), r0, nr))
        return [(int(r0[i]), int(nr[i])) for i in range(n)]

    def ranks(self):
        """ACA ranks of all internal nodes, level by level, left to right (as ``HODLRSolver.ranks()``)."""
        h = self._need()
        cap = 1 << 16
        buf, cnt = (C.c_int32 * cap)(), C.c_int32(0)
        N.check(N.lib.gh_hodlr_mgpu_ranks(h, buf, cap, C.byref(cnt)))
        return [int(buf[i]) for i in range(cnt.value)]
