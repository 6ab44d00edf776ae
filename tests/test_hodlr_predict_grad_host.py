"""Host-side checks of the HODLR solver's device-resident predict / likelihood gradient (gh_hodlr_predict, gh_hodlr_grad,
gh_debug_set_hodlr_strip_cols): the binding, the argument validation that needs no device, and the solver protocol that
``GP`` routes on.  The numbers are checked on the GPU in tests/test_gpu_hodlr_predict_grad.py."""
import os
import re

import numpy as np
import pytest

from george_amd import kernels, HODLRSolver
from george_amd import _native as N
from george_amd.solvers.multigpu import MultiGPUHODLRSolver

NEW = ("gh_hodlr_predict", "gh_hodlr_grad", "gh_debug_set_hodlr_strip_cols")


def test_entry_points_are_bound_and_exported():
    for name in NEW:
        assert name in N.SIGNATURES and hasattr(N.lib, name)
    # the contracts mirror the dense counterparts, argument for argument
    assert N.SIGNATURES["gh_hodlr_predict"] == N.SIGNATURES["gh_chol_predict"]
    assert N.SIGNATURES["gh_hodlr_grad"] == N.SIGNATURES["gh_chol_grad"]
    assert N.SIGNATURES["gh_debug_set_hodlr_strip_cols"] == N.SIGNATURES["gh_debug_set_hodlr_passes"]


def test_solver_protocol():
    assert callable(HODLRSolver.predict) and callable(HODLRSolver.grad)
    # what the class does not define it does not offer: GP routes on callable(getattr(solver, name, None))
    for name in ("objective", "profile", "loo", "loo_objective", "lgo", "fisher", "remove", "predict_gradient", "truncate",
                 "append", "sample_conditional"):
        assert not callable(getattr(HODLRSolver, name, None)), name
    # the tree split over several devices keeps the generic branch of GP.predict and has no fused gradient
    for name in ("predict", "grad"):
        assert not callable(getattr(MultiGPUHODLRSolver, name, None)), name


def test_null_handle_is_a_bad_argument():
    buf = np.zeros(4)
    which = np.ones(2, dtype=np.uint32)
    with pytest.raises(ValueError):
        N.check(N.lib.gh_hodlr_predict(None, None, N.ptr(buf), N.ptr(buf), 1, N.ptr(buf), None, None))
    with pytest.raises(ValueError):
        N.check(N.lib.gh_hodlr_grad(None, None, N.ptr(which), N.ptr(buf), N.ptr(buf), None, None))


def test_before_compute():
    s = HODLRSolver(1.0 * kernels.ExpSquaredKernel(1.0), tol=1e-8)
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        s.predict(s.kernel, np.zeros(3), np.zeros((2, 1)), return_var=True)
    with pytest.raises(RuntimeError, match="you must call 'compute' first"):
        s.grad(np.zeros(3), np.ones(2, dtype=np.uint32))


def test_strip_width_switch_returns_the_previous_value():
    set_cols = N.lib.gh_debug_set_hodlr_strip_cols
    first = set_cols(64)
    try:
        assert set_cols(192) == 64
        assert set_cols(0) == 192             # 0 or a negative value: the automatic choice (reported as 0)
        assert set_cols(-5) == 0
        assert set_cols(0) == 0
    finally:
        set_cols(first)


def _scratch_bytes(tu):
    """{kernel symbol: scratch bytes per lane} from the compiler's resource report the build keeps (george_amd/csrc/Makefile)"""
    path = os.path.join(os.path.dirname(N.LIB_PATH), "build", tu + ".remarks")
    assert os.path.exists(path), "%s: the build writes it (make -C george_amd/csrc)" % path
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and cur:
                out[cur] = int(m.group(1))
    return out


def test_new_kernels_use_no_scratch_memory():
    """The column reduction, the identity strip and the PMAX = 4 / 16 forms of the strip gradient reduction use no scratch (the
    evaluator's runtime-indexed arrays live in LDS there); the GH_MAX_GRAD form may use what the dense kernel of that width uses."""
    hod, kmat = {**_scratch_bytes("gh_hodlr_predict"), **_scratch_bytes("gh_hodlr_apply")}, _scratch_bytes("gh_kmat")
    shared = _scratch_bytes("gh_predict")

    def one(table, *parts):
        hits = [v for k, v in table.items() if all(p in k for p in parts)]
        assert len(hits) == 1, (parts, hits)
        return hits[0]

    for name in ("gh_colred_kernel", "gh_colfinal_kernel"):       # the reduction every solver shares: each of its instantiations
        hits = {k: v for k, v in shared.items() if name in k}
        assert hits and not any(hits.values()), (name, hits)
    assert one(hod, "hodlr_eye_strip_kernel") == 0
    assert one(hod, "hodlr_kgrad_strip_kernelILi4E") == 0
    assert one(hod, "hodlr_kgrad_strip_kernelILi16E") == 0
    assert one(hod, "hodlr_kgrad_strip_kernelILi%dE" % N.GH_MAX_GRAD) <= one(kmat, "kgrad_reduce_kernelILi%dE" % N.GH_MAX_GRAD)
