"""The two-level dense Cholesky driver (gh_chol.hip, factor_two_level; launch list: gh_chol_plan.h): groups of consecutive inner
panels are applied to the matrix behind them in one launch of K = the group's width.  Every element still receives the same
k-steps in the same ascending order, so the factor is IDENTICAL to the one-level driver's, bit for bit, whatever the groups."""
import ctypes as C

import numpy as np
import pytest

import zoo
from george_amd import kernels, BasicSolver
from george_amd import _native as N

pytestmark = pytest.mark.gpu

# (group maximum, margin of the group rule).  0, 0 = the library's defaults: at these sizes single panels or a few groups of
# two, through the two-level driver; a margin of 12 gives groups that grow to the maximum and are cut back again (asserted
# below from the plan itself); 1e12 groups of the maximum up to the end.
MODES = [(1, 0.0), (0, 0.0), (2, 12.0), (4, 12.0), (8, 12.0), (8, 1e12)]


def _set(mode):
    N.lib.gh_debug_set_update_group(mode[0])
    N.lib.gh_debug_set_update_hide(mode[1])


def _groups(np_, nb, bound, gmax, hide):
    ns, no, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    N.check(N.lib.gh_debug_chol_plan(np_, nb, bound, gmax, hide, None, 0, C.byref(ns), None, 0, C.byref(no), C.byref(ne)))
    ops = (C.c_int64 * (no.value * 12))()
    N.check(N.lib.gh_debug_chol_plan(np_, nb, bound, gmax, hide, None, 0, C.byref(ns), ops, no.value, C.byref(no), C.byref(ne)))
    sizes, cur = [], 0
    for i in range(no.value):
        kind = ops[12 * i]
        cur += kind == 0
        if kind in (2, 4):
            sizes.append(cur); cur = 0
    return sizes


def _factor(s):
    old = BasicSolver.PICKLE_FACTOR_MAX_N
    BasicSolver.PICKLE_FACTOR_MAX_N = None
    try:
        return s.__getstate__()["_factor_state"]             # gh_chol_export_factor: (packed lower triangle, diagonal-block inverses)
    finally:
        BasicSolver.PICKLE_FACTOR_MAX_N = old


@pytest.mark.parametrize("n,nb", [(30000, 0), (24576 + 300, 512), (24576 + 300, 1024)])
def test_every_group_maximum_gives_the_same_bits(n, nb):
    """N = 30000 with the solver's own widths: wide panels, then 1024s, a ragged end; N = 24876 with 512- and 1024-column panels:
    49 and 25 panels, groups of 4 and 8 and their cut-back.  Factor, diagonal-block inverses, log-determinant, quadratic form
    and alpha are compared bit for bit against the one-level driver; a second compute() on the same handle; profile on and off."""
    np_ = (n + 127) // 128 * 128
    plans = {m: _groups(np_, nb or 1024, 0 if nb else 25600, m[0], m[1]) for m in MODES if m[0] > 1}
    print(n, nb, plans)
    # what the modes are there for: groups of 4 and of 8 occur, and groups that grew are cut back again before the end
    assert max(plans[(4, 12.0)]) == 4 and max(plans[(8, 1e12)]) == 8
    for m in ((4, 12.0), (8, 12.0)):
        assert plans[m][-1] == 1 and len(set(plans[m])) >= 3 and max(plans[m]) >= 4
    x, yerr, y = zoo.bench_data(n)
    kernel = np.var(y) * kernels.ExpSquaredKernel(1.0)
    ref = None
    try:
        for mode in MODES:
            for profile in ((False, True) if mode[:2] == (4, 12.0) else (False,)):
                _set(mode)
                s = BasicSolver(kernel, nb=nb, profile=profile)
                s.compute(x[:, None], yerr)
                got = (s.log_determinant, s.dot_solve(y), s.apply_inverse(y)) + _factor(s)
                s.compute(x[:, None], yerr)                  # the handle's plan and events are re-used
                assert (s.log_determinant, s.dot_solve(y)) == got[:2]
                if profile:
                    p = N.gh_chol_profile()
                    N.check(N.lib.gh_chol_get_profile(s._handle, C.byref(p)))
                    # the far launches are a part of the update launches, and all of them together do the flops of the factorisation
                    # that are not inside a panel: lower tiles only, each k once (within the tiles the trapezoids round up to)
                    assert p.n_trailing >= 1 and p.update_flops > p.trailing_flops > 0 and p.ms_update_union >= p.ms_trailing * 0.5 > 0
                    assert 0.8 * np_ ** 3 / 3 < p.update_flops < 1.1 * np_ ** 3 / 3
                del s
                if ref is None:
                    ref = got
                    continue
                assert got[0] == ref[0] and got[1] == ref[1], (mode, got[:2], ref[:2])
                for q in (2, 3, 4):
                    assert np.array_equal(got[q], ref[q]), (mode, profile, q)
                del got
    finally:
        _set((0, 0.0))


def test_not_positive_definite_gives_the_same_info_in_every_mode():
    """the rank-2 CosineKernel without noise, at a size that takes the new driver: LinAlgError and the same failing pivot"""
    n = 24576 + 300
    k = kernels.CosineKernel(log_period=0.0)
    x = np.linspace(0, 3, n)
    infos = []
    try:
        for mode in MODES:
            _set(mode)
            s = BasicSolver(k)
            with pytest.raises(np.linalg.LinAlgError):
                s.compute(x[:, None], np.zeros(n))
            infos.append(int(N.lib.gh_chol_info(s._handle)))
            del s
    finally:
        _set((0, 0.0))
    print(infos)
    assert infos[0] > 0 and len(set(infos)) == 1
