"""compute()+log_likelihood() (bench.DenseJob, inputs resident) with the one-level and the two-level trailing update in ONE process
(gh_debug_set_update_group / gh_debug_set_update_hide): per size the best and median step of every arm, the groups the rule
forms, and the log-likelihood, which must be identical bit for bit.
python scripts/dev/two_level_ab.py [sizes]      ARMS="1:0,0:0" (gmax:hide; 1 = one-level, 0 = the default)  STEPS=8  ROUNDS=2"""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from george_amd import _native as N  # noqa: E402
import torch  # noqa: E402

ARMS = [(int(a.split(":")[0]), float(a.split(":")[1])) for a in os.environ.get("ARMS", "1:0,0:0").split(",")]
STEPS, ROUNDS = int(os.environ.get("STEPS", "8")), int(os.environ.get("ROUNDS", "2"))
sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [65536, 49152, 32768, 24576]


def groups(n, arm):
    prev_g, prev_h = N.lib.gh_debug_set_update_group(arm[0]), N.lib.gh_debug_set_update_hide(arm[1])
    gmax, hide = N.lib.gh_debug_set_update_group(prev_g), N.lib.gh_debug_set_update_hide(prev_h)      # (what 0 stands for)
    np_ = (n + 127) // 128 * 128
    ns, no, ne = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    N.check(N.lib.gh_debug_chol_plan(np_, 1024, 25600, gmax, hide, None, 0, C.byref(ns), None, 0, C.byref(no), C.byref(ne)))
    ops = (C.c_int64 * (no.value * 12))()
    N.check(N.lib.gh_debug_chol_plan(np_, 1024, 25600, gmax, hide, None, 0, C.byref(ns), ops, no.value, C.byref(no), C.byref(ne)))
    sizes_, cur = [], 0
    for i in range(no.value):
        cur += ops[12 * i] == 0
        if ops[12 * i] in (2, 4):
            sizes_.append(cur); cur = 0
    while len(sizes_) > 1 and sizes_[-1] == 1 and sizes_[-2] == 1:
        sizes_.pop()
    return gmax, hide, " ".join(str(v) for v in sizes_) + " 1 ..."


print("| N | gmax | hide | groups | ms min / median / max | against the first arm (median) | log-likelihood |\n|---|---|---|---|---|---|---|")
try:
    for n in sizes:
        res = {}
        for rnd in range(ROUNDS):
            for arm in ARMS:
                N.lib.gh_debug_set_update_group(arm[0]); N.lib.gh_debug_set_update_hide(arm[1])
                job = bench.DenseJob(n, 0, 0, profile=False)
                ts = []
                for rep in range(2 + (STEPS + ROUNDS - 1) // ROUNDS):
                    torch.cuda.synchronize(); t0 = time.perf_counter(); v = job.step(); torch.cuda.synchronize()
                    if rep >= 2: ts.append((time.perf_counter() - t0) * 1e3)
                res.setdefault(arm, []).extend(ts); res[(arm, "ll")] = float(v)
                job.close()
        base = float(np.median(res[ARMS[0]]))
        for arm in ARMS:
            assert res[(arm, "ll")] == res[(ARMS[0], "ll")], (n, arm, res[(arm, "ll")], res[(ARMS[0], "ll")])
            gmax, hide, gs = groups(n, arm)
            t = res[arm]
            print("| %d | %d | %g | %s | %.2f / %.2f / %.2f | %+.2f %% | %.17g |" % (
                n, gmax, hide, gs if gmax > 1 else "one-level", min(t), float(np.median(t)), max(t), (float(np.median(t)) / base - 1) * 100,
                res[(arm, "ll")]), flush=True)
finally:
    N.lib.gh_debug_set_update_group(0); N.lib.gh_debug_set_update_hide(0.0)
