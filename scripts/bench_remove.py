"""``GP.remove`` against its two yardsticks on one MI355X: a full ``GP.compute`` of the kept points (T_full) and
``solver.dot_solve(y)`` (T_sweep), both from a build of the PARENT commit timed by a child process in the same session.

    python scripts/bench_remove.py --parent DIR [--n 4096,16384,65536] [--out profiles/remove/remove_time.json]

DIR is a built checkout of the parent commit; the child (``--only yardsticks --root DIR``) imports ``george_amd`` from it and
writes the yardsticks to a file this process reads.  Without ``--parent`` the yardsticks are measured in this build and the
output says so (``yardstick_build``).

Every remove starts from the same state: ``compute`` at N points (not timed), then ``remove`` (timed: the wall clock of the public
call, which returns after the device has finished).  Each figure is the median of ``--reps`` (>= 20) calls after ``--warmup``
(>= 3), with min and max.  ``gather_ms`` (device time of gathering the kept rows and columns into the new buffers, HIP events) comes
from a second, profiled GP, three calls, outside the timed ones.  The update is forced (``gh_debug_set_remove_path(1)``, no point
limit): the table is what the solver's routing constants are set from.

    N in (4096, 16384, 65536); removed: point 0; point N/2; point N - 200; the first 128; the first 1024; 64 scattered

Each child runs under its own ``timeout``; host threads are capped at 16.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16"))))


def data(n):
    rng = np.random.RandomState(1234)
    x = np.sort(rng.uniform(0, 10, n))
    return x, 0.1 * np.ones(n), np.sin(x)


def cases(n):
    rng = np.random.RandomState(n)
    return [("point 0", [0]), ("point N/2", [n // 2]), ("point N-200", [n - 200]), ("first 128", list(range(128))),
            ("first 1024", list(range(1024))), ("64 scattered", sorted(rng.choice(n, 64, replace=False).tolist()))]


def stats(ts):
    ts = 1e3 * np.asarray(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), reps=len(ts))


def timed(fn, warmup, reps, before=None):
    ts = []
    for i in range(warmup + reps):
        if before is not None:
            before()
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i >= warmup:
            ts.append(dt)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,16384,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full-reps", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "yardsticks"])
    ap.add_argument("--root", default=ROOT, help="where george_amd is imported from")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: the yardsticks' build")
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove", "remove_time.json"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        ap.error("a timing is the median of at least 20 calls after at least 3 warm-up calls")
    ns = [int(v) for v in a.n.split(",") if v]
    out = dict(yardstick_build="this tree" if os.path.abspath(a.root) == ROOT else os.path.basename(os.path.abspath(a.root)), rows=[])

    def emit(row=None):
        if row is not None:
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    yard = {}
    if a.parent and a.only != "yardsticks":
        # the child first: this process has not opened the device yet
        yfile = os.path.abspath(a.out) + ".yardsticks"
        cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--only", "yardsticks",
               "--root", a.parent, "--n", a.n, "--reps", str(a.reps), "--warmup", str(a.warmup), "--full-reps", str(a.full_reps),
               "--out", yfile]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit("the yardstick child ended with status %d: nothing more is started" % rc)
        with open(yfile) as f:
            prev = json.load(f)
        os.remove(yfile)
        out["yardstick_build"] = "parent commit (" + prev["yardstick_build"] + ")"
        for r in prev["rows"]:
            yard[(r["op"], r["n"], r.get("case"))] = r
            out["rows"].append(r)

    sys.path.insert(0, os.path.abspath(a.root))
    import george_amd
    from george_amd import GP, kernels
    if george_amd.device_count() <= 0:
        sys.exit("no MI355X visible: nothing is measured without one")

    for n in ns:
        x, yerr, y = data(n)
        amp = float(np.var(y))
        gp = GP(amp * kernels.ExpSquaredKernel(1.0))
        if not yard or a.only == "yardsticks":
            for name, rem in cases(n):
                keep = np.delete(np.arange(n), rem)
                xk, ek = x[keep], yerr[keep]
                r = dict(op="compute", n=n, case=name, kept=len(keep), **timed(lambda: gp.compute(xk, ek), 1, a.full_reps))
                yard[("compute", n, name)] = r
                emit(r)
            gp.compute(x, yerr)
            r = dict(op="dot_solve", n=n, case=None, **timed(lambda: gp.solver.dot_solve(y), a.warmup, a.reps))
            yard[("dot_solve", n, None)] = r
            emit(r)
        if a.only == "yardsticks":
            continue
        from george_amd import _native as N
        from george_amd import BasicSolver
        N.lib.gh_debug_set_remove_path(1)
        BasicSolver.REMOVE_MAX_POINTS, BasicSolver.REMOVE_MIN_N = 1 << 30, 0
        gpp = GP(amp * kernels.ExpSquaredKernel(1.0), profile=True)           # the gather's share only
        t_sweep = yard[("dot_solve", n, None)]["median_ms"]
        for name, rem in cases(n):
            t = timed(lambda: gp.remove(rem), a.warmup, a.reps, before=lambda: gp.compute(x, yerr))
            assert gp.solver.last_remove_path == "update" and len(gp._x) == n - len(rem)
            gather = []
            for _ in range(3):
                gpp.compute(x, yerr)
                gpp.remove(rem)
                gather.append(float(gpp.solver.profile()["ms_remove_gather"]))
            t_full = yard[("compute", n, name)]["median_ms"]
            emit(dict(op="remove", n=n, case=name, removed=len(rem), gather_ms=float(np.median(gather)), t_sweep_ms=t_sweep,
                      t_full_ms=t_full, full_over_remove=t_full / t["median_ms"], **t))
        del gp, gpp
    emit()


if __name__ == "__main__":
    main()
