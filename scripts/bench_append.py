"""``GP.append`` against its two yardsticks on one MI355X: a full ``GP.compute`` of the concatenated data (T_full), and
``solver.dot_solve(y)`` (T_sweep) -- one chained sweep over the same 4 N^2 bytes of factor plus a reduction and a
synchronisation.

The yardsticks are taken with profiling off, and may come from another build of the package: ``--only yardsticks --root DIR``
imports ``george_amd`` from DIR (a checkout of the parent commit, built) and writes them to ``--out``; the append run reads them
with ``--yardsticks FILE``.  Without ``--yardsticks`` they are measured in this build, in the same process, first.  The output
says which (``yardstick_build``).

Every append starts from the same state: ``compute`` once at n points, then per sample ``append(m points)`` (timed: the wall
clock of the public call, which returns after the device has finished) and ``truncate(n)`` (not timed).  Each figure is the
median of ``--reps`` (>= 20) calls after ``--warmup`` (>= 3) calls, with the spread (min .. max).  The relayout's share
(``relayout_ms``: device time of moving the factor into buffers of a larger Np, HIP events) comes from a second GP with
``profile=True``, five appends, outside the timed calls.  ``T_full`` is the median of ``--full-reps`` calls.

    N in (4096, 16384, 65536); m in (1, 4, 128, 1024); n = N (n = 0 mod 128) and n = N - 64 (n = 64 mod 128)

The conditions at N = 65536 (``conditions`` in the output): m <= 4 without a tile crossing: append <= 2 T_sweep; m = 128:
append <= T_full / 20; m = 1024: append <= T_full / 5.  The smaller N are recorded only.

    python scripts/bench_append.py [--n 4096,16384,65536] [--m 1,4,128,1024] [--paths 0] [--chain-max-m 128]
                                   [--only yardsticks|append] [--root DIR] [--yardsticks FILE] [--out profiles/append/append_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def data(n):
    rng = np.random.RandomState(1234)
    x = np.sort(rng.uniform(0, 10, n))
    return x, 0.1 * np.ones(n), np.sin(x)


def stats(ts):
    ts = 1e3 * np.asarray(ts)
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), reps=len(ts))


def timed(fn, warmup, reps, after=None):
    ts = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if after is not None:
            after()
        if i >= warmup:
            ts.append(dt)
    return stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,16384,65536")
    ap.add_argument("--m", default="1,4,128,1024")
    ap.add_argument("--paths", default="0", help="gh_debug_set_append_path values to measure (0: the library's rule)")
    ap.add_argument("--chain-max-m", type=int, default=128, help="paths 1 and 2 (a sweep per 1 / 4 rows) are not timed above this m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full-reps", type=int, default=5)
    ap.add_argument("--only", default="", choices=["", "yardsticks", "append"])
    ap.add_argument("--root", default=ROOT, help="where george_amd is imported from")
    ap.add_argument("--build", default=None, help="what to call that build in the output (default: 'this tree' / the --root path)")
    ap.add_argument("--yardsticks", default=None, help="a file written by --only yardsticks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append", "append_time.json"))
    a = ap.parse_args()
    if a.reps < 20 or a.warmup < 3:
        ap.error("a timing is the median of at least 20 calls after at least 3 warm-up calls")
    sys.path.insert(0, os.path.abspath(a.root))
    import george_amd
    from george_amd import GP, kernels
    if george_amd.device_count() <= 0:
        sys.exit("no MI355X visible: nothing is measured without one")
    build = a.build or ("this tree" if os.path.abspath(a.root) == ROOT else a.root)
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ms, paths = ints(a.m), ints(a.paths)
    out = dict(yardstick_build=build, rows=[], conditions=[])
    yard = {}
    if a.yardsticks:
        with open(a.yardsticks) as f:
            prev = json.load(f)
        out["yardstick_build"] = prev["yardstick_build"]
        for r in prev["rows"]:
            if r["op"] in ("compute", "dot_solve"):
                yard[(r["op"], r["n"])] = r
                out["rows"].append(r)

    def emit(row=None):
        if row is not None:
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)

    for n_big in ints(a.n):
        x, yerr, y = data(n_big + max(ms))
        amp = float(np.var(y[:n_big]))
        gp = GP(amp * kernels.ExpSquaredKernel(1.0))
        # ---- yardsticks (profiling off)
        if a.only != "append" and not a.yardsticks:
            for m in sorted(set(ms)):
                r = dict(op="compute", n=n_big + m, **timed(lambda: gp.compute(x[:n_big + m], yerr[:n_big + m]), 1, a.full_reps))
                yard[("compute", n_big + m)] = r
                emit(r)
            gp.compute(x[:n_big], yerr[:n_big])
            r = dict(op="dot_solve", n=n_big, **timed(lambda: gp.solver.dot_solve(y[:n_big]), a.warmup, a.reps))
            yard[("dot_solve", n_big)] = r
            emit(r)
        if a.only == "yardsticks":
            continue
        from george_amd import _native as N
        t_sweep = yard[("dot_solve", n_big)]["median_ms"]
        gpp = GP(amp * kernels.ExpSquaredKernel(1.0), profile=True)          # the relayout's share only
        # ---- append
        for n in (n_big, n_big - 64):
            gp.compute(x[:n], yerr[:n])
            gpp.compute(x[:n], yerr[:n])
            for path in paths:
                N.lib.gh_debug_set_append_path(path)
                try:
                    for m in ms:
                        if path in (1, 2) and m > a.chain_max_m:
                            continue
                        t = timed(lambda: gp.append(x[n:n + m], yerr[n:n + m]), a.warmup, a.reps, after=lambda: gp.truncate(n))
                        relay = []
                        for _ in range(5):
                            gpp.append(x[n:n + m], yerr[n:n + m])
                            relay.append(gpp.solver.profile()["ms_append_relayout"])
                            gpp.truncate(n)
                        crossing = -(-(n + m) // 128) > -(-n // 128)
                        t_full = yard[("compute", n_big + m)]["median_ms"]
                        emit(dict(op="append", n=n, m=m, path=path, tile_crossing=crossing, relayout_ms=float(np.median(relay)),
                                  t_sweep_ms=t_sweep, t_full_ms=t_full, over_sweep=t["median_ms"] / t_sweep,
                                  full_over_append=t_full / t["median_ms"], **t))
                        if n_big == 65536 and path == 0:
                            c = None
                            if m <= 4 and not crossing:
                                c = dict(n=n, m=m, rule="append <= 2 T_sweep", append_ms=t["median_ms"], bound_ms=2 * t_sweep)
                            elif m in (128, 1024):
                                div = 20 if m == 128 else 5
                                c = dict(n=n, m=m, rule="append <= T_full / %d" % div, append_ms=t["median_ms"], bound_ms=t_full / div)
                            if c is not None:
                                c["met"] = bool(c["append_ms"] <= c["bound_ms"])
                                out["conditions"].append(c)
                                emit()
                finally:
                    N.lib.gh_debug_set_append_path(0)
        del gp, gpp
    emit()
    for c in out["conditions"]:
        print(json.dumps(c))


if __name__ == "__main__":
    main()
