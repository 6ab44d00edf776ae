"""Timing of the device-side neighbour search of ``VecchiaSolver`` against the host search of the same build (needs an MI355X).

For the problems of ``scripts/bench_vecchia_predict.py`` -- N in ``--n`` (65536, 262144, 1048576), 1-D (sorted) and 3-D, m in
``--m`` (16, 32, 64), ``--mtest`` (100000) test points drawn uniformly over the data's box -- wall-clock medians with min .. max, in
one process, of

    host_search      ``vecchia_query_neighbors(x, t, m)`` alone (the tree of the data set is built outside the timed calls)
    predict_host     ``solver.predict_local(kernel, r, t, return_var=True, search="host")``, unassisted
    predict_device   the same with ``search="device"`` (the grid of the data set is built in the warm-up call: ``grid_ms``
                     is that first call minus the median)

then the two routes to ``compute``'s default table, ``vecchia_neighbors(x, m)`` and ``vecchia_neighbors(x, m, device=0)``, at
N = 262144, 3-D (``table_host`` / ``table_device``; the device route builds its grid inside every call), and the occupancy
comparison: the fused call of the C ABI with ``occupancy`` in ``--occupancy`` (4, 8, 16, 32) at N = 262144 and 1048576, 1-D and 3-D,
m = 16 and 64 (``occupancy`` rows; 0 in the other rows is the library's automatic value, ``VG_OCCUPANCY`` in
george_amd/csrc/gh_vecchia_impl.h).  Every call returns host values, so the device work has ended when the clock stops.  The
solvers are computed with the table from the device route (the host route at N = 1048576 takes minutes and is not what is
measured).  No time is asserted anywhere.  Writes ``profiles/vecchia/search_time.json``.

    python scripts/bench_vecchia_search.py [--n 65536] [--m 16,32,64] [--dims 1,3] [--mtest 100000] [--out ...]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)

import george_amd  # noqa: E402
from george_amd import VecchiaSolver  # noqa: E402
from george_amd import _native as N  # noqa: E402
from george_amd.solvers import vecchia  # noqa: E402
from george_amd.solvers.vecchia import vecchia_neighbors, vecchia_query_neighbors  # noqa: E402
from bench_vecchia import problem  # noqa: E402
from bench_vecchia_predict import test_points  # noqa: E402


def timed(fn, warmup, reps):
    """(median, min, max, first call) in ms"""
    first = None
    for _ in range(max(warmup, 1)):
        t0 = time.perf_counter()
        fn()
        first = 1e3 * (time.perf_counter() - t0) if first is None else first
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), first


def fused(solver, y, t, m, occupancy):
    mu, var = np.empty(len(t)), np.empty(len(t))
    N.check(N.lib.gh_vecchia_predict_local_search(solver._handle, solver._dk.handle, solver._dk.handle, N.ptr(y), N.ptr(t), len(t), m,
                                                  occupancy, N.ptr(mu), N.ptr(var), None))
    return mu, var


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[16, 32, 64])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--mtest", type=int, default=100000)
    ap.add_argument("--occupancy", type=ints, default=[4, 8, 16, 32])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecchia", "search_time.json"))
    args = ap.parse_args()
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_vecchia_search.py needs an MI355X")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    rows = []

    def add(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(args.out, "w") as f:                # (after every row: a run that is cut short keeps what it measured)
            json.dump(rows, f, indent=1)
            f.write("\n")

    def ms(t):
        return dict(ms=t[0], ms_min=t[1], ms_max=t[2])

    header = open(os.path.join(ROOT, "george_amd", "csrc", "gh_vecchia_impl.h")).read()
    add(op="automatic_occupancy", occupancy=int(re.search(r"#define VG_OCCUPANCY (\d+)", header).group(1)), compared_with=args.occupancy)
    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            t = test_points(x, args.mtest)
            if ndim > 1:
                vecchia._tree(x)
            for m in args.m:
                base = dict(n=n, ndim=ndim, m=m, m_test=args.mtest)
                solver = VecchiaSolver(make_kernel(), m=m, neighbors=vecchia_neighbors(x, m, device=0))
                solver.compute(x, yerr)
                kernel = solver.kernel
                add(op="host_search", reps=args.host_reps, **ms(timed(lambda: vecchia_query_neighbors(x, t, m), 1, args.host_reps)), **base)
                host = solver.predict_local(kernel, y, t, return_var=True, search="host")
                add(op="predict_host", reps=args.host_reps,
                    **ms(timed(lambda: solver.predict_local(kernel, y, t, return_var=True, search="host"), 0, args.host_reps)), **base)
                tm = timed(lambda: solver.predict_local(kernel, y, t, return_var=True, search="device"), 1, args.reps)
                dev = solver.predict_local(kernel, y, t, return_var=True, search="device")
                add(op="predict_device", reps=args.reps, occupancy=0, grid_ms=tm[3] - tm[0],
                    same_bits=bool(np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1])), **ms(tm), **base)
                if n >= 262144 and m in (16, 64):
                    for occ in args.occupancy:
                        tm = timed(lambda: fused(solver, y, t, m, occ), 1, args.reps)
                        add(op="occupancy", occupancy=occ, reps=args.reps, grid_ms=tm[3] - tm[0], **ms(tm), **base)
                del solver
            VecchiaSolver.release_pool()
    n, m = 262144, 32
    if n in args.n and 3 in args.dims:
        _, x, _, _ = problem(3, n)
        add(op="table_device", n=n, ndim=3, m=m, reps=args.reps, **ms(timed(lambda: vecchia_neighbors(x, m, device=0), 1, args.reps)))
        add(op="table_host", n=n, ndim=3, m=m, reps=args.host_reps, **ms(timed(lambda: vecchia_neighbors(x, m), 0, args.host_reps)))
        add(op="table_same", n=n, ndim=3, m=m, same=bool(np.array_equal(vecchia_neighbors(x, m, device=0), vecchia_neighbors(x, m))))


if __name__ == "__main__":
    main()
