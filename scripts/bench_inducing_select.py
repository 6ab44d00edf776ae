"""Timing of the max-min selection of inducing points on the device against the host routine of the same build: the table of
the README's inducing section (needs an MI355X).

Problems: the 1-D and 3-D timing problems of ``scripts/bench_inducing.py`` (``bench_vecchia.problem``) for N in ``--n`` (65536,
262144, 1048576) and m in ``--m`` (256, 1024, 4096), and one full ordering (m = N) at ``--full-n`` (65536) points in 3-D.

    device_ms   ``inducing_points(x, m, device=0)``: the first point on the host (one pass over x), the upload, one kernel per pick
                and the indices back; the median of ``--reps`` (10) calls after ``--warmup`` (2), with min .. max
    abi_ms      ``gh_inducing_select`` alone on the same host arrays with that first point, measured the same way
    host_s      ``inducing_points(x, m)``, the yardstick -- the parent commit's code unchanged: the median of ``--host-reps`` (3) calls
                while one takes under ``--host-once`` (2) seconds, else that one call
    equal       the two index arrays are equal (``np.array_equal``); ``speedup`` = host_s / device time

Every call returns host arrays, so the device work has ended when the clock stops.  Writes ``profiles/inducing/select_time.json``.

    python scripts/bench_inducing_select.py [--n 65536,262144] [--m 256,1024] [--dims 1,3] [--reps 10] [--full-n 65536] [--out ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import george_amd  # noqa: E402
from george_amd import _native as N  # noqa: E402
from george_amd.solvers.inducing import inducing_points  # noqa: E402


def spread(ts):
    return dict(ms=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), ms_max=1e3 * float(np.max(ts)))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def one_row(x, m, args, what):
    n, ndim = x.shape
    k = min(m, n)
    ts, idx_dev = timed(lambda: inducing_points(x, m, device=args.device), args.warmup, args.reps)
    row = dict(what=what, n=n, ndim=ndim, m=m, reps=args.reps)
    row.update({"device_" + key: v for key, v in spread(ts).items()})
    first = int(idx_dev[0])
    idx_abi = np.empty(k, dtype=np.int64)

    def abi():
        N.check(N.lib.gh_inducing_select(args.device, N.ptr(x), n, ndim, first, m, N.ptr(idx_abi), None))
        return idx_abi

    ts, _ = timed(abi, args.warmup, args.reps)
    row.update({"abi_" + key: v for key, v in spread(ts).items()})
    row["abi_us_per_pick"] = 1e3 * row["abi_ms"] / max(k - 1, 1)
    t0 = time.perf_counter()
    idx_host = inducing_points(x, m)
    hs = [time.perf_counter() - t0]
    if hs[0] < args.host_once:
        hs, idx_host = timed(lambda: inducing_points(x, m), 0, args.host_reps)
    row.update(host_s=float(np.median(hs)), host_calls=len(hs))
    row["equal"] = bool(np.array_equal(idx_dev, idx_host) and np.array_equal(idx_abi, idx_host))
    row["speedup"] = row["host_s"] / (1e-3 * row["device_ms"])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[256, 1024, 4096])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--full-n", type=int, default=65536, help="points of the full ordering in 3-D; 0: none")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-once", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inducing", "select_time.json"))
    args = ap.parse_args()
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_inducing_select.py needs an MI355X")
    from bench_vecchia import problem
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = []

    def save():                                       # (after every row: a run that is cut short keeps what it measured)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")

    for ndim in args.dims:
        for n in args.n:
            x = np.ascontiguousarray(problem(ndim, n)[1])
            for m in args.m:
                if m <= n:
                    rows.append(one_row(x, m, args, "select"))
                    save()
    if args.full_n > 0:
        rows.append(one_row(np.ascontiguousarray(problem(3, args.full_n)[1]), args.full_n, args, "full_ordering"))
        save()


if __name__ == "__main__":
    main()
