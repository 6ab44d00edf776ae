#!/usr/bin/env python3
"""Wall clock of ``InducingSolver.grad_inducing`` beside ``InducingSolver.grad`` on one MI355X.

Problems: the 1-D and 3-D timing problems of ``scripts/bench_inducing.py`` (``bench_vecchia.problem``) for N in ``--n`` and
m in ``--m``, relative jitter ``--jitter``, the objectives of ``--objectives`` (dtc, fitc, vfe).  Per configuration the solver is
computed once and each call is timed ``--reps`` times after ``--warmup``: the median, with min and max.  Rows:

    op = "grad"            ``s.grad(r, which)`` of this build
    op = "grad_inducing"   ``s.grad_inducing(r, which)`` of this build: the same work and one more pass of N m input gradients
    op = "grad", build = "parent"   ``s.grad`` of the package under ``--parent`` (a built checkout of the parent commit), timed by
                           a child process in the same session -- what ``grad`` cost before the body was shared (dtc and fitc only)

    python scripts/bench_inducing_ugrad.py [--n 16384,65536] [--m 256,1024] [--dims 1,3] [--parent DIR] [--out ...]

Writes ``profiles/inducing/ugrad_time.json``.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTIVES = {"dtc": dict(method="dtc"), "fitc": dict(method="fitc"), "vfe": dict(method="dtc", variational=True)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(ms=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), ms_max=1e3 * float(np.max(ts)))


def run(args, build):
    """the rows of the package that is importable first; ``build`` == "parent": ``grad`` alone, without the bound"""
    import george_amd
    from george_amd import InducingSolver
    from bench_vecchia import problem
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_inducing_ugrad.py needs an MI355X")
    rows = []
    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            for m in args.m:
                if m > n:
                    continue
                for objective in args.objectives:
                    if build == "parent" and objective == "vfe":
                        continue
                    kernel = make_kernel()
                    s = InducingSolver(kernel, inducing=m, jitter=args.jitter, **OBJECTIVES[objective])
                    s.compute(x, yerr)
                    which = kernel.unfrozen_mask.astype(np.uint32)
                    base = dict(build=build, ndim=ndim, n=n, m=m, objective=objective, reps=args.reps)
                    rows.append(dict(base, op="grad", **timed(lambda: s.grad(y, which), args.warmup, args.reps)))
                    if build != "parent":
                        rows.append(dict(base, op="grad_inducing", **timed(lambda: s.grad_inducing(y, which), args.warmup, args.reps)))
                    del s
                    InducingSolver.release_pool()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[16384, 65536])
    ap.add_argument("--m", type=ints, default=[256, 1024])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--objectives", type=lambda s: s.split(","), default=["dtc", "fitc", "vfe"])
    ap.add_argument("--jitter", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its grad is timed by a child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)          # (the child: rows of the package under this root, as JSON)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    if args.child:
        sys.path.insert(0, os.path.abspath(args.child))
        print("ROWS " + json.dumps(run(args, "parent")), flush=True)
        return
    sys.path.insert(0, ROOT)
    rows = run(args, "this")
    if args.parent:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", args.parent, "--n", ",".join(map(str, args.n)), "--m", ",".join(map(str, args.m)),
               "--dims", ",".join(map(str, args.dims)), "--objectives", ",".join(args.objectives), "--jitter", repr(args.jitter),
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
        rows += json.loads([line for line in out.splitlines() if line.startswith("ROWS ")][-1][5:])
    for r in rows:
        print(json.dumps(r), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", "inducing", "ugrad_time.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
