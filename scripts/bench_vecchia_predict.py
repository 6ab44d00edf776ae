"""Timing of ``VecchiaSolver.predict_local`` against the predictor through ``Q``, and the accuracy table of both.

``--what time`` (needs an MI355X): wall-clock medians of ``--reps`` (20) calls after ``--warmup`` (2), with min .. max, of

    local_device   ``solver.predict_local(kernel, r, t, return_var=True, neighbors=table)``: the device call with the table given
    search         ``vecchia_query_neighbors(x, t, m)`` on its own: the host search the call runs when no table is given
                   (the tree of the data set is built once, outside the timed calls: ``tree_s``)
    global         ``solver.predict(kernel, r, t, return_var=True)`` through ``Q`` at M = 1000: the yardstick from this build

for N in ``--n`` (65536, 262144, 1048576), 1-D (sorted uniform points, ``var(y) * ExpSquared``) and 3-D (uniform points sorted by
their first coordinate, ``Matern52 + Constant``) -- the problems of ``scripts/bench_vecchia.py`` --, m in ``--m`` (16, 32, 64) and
M in ``--mtest`` (1000, 100000) test points drawn uniformly over the data's box.  Every call returns host values, so the device
work has ended when the clock stops.  ``--parent-tree PATH`` names a checkout of the parent commit with its library built: the
same ``global`` rows are then measured in a child process that imports the package from there (``--tree``) and recorded as
``global_parent``.  No time is asserted anywhere.  Writes ``profiles/vecchia/predict_local_time.json``.

``--what accuracy`` (CPU only): both predictors restated in NumPy (tests/vecchia_ref.py, tests/vecchia_local_ref.py) against
dense LAPACK at N = 2000, error bars 0.1 of the amplitude, default tables, 300 random test points, m = 8 / 16 / 32 / 64.  Per row:
the largest ``|mu - mu_dense| / sd_dense``, the smallest variance, the range of the variance over the dense one, and the largest
error in units of the predictor's OWN standard deviation (``null`` where its variance is not positive).  Writes
``profiles/vecchia/predict_local_accuracy.json``.

    python scripts/bench_vecchia_predict.py --what time [--n 65536] [--m 16,32,64] [--dims 1,3] [--mtest 1000,100000] [--out ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree PATH: import the package (and its built library) from another checkout, e.g. one of the parent commit
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else ROOT
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(TREE, "scripts"))
sys.path.insert(0, TREE)

import george_amd  # noqa: E402
from george_amd import VecchiaSolver, kernels  # noqa: E402
from george_amd.solvers import vecchia  # noqa: E402
from george_amd.solvers.vecchia import vecchia_neighbors  # noqa: E402
from bench_vecchia import problem  # noqa: E402


def timed(fn, warmup, reps):
    """(median, min, max) in ms"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def test_points(x, mtest):
    rng = np.random.RandomState(7)
    lo, hi = x.min(axis=0), x.max(axis=0)
    return np.ascontiguousarray(lo + (hi - lo) * rng.rand(mtest, x.shape[1]))


def run_time(args, save):
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_vecchia_predict.py --what time needs an MI355X")
    has_local = hasattr(VecchiaSolver, "predict_local")
    rows = []

    def add(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        save(rows)

    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            for m in args.m:
                solver = VecchiaSolver(make_kernel(), m=m)
                solver.compute(x, yerr)
                base = dict(n=n, ndim=ndim, m=m)
                t = test_points(x, 1000)
                ms = timed(lambda: solver.predict(solver.kernel, y, t, return_var=True), args.warmup, args.reps)
                add(op=args.global_label, m_test=1000, ms=ms[0], ms_min=ms[1], ms_max=ms[2], **base)
                if not has_local or args.global_only:
                    continue
                t0 = time.perf_counter()
                if ndim > 1:                                                 # (sorted 1-D inputs need no tree)
                    vecchia._tree(x)
                tree_s = time.perf_counter() - t0
                for mtest in args.mtest:
                    t = test_points(x, mtest)
                    reps = args.reps if mtest <= 10000 else max(3, args.reps // 4)
                    ms = timed(lambda: vecchia.vecchia_query_neighbors(x, t, m), 1, reps)
                    add(op="search", m_test=mtest, ms=ms[0], ms_min=ms[1], ms_max=ms[2], reps=reps, tree_s=tree_s, **base)
                    table = vecchia.vecchia_query_neighbors(x, t, m)
                    ms = timed(lambda: solver.predict_local(solver.kernel, y, t, return_var=True, neighbors=table), args.warmup, args.reps)
                    add(op="local_device", m_test=mtest, ms=ms[0], ms_min=ms[1], ms_max=ms[2], **base)
                del solver
            VecchiaSolver.release_pool()
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--what", "time", "--global-only", "--global-label", "global_parent", "--out", args.out + ".parent",
               "--n", ",".join(map(str, args.n)), "--m", ",".join(map(str, args.m)), "--dims", ",".join(map(str, args.dims)),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--tree", args.parent_tree]
        subprocess.check_call(cmd)
        rows += json.load(open(args.out + ".parent"))
        os.remove(args.out + ".parent")
        save(rows)
    return rows


def run_accuracy(args):
    from oracle import solver_np
    import vecchia_local_ref
    import vecchia_ref
    rows = []
    n, ntest = 2000, 300
    rng = np.random.RandomState(2000)
    x1 = np.sort(rng.uniform(0, 100, n))[:, None]
    x2 = rng.uniform(0, 6, (n, 2))
    x2 = x2[np.argsort(x2[:, 0], kind="stable")]
    cases = [("1-D Matern-3/2", 1.0 * kernels.Matern32Kernel(1.0), x1), ("1-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(1.0), x1),
             ("2-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(0.25, ndim=2), x2)]
    for name, kernel, x in cases:
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.randn(n)
        t = x.min(axis=0) + (x.max(axis=0) - x.min(axis=0)) * rng.rand(ntest, x.shape[1])
        d = vecchia_ref.dense(kernel, x, 0.1, y, t)
        sd = np.sqrt(d["var"])
        for m in (8, 16, 32, 64):
            ref = vecchia_ref.reference(kernel, x, 0.1, vecchia_neighbors(x, m), r=y)
            gmu, gvar, _ = ref.predict(kernel, t)
            lmu, lvar = vecchia_local_ref.predict(kernel, kernel, x, 0.1, y, t, vecchia_local_ref.query_neighbors(x, t, m))
            for which, mu, var in (("through Q", gmu, gvar), ("m nearest data points", lmu, lvar)):
                own = float(np.max(np.abs(mu - d["mu"]) / np.sqrt(var))) if np.all(var > 0) else None
                rows.append(dict(case=name, predictor=which, n=n, m=m, max_err_over_sd_dense=float(np.max(np.abs(mu - d["mu"]) / sd)),
                                 min_var=float(var.min()), var_over_dense_min=float((var / d["var"]).min()),
                                 var_over_dense_max=float((var / d["var"]).max()), max_err_over_own_sd=own))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="time", choices=["time", "accuracy"])
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[16, 32, 64])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--mtest", type=ints, default=[1000, 100000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--global-only", action="store_true")
    ap.add_argument("--global-label", default="global")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "vecchia", "predict_local_time.json" if args.what == "time" else "predict_local_accuracy.json")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save(rows):                                   # (after every configuration: a run that is cut short keeps what it measured)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")

    save(run_time(args, save) if args.what == "time" else run_accuracy(args))


if __name__ == "__main__":
    main()
