"""Timing of ``VecchiaSolver.fisher_blocks`` (gh_vecchia_fisher), the expected information of the hyper-parameters for the Vecchia
likelihood.  Needs an MI355X.  Writes ``profiles/vecchia/fisher_time.json``.

Wall-clock medians (with minimum and maximum) of ``--reps`` (20) calls after ``--warmup`` (2) of

    fisher       ``solver.fisher_blocks()`` on a computed solver: every kernel parameter, no diagonal rows
    nll_grad     ``GP.nll_and_grad`` of the same build in the same session, at a parameter vector that changes from call to call:
                 the yardstick -- one factorisation and one pass of the gradient kernel over the same blocks

for N in ``--n`` (65536, 262144, 1048576) and m in ``--m`` (16, 32, 64) on the 1-D inputs of scripts/bench_vecchia.py (a fixed
point density), with two kernels: ``var(y) * ExpSquared`` (2 parameters) and the 17-node composite of docs/tutorials/hyper.rst
(11 parameters; error bars 0.1 of its amplitude).  Every call returns host values, so the device work has ended when the clock
stops.  At N = ``--dense-n`` (4096) also ``BasicSolver.fisher`` and, at m = 64, the largest difference of the two matrices over
``sqrt(F_aa F_bb)`` -- the two are different quantities unless every predecessor is in the conditioning set, so that figure says
how far the information of the approximate likelihood is from the dense one on this problem, not how accurate the kernel is
(tests/test_gpu_vecchia_fisher.py pins that).  ``--big`` adds one ``GP.fisher_information()`` at N = 1 048 576 in 3-D with m = 32
(the neighbour table from the device search), timed once.

    python scripts/bench_vecchia_fisher.py [--n 65536,262144] [--m 16,32,64] [--reps 20] [--big] [--out ...]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import george_amd  # noqa: E402
from george_amd import GP, BasicSolver, VecchiaSolver, kernels  # noqa: E402


def hyper_kernel():
    """the 17-node composite of docs/tutorials/hyper.rst (tests/loo_ref.py: kernel_hyper)"""
    K = kernels
    k1 = 66.0 ** 2 * K.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * K.ExpSquaredKernel(90.0 ** 2) * K.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * K.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * K.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def problem(name, n):
    rng = np.random.RandomState(1234)
    x = np.sort(rng.uniform(0, 10.0 * n / 16384.0, n))[:, None]              # a fixed point density: 1638 points per unit
    y = np.sin(x[:, 0])
    if name == "expsq":
        return (lambda: np.var(y) * kernels.ExpSquaredKernel(1.0)), x, 0.1 * np.ones(n), y
    return hyper_kernel, x, 6.6 * np.ones(n), 66.0 * y


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts))), out


def run(args, save):
    rows = []
    for n in sorted(set(args.n + [args.dense_n])):
        for name in ("expsq", "hyper"):
            make_kernel, x, yerr, y = problem(name, n)
            dense_F = None
            if n == args.dense_n:
                b = BasicSolver(make_kernel())
                b.compute(x, yerr)
                t, dense_F = timed(b.fisher, args.warmup, args.reps)
                rows.append(dict(t, solver="BasicSolver", op="fisher", kernel=name, n=n, planes=len(dense_F)))
                print(json.dumps(rows[-1]), flush=True)
                del b
                BasicSolver.release_pool()
            for m in args.m:
                base = dict(solver="VecchiaSolver", kernel=name, n=n, m=m)
                s = VecchiaSolver(make_kernel(), m=m)
                s.compute(x, yerr)
                t, F = timed(s.fisher_blocks, args.warmup, args.reps)
                row = dict(t, op="fisher", planes=len(F), **base)
                if dense_F is not None and m == 64:
                    d = np.sqrt(np.diag(dense_F))
                    row["diff_to_dense_over_S"] = float(np.max(np.abs(F - dense_F) / np.outer(d, d)))
                rows.append(row)
                print(json.dumps(row), flush=True)
                del s
                gp = GP(make_kernel(), solver=VecchiaSolver, m=m)
                gp.compute(x, yerr)
                p0 = gp.get_parameter_vector()
                count = [0]

                def nll_grad():
                    count[0] += 1
                    return gp.nll_and_grad(p0 + 1e-6 * (count[0] % 7), y)

                t, _ = timed(nll_grad, args.warmup, args.reps)
                rows.append(dict(t, op="nll_grad", **base))
                rows[-1]["fisher_over_nll_grad"] = row["ms"] / t["ms"]
                print(json.dumps(rows[-1]), flush=True)
                del gp
                save(rows)
    if args.big:
        n, m = 1048576, 32
        rng = np.random.RandomState(1234)
        x = rng.uniform(0, 1, (n, 3)) * (n / 16384.0) ** (1.0 / 3)
        x = x[np.argsort(x[:, 0], kind="stable")]
        kernel = kernels.Matern52Kernel(0.5, ndim=3) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=3)
        gp = GP(kernel, solver=VecchiaSolver, m=m, search="device")
        t0 = time.perf_counter()
        gp.compute(x, 0.1)
        t1 = time.perf_counter()
        F = gp.fisher_information()
        t2 = time.perf_counter()
        rows.append(dict(solver="VecchiaSolver", op="GP.fisher_information", kernel="Matern52 + Constant", ndim=3, n=n, m=m,
                         compute_s=t1 - t0, ms=1e3 * (t2 - t1), F=F.tolist(), eig_min=float(np.min(np.linalg.eigvalsh(F)))))
        print(json.dumps(rows[-1]), flush=True)
        save(rows)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[16, 32, 64])
    ap.add_argument("--dense-n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecchia", "fisher_time.json"))
    args = ap.parse_args()
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_vecchia_fisher.py needs an MI355X")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save(rows):                                   # (after every configuration: a run that is cut short keeps what it measured)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")

    save(run(args, save))


if __name__ == "__main__":
    main()
