"""``GP.predict`` and ``GP.grad_log_likelihood`` with the HODLR solver: the device-resident strip driver (``HODLRSolver.predict`` /
``HODLRSolver.grad``: gh_hodlr_predict, gh_hodlr_grad) against the generic NumPy branch of ``GP`` on the same solver.

``generic_ms`` is the path ``GP`` took before those methods existed: a subclass of ``HODLRSolver`` with ``predict = grad = None``
sends ``GP`` through its generic branch, unchanged (K(xs, x) to the host, ``apply_inverse`` on its transpose and ``np.dot``;
``get_inverse()`` and the (N, N, P) tensor of ``kernel.get_gradient`` on the host).  Each timing is the wall clock of the public
``GP`` call -- it returns host arrays, so the device work has ended -- as the median of ``--reps`` (>= 7) calls after ``--warmup``
(>= 2) calls, both paths in one process.  ``max_rel_diff`` is the largest difference between the two results relative to the
largest magnitude of the quantity.

predict: 1-D ExpSquared, tol = 1e-10, N in (4096, 16384, 65536, 262144), M = 1000, modes mean / var, and cov for N <= 65536.
grad:    N in (2048, 4096, 8192, 16384) for var(y) * ExpSquared (two parameters) and the docs/tutorials/hyper.rst:91-95 composite
         (eleven); the generic leg is skipped -- the row says so -- where its (N, N, P) host tensor would exceed 32 GB; fused-only
         rows at N = 32768 and 65536.

    python scripts/bench_hodlr_predict_grad.py [--what predict,grad] [--reps 7] [--warmup 2] [--out profiles/hodlr/predict_grad_time.json]
                                               [--n-predict 4096,...] [--n-grad 2048,...] [--n-grad-fused 32768,65536] [--append]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import george_amd  # noqa: E402
from george_amd import GP, HODLRSolver, kernels  # noqa: E402

GENERIC = "HODLRSolver subclass with predict = grad = None: GP's generic branch, the path before the fused methods, unchanged"
HOST_TENSOR_LIMIT = 32e9


class GenericPathHODLR(HODLRSolver):
    predict = None
    grad = None


def hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def problem(kind, n):
    rng = np.random.RandomState(1234)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        y = np.sin(x)
        return (lambda: np.var(y) * kernels.ExpSquaredKernel(1.0)), x, 0.1 * np.ones(n), y, dict(tol=1e-10)
    x = np.sort(rng.uniform(1960.0, 1990.0, n))
    y = 1.3 * (x - 1975.0) + 3.0 * np.sin(2 * np.pi * x)
    return hyper_kernel, x, 0.5 * np.ones(n), y, dict(tol=1e-8)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def rel_diff(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return max(float(np.max(np.abs(p - q)) / max(np.max(np.abs(q)), 1e-300)) for p, q in zip(a, b))


KW = {"mean": dict(return_cov=False), "var": dict(return_var=True), "cov": dict(return_cov=True)}


def emit(rows, row, out):
    rows.append(row)
    print(json.dumps(row), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)


def pair(make_kernel, x, yerr, kw, fused_only):
    gf = GP(make_kernel(), solver=HODLRSolver, **kw)
    gf.compute(x, yerr)
    assert not gf.solver.dense_fallback, "the dense fallback answered: not the path this script measures"
    gg = None
    if not fused_only:
        gg = GP(make_kernel(), solver=GenericPathHODLR, **kw)
        gg.compute(x, yerr)
    return gf, gg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="predict,grad")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--n-predict", default="4096,16384,65536,262144")
    ap.add_argument("--n-grad", default="2048,4096,8192,16384")
    ap.add_argument("--n-grad-fused", default="32768,65536")
    ap.add_argument("--grad-kernels", default="expsq,hyper")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the rows already in --out")
    a = ap.parse_args()
    if a.reps < 7 or a.warmup < 2:
        ap.error("a timing is the median of at least 7 calls after at least 2 warm-up calls")
    if george_amd.device_count() <= 0:
        sys.exit("no MI355X visible: nothing is measured without one")
    rows = []
    if a.append and a.out and os.path.exists(a.out):
        with open(a.out) as f:
            rows = json.load(f)
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    what = a.what.split(",")
    if "predict" in what:
        for n in ints(a.n_predict):
            mk, x, yerr, y, kw = problem("expsq", n)
            gf, gg = pair(mk, x, yerr, kw, False)
            t = np.sort(np.random.RandomState(n).uniform(0, 10, a.m))
            for mode in ("mean", "var", "cov"):
                if mode == "cov" and n > 65536:
                    continue
                tf, rf = timed(lambda: gf.predict(y, t, **KW[mode]), a.warmup, a.reps)
                tg, rg = timed(lambda: gg.predict(y, t, **KW[mode]), a.warmup, a.reps)
                emit(rows, dict(op="predict", kernel="expsq", n=n, m=a.m, mode=mode, generic_ms=tg, fused_ms=tf, speedup=tg / tf,
                                max_rel_diff=rel_diff(rf, rg), generic_path=GENERIC), a.out)
            del gf, gg
    if "grad" in what:
        for kind in a.grad_kernels.split(","):
            for n, fused_only in [(n, False) for n in ints(a.n_grad)] + [(n, True) for n in ints(a.n_grad_fused)]:
                mk, x, yerr, y, kw = problem(kind, n)
                P = len(mk())
                too_big = 8.0 * n * n * P > HOST_TENSOR_LIMIT
                gf, gg = pair(mk, x, yerr, kw, fused_only or too_big)
                tf, rf = timed(lambda: gf.grad_log_likelihood(y), a.warmup, a.reps)
                row = dict(op="grad", kernel=kind, n=n, m=None, mode="grad", n_params=P, generic_ms=None, fused_ms=tf, speedup=None,
                           max_rel_diff=None, max_rank=int(max(gf.solver.ranks())), generic_path=GENERIC)
                if gg is not None:
                    tg, rg = timed(lambda: gg.grad_log_likelihood(y), a.warmup, a.reps)
                    row.update(generic_ms=tg, speedup=tg / tf, max_rel_diff=rel_diff(rf, rg))
                elif too_big:
                    row["generic_path"] = "skipped: the (N, N, P) host tensor of the generic branch would take %.0f GB" % (8e-9 * n * n * P)
                else:
                    row["generic_path"] = "not run: fused-only row"
                emit(rows, row, a.out)
                del gf, gg


if __name__ == "__main__":
    main()
