"""Many likelihood gradients: the loop ``nll_and_grad(v, y)`` (one fused device call per vector, gh_chol_objective) against
ONE ``GP.nll_and_grad_batch(vectors, y)`` (gh_chol_objective_grad_batch), in one process.

Grid: N in {468, 1024, 2048, 4096} x B in {1, 8, 36, 128}, on two kernels -- 1-D ExpSquared (the fast form) and the 17-node
docs/tutorials/hyper.rst composite (the postfix walker), both with fitted mean and white noise.  Both paths are warmed up,
each is timed as the median of --reps runs, and one JSON object per configuration is printed: both times, their ratio, and
the largest difference of the two gradients relative to the largest gradient magnitude of the member.

    python scripts/dev/grad_batch_time.py [--reps 5] [--ns 468,1024,2048,4096] [--bs 1,8,36,128] [--kernels expsq,hyper]
                                          [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from george_amd import GP, kernels  # noqa: E402


def hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def problem(kind, n, B):
    rng = np.random.RandomState(n + B)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        gp = GP(np.var(np.sin(x)) * kernels.ExpSquaredKernel(1.0), mean=0.0, fit_mean=True, white_noise=np.log(0.01),
                fit_white_noise=True)
        y = np.sin(x) + 0.1 * rng.randn(n)
    else:
        x = np.sort(rng.uniform(0, 40, n))
        gp = GP(hyper_kernel(), mean=0.0, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True)
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
    gp.compute(x, 0.1)
    p0 = gp.get_parameter_vector()
    return gp, y, p0 + 1e-3 * rng.randn(B, len(p0))


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", default="468,1024,2048,4096")
    ap.add_argument("--bs", default="1,8,36,128")
    ap.add_argument("--kernels", default="expsq,hyper")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for kind in a.kernels.split(","):
        for n in (int(v) for v in a.ns.split(",")):
            for B in (int(v) for v in a.bs.split(",")):
                gp, y, vec = problem(kind, n, B)
                p0 = gp.get_parameter_vector()

                def loop():
                    out = [gp.nll_and_grad(v, y) for v in vec]
                    gp.set_parameter_vector(p0)
                    return np.array([o[0] for o in out]), np.array([o[1] for o in out])

                def batch():
                    return gp.nll_and_grad_batch(vec, y)

                (nb, gb), (nl, gl) = batch(), loop()
                scale = np.maximum(np.max(np.abs(gl), axis=1, keepdims=True), 1e-300)
                diff = float(np.max(np.abs(gb - gl) / scale))
                t_loop, t_batch = median_time(loop, a.reps), median_time(batch, a.reps)
                row = dict(kernel=kind, n=n, B=B, loop_ms=1e3 * t_loop, batch_ms=1e3 * t_batch, speedup=t_loop / t_batch,
                           max_rel_grad_diff=diff, max_abs_nll_diff=float(np.max(np.abs(nb - nl))))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
