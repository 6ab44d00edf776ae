"""Marginalised predictive over a chain: B predictions as the loop ``set_parameter_vector(v); predict(y, t, ...)`` against
ONE ``GP.predict_batch(vectors, y, t, ...)`` (gh_chol_predict_batch), in one process, in all three return modes.

Shapes: the docs/tutorials/hyper.rst:255-268 one (N = 468, M = 250, B = 50), the model.rst:401-408 one (N = 50, M = 500,
B = 24) and N = 1024 / 2048 / 4096 at M = 256, B = 36; two kernels -- 1-D ExpSquared (the fast form) and the hyper.rst
composite (the postfix walker).  Both paths are warmed up, each is timed as the median of --reps runs, and one JSON object
per configuration is printed: both times, their ratio, the largest difference between the two paths relative to the
largest magnitude of the quantity, and for mode "cov" the host SVD draw of sample_conditional_batch (its share of that
call).

    python scripts/dev/predict_batch_time.py [--reps 5] [--shapes 468:250:50,50:500:24] [--kernels expsq,hyper]
                                             [--modes mean,var,cov] [--out file.json]
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
from george_amd.utils import multivariate_gaussian_samples  # noqa: E402

SHAPES = "468:250:50,50:500:24,1024:256:36,2048:256:36,4096:256:36"


def hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def problem(kind, n, m, B):
    rng = np.random.RandomState(n + m)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        gp = GP(np.var(np.sin(x)) * kernels.ExpSquaredKernel(1.0))
        y = np.sin(x) + 0.1 * rng.randn(n)
        t = np.linspace(0, 10, m)
    else:
        x = np.sort(rng.uniform(0, 40, n))
        gp = GP(hyper_kernel(), mean=0.0, fit_mean=True, white_noise=np.log(0.05), fit_white_noise=True)
        y = 50.0 * np.sin(x / 5.0) + rng.randn(n)
        t = np.linspace(0, 40, m)
    gp.compute(x, 0.1)
    p0 = gp.get_parameter_vector()
    return gp, y, t, p0 + 1e-3 * rng.randn(B, len(p0))


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


KW = {"mean": dict(return_cov=False), "var": dict(return_var=True), "cov": dict(return_cov=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=SHAPES, help="N:M:B,...")
    ap.add_argument("--kernels", default="expsq,hyper")
    ap.add_argument("--modes", default="mean,var,cov")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for kind in a.kernels.split(","):
        for shape in a.shapes.split(","):
            n, m, B = (int(v) for v in shape.split(":"))
            gp, y, t, vec = problem(kind, n, m, B)
            p0 = gp.get_parameter_vector()
            for mode in a.modes.split(","):
                kw = KW[mode]

                def loop():
                    out = []
                    for v in vec:
                        gp.set_parameter_vector(v)
                        out.append(gp.predict(y, t, **kw))
                    gp.set_parameter_vector(p0)
                    return out

                def batch():
                    return gp.predict_batch(vec, y, t, **kw)

                rb, rl = batch(), loop()
                if mode == "mean":
                    pairs = [(rb, np.array(rl))]
                else:
                    pairs = [(rb[0], np.array([o[0] for o in rl])), (rb[1], np.array([o[1] for o in rl]))]
                diff = max(float(np.max(np.abs(p - q)) / max(np.max(np.abs(q)), 1e-300)) for p, q in pairs)
                t_loop, t_batch = median_time(loop, a.reps), median_time(batch, a.reps)
                row = dict(kernel=kind, n=n, m=m, B=B, mode=mode, loop_ms=1e3 * t_loop, batch_ms=1e3 * t_batch,
                           speedup=t_loop / t_batch, max_rel_diff=diff)
                if mode == "cov":
                    mu, cov = rb

                    def draws():
                        for b in range(B):
                            multivariate_gaussian_samples(cov[b], 1, mean=mu[b])

                    row["host_draw_ms"] = 1e3 * median_time(draws, a.reps)
                    row["draw_share_of_sample_conditional_batch"] = row["host_draw_ms"] / (row["host_draw_ms"] + row["batch_ms"])
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
