"""Emcee-style ensemble step: B log-likelihoods as the loop ``set_parameter_vector(v); log_likelihood(y)`` against ONE
``GP.log_likelihood_batch(vectors, y)`` (gh_chol_objective_batch), in one process.

For N in {468, 1024, 2048, 4096}, B in {1, 8, 36, 128} and two kernels -- 1-D ExpSquared (the fast form) and the
docs/tutorials/hyper.rst:91-95 composite (the postfix walker) -- it warms both paths up, takes the median of --reps
timings of each and prints one JSON object per configuration: likelihoods per second both ways, their ratio, and the
host preparation of the batched call (the Python mapping of the vectors to kernel rows / sigma / r plus the kernel's
flattening -- everything in front of the native call; the native call's own host part is the node expansion, a few
microseconds).

    python scripts/dev/batch_time.py [--reps 5] [--n 468,1024] [--b 1,36] [--kernels expsq,hyper] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from george_amd import GP, BasicSolver, kernels  # noqa: E402
from george_amd.program import DeviceKernel  # noqa: E402


def hyper_kernel():
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def problem(kind, n, B):
    rng = np.random.RandomState(n)
    if kind == "expsq":
        x = np.sort(rng.uniform(0, 10, n))
        gp = GP(np.var(np.sin(x)) * kernels.ExpSquaredKernel(1.0))
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
    ap.add_argument("--n", default="468,1024,2048,4096")
    ap.add_argument("--b", default="1,8,36,128")
    ap.add_argument("--kernels", default="expsq,hyper")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for kind in a.kernels.split(","):
        for n in [int(v) for v in a.n.split(",")]:
            for B in [int(v) for v in a.b.split(",")]:
                gp, y, vec = problem(kind, n, B)
                p0 = gp.get_parameter_vector()

                def loop():
                    for v in vec:
                        gp.set_parameter_vector(v)
                        gp.log_likelihood(y)
                    gp.set_parameter_vector(p0)

                def batch():
                    return gp.log_likelihood_batch(vec, y)

                def prep():
                    gp._batch_inputs(vec, y, quiet=True)
                    DeviceKernel(gp.kernel)

                ll_b = batch()
                loop()
                ll_l = np.array([(gp.set_parameter_vector(v), gp.log_likelihood(y))[1] for v in vec])
                gp.set_parameter_vector(p0)
                t_loop, t_batch, t_prep = median_time(loop, a.reps), median_time(batch, a.reps), median_time(prep, a.reps)
                row = dict(kernel=kind, n=n, B=B, loop_ms=1e3 * t_loop, batch_ms=1e3 * t_batch,
                           loop_lik_per_s=B / t_loop, batch_lik_per_s=B / t_batch, speedup=t_loop / t_batch,
                           host_prep_ms=1e3 * t_prep,
                           max_rel_diff=float(np.max(np.abs(ll_b - ll_l) / np.abs(ll_l))))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
