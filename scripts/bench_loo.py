#!/usr/bin/env python3
"""Wall clock of leave-one-out cross-validation on the dense solver, beside the marginal-likelihood calls it mirrors.

Quantity   GP.loo_log_likelihood(y) on a computed GP (the value path: L^-1 and a column reduction), and
           GP.loo_nll_and_grad(p, y) at a new p (one fused call: build, factor, K^-1, S S^T, contraction);
           beside them GP.compute, GP.nll and GP.nll_and_grad of THIS build and -- ``--parent DIR``, a directory that holds a
           built checkout of the parent commit -- of the parent, timed by a child process in the same session.
Method     median of 20 calls after 3 warm-ups, min .. max kept; every fused call gets a parameter vector it has not just seen.
Sizes      N = 4096, 16 384, 32 768 on 1-D ExpSquared and on the hyper.rst composite.
Today      at N = 4096 and 16 384 also what a user does without this feature: ``solver.get_inverse()`` to the host and the
           NumPy formulas: the value (diag, alpha), median of 3 after a warm-up; the gradient given those (v, the matrix
           B = 1/2 (v a^T + a v^T) - K^-1 diag(w) K^-1, and its contraction with ``kernel.get_gradient`` 128 rows at a
           time, since the (N, N, P) tensor does not fit), and the matrix B alone -- median of 3 after a warm-up at
           N = 4096, ONE call without warm-up at N = 16 384 (it takes a minute).

Writes profiles/loo/loo_time.json (``--out``).  Expectation from flop counts, not from a run: loo_nll_and_grad about 2x the
parent's nll_and_grad, loo_log_likelihood about the parent's compute."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 16384, 32768)
TODAY_SIZES = (4096, 16384)


def _kernel(name, kernels, y):
    if name == "expsq":
        return float(np.var(y)) * kernels.ExpSquaredKernel(1.0)
    k1 = 66.0 ** 2 * kernels.ExpSquaredKernel(metric=67.0 ** 2)
    k2 = 2.4 ** 2 * kernels.ExpSquaredKernel(90.0 ** 2) * kernels.ExpSine2Kernel(gamma=2.0 / 1.3 ** 2, log_period=0.0)
    k3 = 0.66 ** 2 * kernels.RationalQuadraticKernel(log_alpha=np.log(0.78), metric=1.2 ** 2)
    k4 = 0.18 ** 2 * kernels.ExpSquaredKernel(1.6 ** 2)
    return k1 + k2 + k3 + k4


def _data(name, n):
    rng = np.random.RandomState(n)
    if name == "expsq":
        x = np.sort(rng.uniform(0.0, n / 70.0, n))
        return x, 0.1 + 0.05 * rng.rand(n), np.sin(x) + 0.1 * rng.randn(n)
    x = np.sort(rng.uniform(0.0, 40.0, n))
    return x, 6.0 + 3.0 * rng.rand(n), 50.0 * np.sin(x / 5.0) + 6.0 * rng.randn(n)


def _time(fn, reps, warm):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warm + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), calls=reps)


def measure(names, sizes, reps, warm, loo):
    """the timings of the package that is importable right now (``loo``: it has the leave-one-out methods)"""
    from george_amd import GP, kernels
    out = []
    for name in names:
        for n in sizes:
            x, yerr, y = _data(name, n)
            gp = GP(_kernel(name, kernels, y))
            gp.compute(x, yerr)
            p0 = gp.get_parameter_vector()
            fresh = lambda i: p0 + 1e-9 * (1 + i % 2)                 # noqa: E731  (never the vector just computed)
            row = dict(kernel=name, n=n)
            row["compute_ms"] = _time(lambda i: gp.compute(x, yerr), reps, warm)
            row["nll_ms"] = _time(lambda i: gp.nll(fresh(i), y), reps, warm)
            gp._grad_seen = False
            row["nll_and_grad_ms"] = _time(lambda i: gp.nll_and_grad(fresh(i), y), reps, warm)
            if loo:
                gp.compute(x, yerr)
                row["loo_log_likelihood_ms"] = _time(lambda i: gp.loo_log_likelihood(y), reps, warm)
                row["loo_nll_and_grad_ms"] = _time(lambda i: gp.loo_nll_and_grad(fresh(i), y), reps, warm)
                if n in TODAY_SIZES:
                    gp.compute(x, yerr)
                    r = y - gp._call_mean(gp._x)
                    keep = {}

                    def value(i):
                        Kinv = gp.solver.get_inverse()
                        alpha = gp.solver.apply_inverse(r)
                        c = np.diag(Kinv)
                        keep["s"] = (Kinv, alpha, c)
                        return np.sum(0.5 * np.log(c) - 0.5 * alpha ** 2 / c - 0.5 * np.log(2 * np.pi))

                    def grad_matrix(i):
                        Kinv, alpha, c = keep["s"]
                        u = alpha / c
                        w = 0.5 * (1.0 + alpha * u) / c
                        v = gp.solver.apply_inverse(u)
                        return 0.5 * (np.outer(v, alpha) + np.outer(alpha, v)) - np.dot(Kinv * w[None, :], Kinv)

                    def grad_full(i):
                        B = grad_matrix(i)
                        g = 0.0
                        for s0 in range(0, n, 128):                   # the (N, N, P) tensor of dK does not fit: 128 rows at a time
                            g = g + np.einsum("ijk,ij", gp.kernel.get_gradient(gp._x[s0:s0 + 128], gp._x), B[s0:s0 + 128])
                        return g

                    row["today_value_ms"] = _time(value, 3, 1)
                    row["today_gradient_matrix_ms"] = _time(grad_matrix, 3, 1) if n <= 4096 else _time(grad_matrix, 1, 0)
                    row["today_gradient_ms"] = _time(grad_full, 3, 1) if n <= 4096 else _time(grad_full, 1, 0)
                    keep.clear()
            print(json.dumps(row), flush=True)
            out.append(row)
            del gp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo", "loo_time.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--kernels", default="expsq,hyper")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true", help="(internal) time the importable package's likelihood calls, print JSON")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    names = a.kernels.split(",")
    if a.child:
        rows = measure(names, sizes, a.reps, a.warmup, loo=False)
        print("RESULT " + json.dumps(rows))
        return
    sys.path.insert(0, ROOT)
    rows = measure(names, sizes, a.reps, a.warmup, loo=True)
    parent = None
    if a.parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", a.sizes, "--kernels", a.kernels,
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        txt = subprocess.run(cmd, env=env, cwd=os.path.abspath(a.parent), check=True, stdout=subprocess.PIPE).stdout.decode()
        parent = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for row, prow in zip(rows, parent):
            assert (row["kernel"], row["n"]) == (prow["kernel"], prow["n"])
            row["parent"] = {k: prow[k] for k in ("compute_ms", "nll_ms", "nll_and_grad_ms")}
            row["ratio_loo_grad_over_parent_nll_and_grad"] = row["loo_nll_and_grad_ms"]["median"] / prow["nll_and_grad_ms"]["median"]
            row["ratio_loo_value_over_parent_compute"] = row["loo_log_likelihood_ms"]["median"] / prow["compute_ms"]["median"]
    import george_amd
    doc = dict(what="wall clock, ms: GP.loo_log_likelihood on a computed GP and GP.loo_nll_and_grad at a new parameter vector, "
                    "beside compute / nll / nll_and_grad of this build and of the parent commit's build in the same session",
               method="median of %d calls after %d warm-ups, min .. max kept" % (a.reps, a.warmup),
               devices=george_amd.device_count(), parent_build=bool(parent), results=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
