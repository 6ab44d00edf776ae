#!/usr/bin/env python3
"""Wall clock of leave-group-out cross-validation on the dense solver, beside leave-one-out and the loop of refits.

Quantity   GP.lgo_log_likelihood(y, b) on a computed GP (the value path) and GP.lgo_nll_and_grad(p, y, b) at a new p
           (recompute + one gh_chol_lgo call), windows of b = 16 / 64 / 128 consecutive points;
           beside them GP.loo_log_likelihood and GP.loo_nll_and_grad of THIS build, and -- ``--parent DIR``, a directory that
           holds a built checkout of the parent commit -- the route a user had before, timed by a child process in the same
           session: for every window ``compute`` on the kept points + ``predict`` of the window with ``return_cov``.  The
           loop is timed over ``--refits`` windows (default 8, spread over the data) and scaled to all G of them.
Method     median of 20 calls after 3 warm-ups, min .. max kept; every optimiser call gets a parameter vector it has not just
           seen.
Sizes      N = 4096, 16 384 on 1-D ExpSquared.

Writes profiles/lgo/time.json (``--out``).  No speed threshold is fixed in advance."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 16384)
WINDOWS = (16, 64, 128)


def _data(n):
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0.0, n / 70.0, n))
    return x, 0.1 + 0.05 * rng.rand(n), np.sin(x) + 0.1 * rng.randn(n)


def _time(fn, reps, warm):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warm + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), calls=reps)


def _refit_loop(sizes, windows, refits):
    """the importable package's compute-on-the-kept-points + predict, per window: what the parent commit offers"""
    from george_amd import GP, kernels
    rows = []
    for n in sizes:
        x, yerr, y = _data(n)
        for b in windows:
            G = -(-n // b)
            picks = np.unique(np.linspace(0, G - 1, min(refits, G)).astype(int))
            gp = GP(float(np.var(y)) * kernels.ExpSquaredKernel(1.0))

            def one(g):
                keep = np.ones(n, dtype=bool)
                keep[g * b:(g + 1) * b] = False
                gp.compute(x[keep], yerr[keep])
                return gp.predict(y[keep], x[~keep], return_cov=True)

            one(int(picks[0]))                            # warm-up
            ts = []
            for g in picks:
                t0 = time.perf_counter()
                one(int(g))
                ts.append((time.perf_counter() - t0) * 1e3)
            rows.append(dict(n=n, window=b, groups=G, refits_timed=len(picks), per_refit_ms=float(np.median(ts)),
                             loop_ms=float(np.median(ts)) * G))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--windows", default=",".join(str(w) for w in WINDOWS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--refits", type=int, default=8)
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lgo", "time.json"))
    ap.add_argument("--child", action="store_true", help="(internal) time the importable package's refit loop, print JSON")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    windows = [int(w) for w in a.windows.split(",")]
    if a.child:
        print("RESULT " + json.dumps(_refit_loop(sizes, windows, a.refits)))
        return
    sys.path.insert(0, ROOT)
    import george_amd
    from george_amd import GP, kernels
    rows = []
    for n in sizes:
        x, yerr, y = _data(n)
        gp = GP(float(np.var(y)) * kernels.ExpSquaredKernel(1.0))
        gp.compute(x, yerr)
        p0 = gp.get_parameter_vector()
        row = dict(n=n, loo_log_likelihood_ms=_time(lambda i: gp.loo_log_likelihood(y), a.reps, 3),
                   loo_nll_and_grad_ms=_time(lambda i: gp.loo_nll_and_grad(p0 + 1e-4 * (i + 1), y), a.reps, 3), windows=[])
        for b in windows:
            gp.set_parameter_vector(p0)
            gp.compute(x, yerr)
            w = dict(window=b, groups=-(-n // b),
                     lgo_log_likelihood_ms=_time(lambda i: gp.lgo_log_likelihood(y, b), a.reps, 3),
                     lgo_nll_and_grad_ms=_time(lambda i: gp.lgo_nll_and_grad(p0 + 1e-4 * (i + 1), y, b), a.reps, 3))
            w["ratio_value_over_loo"] = w["lgo_log_likelihood_ms"]["median"] / row["loo_log_likelihood_ms"]["median"]
            w["ratio_grad_over_loo"] = w["lgo_nll_and_grad_ms"]["median"] / row["loo_nll_and_grad_ms"]["median"]
            row["windows"].append(w)
            print("N=%d window %d: value %.2f ms (loo %.2f), value + gradient %.2f ms (loo %.2f)"
                  % (n, b, w["lgo_log_likelihood_ms"]["median"], row["loo_log_likelihood_ms"]["median"],
                     w["lgo_nll_and_grad_ms"]["median"], row["loo_nll_and_grad_ms"]["median"]), flush=True)
        rows.append(row)
    parent = None
    if a.parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", a.sizes, "--windows", a.windows,
               "--refits", str(a.refits)]
        txt = subprocess.run(cmd, env=env, cwd=os.path.abspath(a.parent), check=True, stdout=subprocess.PIPE).stdout.decode()
        parent = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for row in rows:
            for w in row["windows"]:
                for prow in parent:
                    if prow["n"] == row["n"] and prow["window"] == w["window"]:
                        w["parent_refit_loop"] = prow
                        w["ratio_refit_loop_over_value"] = prow["loop_ms"] / w["lgo_log_likelihood_ms"]["median"]
    out = dict(what="GP.lgo_log_likelihood / GP.lgo_nll_and_grad (median of %d calls, ms) beside loo_* of this build%s"
                    % (a.reps, " and the loop of G refits on the parent commit's build in the same session" if parent else ""),
               devices=george_amd.device_count(), parent_build=bool(parent), results=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
