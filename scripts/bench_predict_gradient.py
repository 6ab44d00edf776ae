#!/usr/bin/env python3
"""Wall clock of the input derivatives of a fitted GP's prediction: ``GP.predict_gradient`` (one device call) beside the
host route a user had before it.

Quantity   GP.predict_gradient(y, t) (mean only) and GP.predict_gradient(y, t, return_var=True) on a computed GP at
           N in {4096, 16384, 65536}, M in {1, 64, 1024}, ndim in {1, 3}; the same with return_value=True, and GP.predict
           with the same flags beside it (the values are predict's: that call cannot cost less);
           the host route, spelled out with calls that exist at the parent commit: ``kernel.get_x1_gradient(t, x)`` to the
           host (the (M, N, ndim) tensor), ``solver.apply_inverse`` for alpha and for K^-1 K(x, t), ``np.einsum`` -- for the
           variance also the diagonal term from ``get_x1_gradient`` / ``get_x2_gradient`` at (t, t);
           the host route again on a build of the PARENT commit (``--parent DIR``, timed by a child process in the same
           session).
Method     median of 20 calls after 3 warm-ups, min .. max kept.  A host-route call whose tensor exceeds 2^27 doubles (1 GB)
           takes seconds: 3 calls after 1 warm-up there, and said so in the row.

Writes profiles/predict_gradient/time.json (``--out``).  No ratio is fixed in advance: the ratios are what is measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (4096, 16384, 65536)
MS = (1, 64, 1024)
NDIMS = (1, 3)


def _time(fn, reps, warm):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warm + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), calls=reps)


def _problem(n, ndim):
    from george_amd import GP, kernels
    rng = np.random.RandomState(n + ndim)
    if ndim == 1:
        x = np.sort(rng.uniform(0.0, 10.0, n))[:, None]
        kernel = kernels.ExpSquaredKernel(1.0)
    else:
        x = rng.uniform(0.0, 1.0, (n, ndim))
        x = x[np.argsort(x[:, 0])]
        kernel = kernels.Matern52Kernel(0.5, ndim=ndim)
    y = np.sin(x.sum(axis=1)) + 0.1 * rng.randn(n)
    gp = GP(float(np.var(y)) * kernel)
    gp.compute(x, 0.1)
    return gp, x, y, rng


def _host_route(gp, y, t, want_var):
    """what a user of the parent commit writes"""
    x, kernel = gp._x, gp.kernel
    G = kernel.get_x1_gradient(t, x)
    alpha = gp.solver.apply_inverse(np.ascontiguousarray(y - gp._call_mean(x)))
    dmu = np.einsum("cid,i->cd", G, alpha)
    if not want_var:
        return dmu
    W = gp.solver.apply_inverse(np.ascontiguousarray(kernel.get_value(x, t))).reshape(len(x), len(t))
    idx = np.arange(len(t))
    D = kernel.get_x1_gradient(t, t)[idx, idx] + kernel.get_x2_gradient(t, t)[idx, idx]
    return dmu, D - 2.0 * np.einsum("cid,ic->cd", G, W)


def measure(reps, warm, device_form, max_n):
    """the timings of the package that is importable right now (``device_form``: it has GP.predict_gradient)"""
    rows = []
    for n in [v for v in NS if v <= max_n]:
        for ndim in NDIMS:
            gp, x, y, rng = _problem(n, ndim)
            for m in MS:
                t = x[rng.randint(0, n, m)] + 0.01 * rng.randn(m, ndim)
                for want_var in (False, True):
                    row = dict(n=n, m=m, ndim=ndim, return_var=want_var, host_tensor_bytes=8 * m * n * ndim)
                    slow = m * n * ndim > (1 << 27)
                    row["host_route_ms"] = _time(lambda i: _host_route(gp, y, t, want_var), 3 if slow else reps, 1 if slow else warm)
                    if device_form:
                        row["predict_gradient_ms"] = _time(lambda i: gp.predict_gradient(y, t, return_var=want_var), reps, warm)
                        row["predict_gradient_with_value_ms"] = _time(
                            lambda i: gp.predict_gradient(y, t, return_var=want_var, return_value=True), reps, warm)
                        row["predict_ms"] = _time(lambda i: gp.predict(y, t, return_cov=False, return_var=want_var), reps, warm)
                        row["host_route_over_device"] = row["host_route_ms"]["median"] / row["predict_gradient_ms"]["median"]
                    print(json.dumps(row), flush=True)
                    rows.append(row)
            del gp
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_gradient", "time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-n", type=int, default=65536, help="leave out the sizes above this N")
    ap.add_argument("--child", action="store_true", help="(internal) time the importable package's host route, print JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.reps, a.warmup, False, a.max_n)))
        return
    sys.path.insert(0, ROOT)
    rows = measure(a.reps, a.warmup, True, a.max_n)
    parent = None
    if a.parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--max-n", str(a.max_n)]
        child = subprocess.Popen(cmd, env=env, cwd=os.path.abspath(a.parent), stdout=subprocess.PIPE, universal_newlines=True)
        for ln in child.stdout:                        # (its rows are shown as they come)
            if ln.startswith("RESULT "):
                parent = json.loads(ln[7:])
            else:
                print("parent: " + ln, end="", flush=True)
        if child.wait() != 0 or parent is None:
            raise RuntimeError("the parent build's run failed")
        for row, prow in zip(rows, parent):
            assert (row["n"], row["m"], row["ndim"], row["return_var"]) == (prow["n"], prow["m"], prow["ndim"], prow["return_var"])
            row["parent_host_route_ms"] = prow["host_route_ms"]
    import george_amd
    doc = dict(what="wall clock, ms: GP.predict_gradient (one device call) beside the host route (get_x1_gradient to the host, "
                    "apply_inverse, einsum) of this build and of the parent commit's build in the same session, and "
                    "GP.predict with the same flags",
               method="median of %d calls after %d warm-ups, min .. max kept (the host route: 3 calls after 1 warm-up where "
                      "its tensor exceeds 2^27 doubles)" % (a.reps, a.warmup),
               devices=george_amd.device_count(), parent_build=bool(parent), max_n=a.max_n, results=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
