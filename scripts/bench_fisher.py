#!/usr/bin/env python3
"""Wall clock of GP.fisher_information on the dense solver, beside the host route it replaces and nll_and_grad as a scale.

Quantity   GP.fisher_information() on a computed GP (gh_chol_fisher: L^-1, two triangular GEMMs per kernel parameter, the
           pair contraction); GP.nll_and_grad(p, y) at a new p of the same build as a scale; and the host route, which uses
           only interfaces the parent commit has: ``solver.get_inverse()`` to the host, ``kernel.get_gradient(x)``, one
           ``Kinv @ G[:, :, p]`` per parameter and the pairwise ``einsum`` -- timed in THIS build and, with ``--parent DIR``
           (a directory that holds a built checkout of the parent commit), in the parent's by a child process in the same
           session.
Method     median of 20 calls after 3 warm-ups, min .. max kept (a quarter of the calls above N = 16 384); the host route
           median of 3 after a warm-up at N = 4096, ONE call without warm-up above, and only where its (N, N, P) host tensor
           stays under ``--host-bytes`` (8 GB).
Sizes      N = 4096, 16 384, 32 768 on 1-D ExpSquared (2 parameters) and on the hyper.rst composite (11 parameters).

Products   what chose the product form: per size the GEMMs of one kernel parameter alone on the chip
           through gh_dev_gemm, HIP events, median of ``--reps`` launches, forms alternated -- the full product K^-1 D of the
           non-symmetric form against the two triangular ones of W = (L^-1 D) L^-T (lower tiles with k <= row, then k <= column).

Writes profiles/fisher/time.json (``--out``).  Expectation from flop counts, not from a run: N^3 multiply-adds per kernel
parameter in two triangular products, roughly 0.06-0.12 s per parameter at N = 16 384."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 16384, 32768)


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


def product_forms(sizes, reps):
    """ms of the GEMMs of ONE kernel parameter in the two forms, on random operands of the right shapes"""
    import ctypes as C
    import torch
    from george_amd import _native as N
    dp = C.POINTER(C.c_double)
    LOWER, B_NMAJOR, KHI_COL, KHI_ROW = 4, 2, 16, 32
    out = []
    for n in sizes:
        a, b, c = (torch.randn(n, n, dtype=torch.float64, device="cuda") for _ in range(3))
        ptr = lambda t: C.cast(t.data_ptr(), dp)                      # noqa: E731
        forms = dict(full_Kinv_D=B_NMAJOR, tri_Linv_D=B_NMAJOR | LOWER | KHI_ROW, tri_T_LinvT=LOWER | KHI_COL)
        ms = {k: [] for k in forms}
        for rep in range(reps + 1):
            for name, flags in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                N.check(N.lib.gh_dev_gemm(ptr(c), n, ptr(a), n, ptr(b), n, n, n, n, 1.0, 0.0, flags, None))
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[name].append(e0.elapsed_time(e1))
        row = dict(n=n, launches=reps)
        row.update({k + "_ms": float(np.median(v)) for k, v in ms.items()})
        row["symmetric_over_full"] = (row["tri_Linv_D_ms"] + row["tri_T_LinvT_ms"]) / row["full_Kinv_D_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
        del a, b, c
    return out


def host_route(gp):
    """F over the kernel parameters from interfaces every build has (the NumPy branch of GP.fisher_information)"""
    Kinv = gp.solver.get_inverse()
    G = gp.kernel.get_gradient(gp._x)
    M = np.stack([np.dot(Kinv, G[:, :, p]) for p in range(G.shape[2])])
    return 0.5 * np.einsum("aij,bji->ab", M, M)


def measure(names, sizes, reps, warm, host_bytes, fisher):
    """the timings of the package that is importable right now (``fisher``: it has GP.fisher_information)"""
    from george_amd import GP, kernels
    out = []
    for name in names:
        for n in sizes:
            x, yerr, y = _data(name, n)
            gp = GP(_kernel(name, kernels, y))
            gp.compute(x, yerr)
            p0 = gp.get_parameter_vector()
            fresh = lambda i: p0 + 1e-9 * (1 + i % 2)                 # noqa: E731  (never the vector just computed)
            row = dict(kernel=name, n=n, parameters=len(p0))
            r = reps if n <= 16384 else max(3, reps // 4)
            gp._grad_seen = False
            row["nll_and_grad_ms"] = _time(lambda i: gp.nll_and_grad(fresh(i), y), r, warm)
            gp.compute(x, yerr)
            F = None
            if fisher:
                row["fisher_information_ms"] = _time(lambda i: gp.fisher_information(), r, warm)
                F = gp.fisher_information()
            if 8 * n * n * len(p0) <= host_bytes:
                keep = {}

                def host(i):
                    keep["F"] = host_route(gp)

                row["host_route_ms"] = _time(host, 3, 1) if n <= 4096 else _time(host, 1, 0)
                if F is not None:
                    d = np.sqrt(np.diag(F))
                    row["host_route_max_difference_over_sqrt_FaaFbb"] = float(np.max(np.abs(keep["F"] - F) / np.outer(d, d)))
            print(json.dumps(row), flush=True)
            out.append(row)
            del gp
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisher", "time.json"))
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--kernels", default="expsq,hyper")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-bytes", type=float, default=8e9, help="largest (N, N, P) host tensor the host route is timed with")
    ap.add_argument("--child", action="store_true", help="(internal) time the importable package's host route, print JSON")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    names = a.kernels.split(",")
    if a.child:
        rows = measure(names, sizes, a.reps, a.warmup, a.host_bytes, fisher=False)
        print("RESULT " + json.dumps(rows))
        return
    sys.path.insert(0, ROOT)
    rows = measure(names, sizes, a.reps, a.warmup, a.host_bytes, fisher=True)
    forms = product_forms([n for n in sizes if n <= 16384], a.reps)
    parent = None
    if a.parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--sizes", a.sizes, "--kernels", a.kernels,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--host-bytes", str(a.host_bytes)]
        txt = subprocess.run(cmd, env=env, cwd=os.path.abspath(a.parent), check=True, stdout=subprocess.PIPE).stdout.decode()
        parent = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for row, prow in zip(rows, parent):
            assert (row["kernel"], row["n"]) == (prow["kernel"], prow["n"])
            row["parent"] = {k: prow[k] for k in ("nll_and_grad_ms", "host_route_ms") if k in prow}
    import george_amd
    doc = dict(what="wall clock, ms: GP.fisher_information on a computed GP, beside nll_and_grad at a new parameter vector and "
                    "the host route (get_inverse + get_gradient + NumPy products) of this build and of the parent commit's "
                    "build in the same session",
               method="median of %d calls after %d warm-ups (a quarter of the calls above N = 16384), min .. max kept; the host "
                      "route: median of 3 after a warm-up at N = 4096, one call above" % (a.reps, a.warmup),
               devices=george_amd.device_count(), parent_build=bool(parent), results=rows, product_forms=forms)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
