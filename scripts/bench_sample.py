#!/usr/bin/env python3
"""Wall clock of drawing from a fitted GP: ``factor="cholesky"`` (pivoted Cholesky on the device) beside ``factor="svd"``
(the reference's path: the covariance to the host, ``np.random.multivariate_normal``).

Quantity   GP.sample_conditional(y, t, size=16) on a computed GP at N = 4096, M in {256, 1024, 4096}, both factors;
           GP.sample_conditional_batch(vectors, y, t, size=16) at (N, M, B) = (468, 250, 50) and (1024, 250, 36), both factors;
           the split of the single device call: ``predict(return_cov=True)`` alone, ``gh_dev_pstrf`` alone on that covariance
           (device pointers), and the remainder (normals to the device, the GEMM, draws back);
           the "svd" path again on a build of the PARENT commit (``--parent DIR``, timed by a child process in the same
           session): the yardstick that the keyword changed nothing there.
Method     median of 20 calls after 3 warm-ups, min .. max kept.  The SVD path at M = 4096 takes seconds per call: 3 calls
           after 1 warm-up there, and said so in the row.
Model      for M > 512 the factor runs in panels of 128 pivots: one workgroup per member and panel, left-looking inside the
           panel, one K = 128 GEMM per full panel.  Predicted from the operation count, not measured: the panels read
           128 * 127 / 2 * m * 8 bytes of factor columns each, about 508 m^2 bytes in all, and the GEMMs read and write the
           padded matrix once per panel, m / 128 * 16 m^2 bytes; a launch-per-column left-looking form would read the
           factor's columns 4 m^3 bytes in total.  Both predictions are written beside the measured full-rank time.

Writes profiles/sample/sample_time.json (``--out``).  No ratio is fixed in advance: the ratios are what is measured."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ((4096, 256), (4096, 1024), (4096, 4096))
BATCH = ((468, 250, 50), (1024, 250, 36))
SIZE = 16


def _time(fn, reps, warm):
    for i in range(warm):
        fn(i)
    ts = []
    for i in range(reps):
        t0 = time.perf_counter()
        fn(warm + i)
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), calls=reps)


def _problem(n):
    from george_amd import GP, kernels
    rng = np.random.RandomState(n)
    x = np.sort(rng.uniform(0.0, 10.0, n))
    y = np.sin(x) + 0.1 * rng.randn(n)
    gp = GP(float(np.var(y)) * kernels.ExpSquaredKernel(1.0), white_noise=np.log(0.01), fit_white_noise=True)
    gp.compute(x, 0.1)
    return gp, x, y, rng


def measure(reps, warm, cholesky, single, batch):
    """the timings of the package that is importable right now (``cholesky``: it has the keyword)"""
    rows = []
    for n, m in single:
        gp, x, y, rng = _problem(n)
        t = np.linspace(0.0, 10.0, m)
        row = dict(call="sample_conditional", n=n, m=m, size=SIZE)
        slow = m >= 4096
        row["svd_ms"] = _time(lambda i: gp.sample_conditional(y, t, SIZE), 3 if slow else reps, 1 if slow else warm)
        if cholesky:
            import torch
            from george_amd import _native as N
            row["cholesky_ms"] = _time(lambda i: gp.sample_conditional(y, t, SIZE, factor="cholesky"), reps, warm)
            row["predict_cov_ms"] = _time(lambda i: gp.predict(y, t, return_cov=True), reps, warm)
            mu, cov = gp.predict(y, t, return_cov=True)
            cd = torch.from_numpy(cov).cuda()
            work = torch.empty_like(cd)
            fac = torch.empty_like(cd)
            piv = torch.zeros(m, dtype=torch.int64, device="cuda")
            rank = torch.zeros(1, dtype=torch.int64, device="cuda")
            tol = m * np.finfo(np.float64).eps * float(np.max(gp.kernel.get_value(gp.parse_samples(t), diag=True)))

            def factor(i):
                work.copy_(cd)
                N.check(N.lib.gh_dev_pstrf(work.data_ptr(), m, m * m, m, 1, tol, fac.data_ptr(), m, m * m, piv.data_ptr(),
                                           rank.data_ptr(), None, None))
                torch.cuda.synchronize()

            row["factor_ms"] = _time(factor, reps, warm)
            row["rank"] = int(rank.cpu()[0])
            row["draws_and_copies_ms"] = row["cholesky_ms"]["median"] - row["predict_cov_ms"]["median"] - row["factor_ms"]["median"]
            # a full-rank factor of the same size (K(t, t) + I): every panel and every GEMM runs
            full = torch.from_numpy(gp.get_matrix(t) + np.eye(m)).cuda()

            def factor_full(i):
                work.copy_(full)
                N.check(N.lib.gh_dev_pstrf(work.data_ptr(), m, m * m, m, 1, -1.0, fac.data_ptr(), m, m * m, piv.data_ptr(),
                                           rank.data_ptr(), None, None))
                torch.cuda.synchronize()

            row["factor_full_rank_ms"] = _time(factor_full, 5 if slow else reps, 1)
            row["full_rank"] = int(rank.cpu()[0])
            if m > 512:
                row["panel_form_bytes_predicted"] = (128 * 127 / 2 * 8 / 128.0 + 16.0 * m / 128.0) * float(m) ** 2
                row["per_column_form_bytes_predicted"] = 4.0 * float(m) ** 3
            row["speedup_over_svd"] = row["svd_ms"]["median"] / row["cholesky_ms"]["median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del gp
    for n, m, B in batch:
        gp, x, y, rng = _problem(n)
        t = np.linspace(0.0, 10.0, m)
        vec = gp.get_parameter_vector() + 1e-2 * rng.randn(B, len(gp))
        row = dict(call="sample_conditional_batch", n=n, m=m, B=B, size=SIZE)
        row["svd_ms"] = _time(lambda i: gp.sample_conditional_batch(vec, y, t, SIZE), 5, 1)
        if cholesky:
            row["cholesky_ms"] = _time(lambda i: gp.sample_conditional_batch(vec, y, t, SIZE, factor="cholesky"), reps, warm)
            row["predict_batch_cov_ms"] = _time(lambda i: gp.predict_batch(vec, y, t, return_cov=True), reps, warm)
            row["speedup_over_svd"] = row["svd_ms"]["median"] / row["cholesky_ms"]["median"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del gp
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample", "sample_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-m", type=int, default=4096, help="leave out the single-call shapes above this M")
    ap.add_argument("--child", action="store_true", help="(internal) time the importable package's svd path, print JSON")
    a = ap.parse_args()
    single = [s for s in SINGLE if s[1] <= a.max_m]
    if a.child:
        print("RESULT " + json.dumps(measure(a.reps, a.warmup, False, single, BATCH)))
        return
    sys.path.insert(0, ROOT)
    rows = measure(a.reps, a.warmup, True, single, BATCH)
    parent = None
    if a.parent:
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--max-m", str(a.max_m)]
        txt = subprocess.run(cmd, env=env, cwd=os.path.abspath(a.parent), check=True, stdout=subprocess.PIPE).stdout.decode()
        parent = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
        for row, prow in zip(rows, parent):
            assert (row["call"], row["n"], row["m"]) == (prow["call"], prow["n"], prow["m"])
            row["parent_svd_ms"] = prow["svd_ms"]
    import george_amd
    doc = dict(what="wall clock, ms: GP.sample_conditional / GP.sample_conditional_batch with factor='cholesky' (device) beside "
                    "factor='svd' (host) of this build and of the parent commit's build in the same session; size = 16",
               method="median of %d calls after %d warm-ups, min .. max kept (the svd path: 3 calls after 1 warm-up at "
                      "M = 4096, 5 after 1 for the batches)" % (a.reps, a.warmup),
               devices=george_amd.device_count(), parent_build=bool(parent), max_m=a.max_m, results=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote " + a.out)


if __name__ == "__main__":
    main()
