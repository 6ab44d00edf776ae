"""Timing of ``VecchiaSolver`` against the solvers that existed before it, and the accuracy table of the README.

``--what time`` (needs an MI355X): wall-clock medians of ``--reps`` (20) calls after ``--warmup`` (2) of

    compute_ll   ``solver.compute(x, yerr)`` + the log-likelihood from ``dot_solve`` and ``log_determinant``
    nll_grad     ``GP.nll_and_grad`` at a parameter vector that changes from call to call (a new factorisation per call)
    predict      ``GP.predict(y, t, return_var=True)`` at M = 1000 test points on a computed GP

for N in ``--n`` (16384, 65536, 262144, 1048576), 1-D (sorted uniform points, ``var(y) * ExpSquared``) and 3-D (uniform points
sorted by their first coordinate, ``Matern52 + Constant``), m in ``--m`` (16, 32, 64).  Every call returns host values, so the
device work has ended when the clock stops.  The default neighbour table is built once per (inputs, m) outside the timed calls
(``table_s``: what that cost on the host) -- it depends on the inputs only.  Yardsticks, same process, same inputs: ``BasicSolver``
up to ``--dense-max`` points (its gradient up to ``--dense-grad-max``), and in 1-D ``HODLRSolver`` at its default tolerance up to
``--hodlr-max`` (its gradient up to ``--hodlr-grad-max``); their code is the parent commit's, unchanged.  ``ll`` is the log-likelihood each solver reports, so the table also
shows what the approximation costs in accuracy at that m.  Writes ``profiles/vecchia/time.json``.

``--what accuracy`` (CPU only): the Vecchia log-likelihood of the NumPy restatement (tests/vecchia_ref.py) against the dense
one at N = 2000, m = 8 / 16 / 32 / 64, error bars 0.1 of the amplitude.  Writes ``profiles/vecchia/accuracy.json``.

    python scripts/bench_vecchia.py --what time [--n 16384,65536] [--m 16,32,64] [--dims 1,3] [--reps 20] [--out ...]
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
from george_amd import GP, BasicSolver, HODLRSolver, VecchiaSolver, kernels  # noqa: E402
from george_amd.solvers.vecchia import vecchia_neighbors  # noqa: E402


def problem(ndim, n):
    rng = np.random.RandomState(1234)
    if ndim == 1:
        x = np.sort(rng.uniform(0, 10.0 * n / 16384.0, n))[:, None]          # a fixed point density: 1638 points per unit
        y = np.sin(x[:, 0])
        return (lambda: np.var(y) * kernels.ExpSquaredKernel(1.0)), x, 0.1 * np.ones(n), y
    x = rng.uniform(0, 1, (n, ndim)) * (n / 16384.0) ** (1.0 / ndim)
    x = x[np.argsort(x[:, 0], kind="stable")]
    y = np.sin(x.sum(axis=1))
    return (lambda: kernels.Matern52Kernel(0.5, ndim=ndim) + kernels.ConstantKernel(log_constant=np.log(0.1 / 3), ndim=ndim)), x, 0.1 * np.ones(n), y


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def time_solver(label, make_kernel, solver, kw, x, yerr, y, t, args, ops):
    """rows for one solver configuration"""
    rows = []
    n = len(x)

    def compute_ll():
        s = solver(make_kernel(), **kw)
        s.compute(x, yerr)
        return -0.5 * (s.dot_solve(y) + s.log_determinant + n * np.log(2 * np.pi))

    base = dict(solver=label, n=n, ndim=x.shape[1], **{k: v for k, v in kw.items() if k == "m"})
    if "compute_ll" in ops:
        ms, ll = timed(compute_ll, args.warmup, args.reps)
        rows.append(dict(base, op="compute_ll", ms=ms, ll=float(ll)))
    gp = GP(make_kernel(), solver=solver, **kw)
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector()
    count = [0]

    def nll_grad():
        count[0] += 1
        return gp.nll_and_grad(p0 + 1e-6 * (count[0] % 7), y)

    if "nll_grad" in ops:
        ms, _ = timed(nll_grad, args.warmup, args.reps)
        rows.append(dict(base, op="nll_grad", ms=ms))
    if "predict" in ops:
        gp.set_parameter_vector(p0)
        gp.compute(x, yerr)
        ms, _ = timed(lambda: gp.predict(y, t, return_var=True), args.warmup, args.reps)
        rows.append(dict(base, op="predict", m_test=len(t), ms=ms))
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def run_time(args, save):
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_vecchia.py --what time needs an MI355X")
    rows = []
    all_ops = ("compute_ll", "nll_grad", "predict")
    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            t = x[np.random.RandomState(7).choice(n, 1000, replace=False)] + 1e-3
            if n <= args.dense_max:
                ops = all_ops if n <= args.dense_grad_max else ("compute_ll", "predict")
                rows += time_solver("BasicSolver", make_kernel, BasicSolver, {}, x, yerr, y, t, args, ops)
                BasicSolver.release_pool()
            if ndim == 1 and n <= args.hodlr_max:
                ops = all_ops if n <= args.hodlr_grad_max else ("compute_ll", "predict")
                rows += time_solver("HODLRSolver", make_kernel, HODLRSolver, {}, x, yerr, y, t, args, ops)
                HODLRSolver.release_pool()
            save(rows)
            for m in args.m:
                t0 = time.perf_counter()
                VecchiaSolver(make_kernel(), m=m)._default_table(x)           # (kept by the class: the timed calls find it)
                table_s = time.perf_counter() - t0
                new = time_solver("VecchiaSolver", make_kernel, VecchiaSolver, dict(m=m), x, yerr, y, t, args, all_ops)
                for r in new:
                    r["table_s"] = table_s
                rows += new
                save(rows)
    return rows


def run_accuracy(args):
    from scipy.linalg import cho_factor, cho_solve
    from oracle import solver_np
    import vecchia_ref
    rows = []
    n = 2000
    rng = np.random.RandomState(2000)
    x1 = np.sort(rng.uniform(0, 10, n))[:, None]
    x2 = rng.uniform(0, 2, (n, 2))
    x2 = x2[np.argsort(x2[:, 0], kind="stable")]
    cases = [("1-D Matern-3/2", 1.0 * kernels.Matern32Kernel(1.0), x1), ("1-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(1.0), x1),
             ("2-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(0.25, ndim=2), x2)]
    for name, kernel, x in cases:
        y = np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.randn(n)
        K = solver_np.kernel_matrix(kernel, x)
        K[np.diag_indices_from(K)] += 0.01
        cf = cho_factor(K, lower=True)
        ll_dense = -0.5 * (np.dot(y, cho_solve(cf, y)) + 2.0 * np.sum(np.log(np.diag(cf[0]))) + n * np.log(2 * np.pi))
        for m in (8, 16, 32, 64):
            ref = vecchia_ref.reference(kernel, x, 0.1, vecchia_neighbors(x, m), r=y)
            rows.append(dict(case=name, n=n, m=m, ll_dense=float(ll_dense), ll_vecchia=float(ref.log_likelihood()),
                             rel_diff=float(abs(ref.log_likelihood() - ll_dense) / abs(ll_dense))))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="time", choices=["time", "accuracy"])
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[16384, 65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[16, 32, 64])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-max", type=int, default=65536)
    ap.add_argument("--dense-grad-max", type=int, default=16384)
    ap.add_argument("--hodlr-max", type=int, default=262144)
    ap.add_argument("--hodlr-grad-max", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "vecchia", "time.json" if args.what == "time" else "accuracy.json")
    before = json.load(open(out)) if args.append and os.path.exists(out) else []
    os.makedirs(os.path.dirname(out), exist_ok=True)

    def save(rows):                                   # (after every configuration: a run that is cut short keeps what it measured)
        with open(out, "w") as f:
            json.dump(before + rows, f, indent=1)
            f.write("\n")

    save(run_time(args, save) if args.what == "time" else run_accuracy(args))


if __name__ == "__main__":
    main()
