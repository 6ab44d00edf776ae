"""Accuracy and timing of ``InducingSolver`` beside ``VecchiaSolver`` and the dense solver: the tables of the README.

``--what accuracy`` (CPU only): on the three problems of ``scripts/bench_vecchia.py --what accuracy`` (N = 2000, seed 2000, error
bars 0.1) the DTC and FITC log-likelihood of the NumPy restatement (tests/inducing_ref.py) at m = 32 .. 512 max-min inducing
points and relative jitter 1e-10, against the dense one, with the Vecchia restatement at m = 64 beside it.  Writes
``profiles/inducing/accuracy.json``.

``--what time`` (on an MI355X): medians of ``--reps`` calls (min .. max kept) of ``compute`` + log-likelihood, ``GP.nll_and_grad``
and ``GP.predict`` with the variance at 1000 points, for m in ``--m`` (256, 1024, 4096) and N in ``--n`` (16384 .. 1048576) in
1-D and 3-D -- the problems of ``scripts/bench_vecchia.py --what time`` -- beside ``VecchiaSolver(m=64)`` and, up to
``--dense-max`` points, ``BasicSolver`` of the same build.  The host's max-min selection is timed on its own (``select_s``) and is
not in those numbers.  Writes ``profiles/inducing/time.json``.

    python scripts/bench_inducing.py --what accuracy
    python scripts/bench_inducing.py --what time [--n 16384,65536] [--m 256,1024] [--dims 1,3] [--reps 20] [--out ...]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import george_amd  # noqa: E402
from george_amd import GP, BasicSolver, InducingSolver, VecchiaSolver, kernels  # noqa: E402
from george_amd.solvers.inducing import inducing_points  # noqa: E402
from george_amd.solvers.vecchia import vecchia_neighbors  # noqa: E402

ACCURACY_CASES = ("1-D Matern-3/2", "1-D ExpSquared", "2-D ExpSquared")


def accuracy_problems():
    """the three problems of bench_vecchia.py's accuracy table, drawn in its order: (name, kernel, x, y)"""
    n = 2000
    rng = np.random.RandomState(2000)
    x1 = np.sort(rng.uniform(0, 10, n))[:, None]
    x2 = rng.uniform(0, 2, (n, 2))
    x2 = x2[np.argsort(x2[:, 0], kind="stable")]
    cases = [("1-D Matern-3/2", 1.0 * kernels.Matern32Kernel(1.0), x1), ("1-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(1.0), x1),
             ("2-D ExpSquared", 1.0 * kernels.ExpSquaredKernel(0.25, ndim=2), x2)]
    return [(name, kernel, x, np.sin(3.0 * x.sum(axis=1)) + 0.1 * rng.randn(n)) for name, kernel, x in cases]


def run_accuracy(cases=ACCURACY_CASES, ms=(32, 64, 128, 256, 512), jitter=1e-10):
    from scipy.linalg import cho_factor, cho_solve
    from oracle import solver_np
    import inducing_ref
    import vecchia_ref
    rows = []
    for name, kernel, x, y in accuracy_problems():
        if name not in cases:
            continue
        n = len(x)
        K = solver_np.kernel_matrix(kernel, x)
        K[np.diag_indices_from(K)] += 0.01
        cf = cho_factor(K, lower=True)
        ll_dense = -0.5 * (np.dot(y, cho_solve(cf, y)) + 2.0 * np.sum(np.log(np.diag(cf[0]))) + n * np.log(2 * np.pi))
        ll_v = vecchia_ref.reference(kernel, x, 0.1, vecchia_neighbors(x, 64), r=y).log_likelihood()
        for m in ms:
            u = x[inducing_points(x, m)]
            jit = jitter * float(np.mean(solver_np.kernel_matrix(kernel, u, diag=True)))
            row = dict(case=name, n=n, m=m, jitter=jitter, ll_dense=float(ll_dense), ll_vecchia_m64=float(ll_v),
                       rel_diff_vecchia_m64=float(abs(ll_v - ll_dense) / abs(ll_dense)))
            for method in ("dtc", "fitc"):
                ll = inducing_ref.reference(kernel, x, 0.1, u, jit, method, r=y).log_likelihood()
                row["ll_" + method] = float(ll)
                row["rel_diff_" + method] = float(abs(ll - ll_dense) / abs(ll_dense))
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return dict(ms=1e3 * float(np.median(ts)), ms_min=1e3 * float(np.min(ts)), ms_max=1e3 * float(np.max(ts))), out


def time_solver(label, make_kernel, solver, kw, x, yerr, y, t, args, extra):
    rows = []
    n = len(x)

    def compute_ll():
        s = solver(make_kernel(), **kw)
        s.compute(x, yerr)
        return -0.5 * (s.dot_solve(y) + s.log_determinant + n * np.log(2 * np.pi))

    base = dict(solver=label, n=n, ndim=x.shape[1], **extra)
    tm, ll = timed(compute_ll, args.warmup, args.reps)
    rows.append(dict(base, op="compute_ll", ll=float(ll), **tm))
    gp = GP(make_kernel(), solver=solver, **kw)
    gp.compute(x, yerr)
    p0 = gp.get_parameter_vector()
    count = [0]

    def nll_grad():
        count[0] += 1
        return gp.nll_and_grad(p0 + 1e-6 * (count[0] % 7), y)

    if not (label == "BasicSolver" and n > args.dense_grad_max):
        tm, _ = timed(nll_grad, args.warmup, args.reps)
        rows.append(dict(base, op="nll_grad", **tm))
    gp.set_parameter_vector(p0)
    gp.compute(x, yerr)
    tm, _ = timed(lambda: gp.predict(y, t, return_var=True), args.warmup, args.reps)
    rows.append(dict(base, op="predict", m_test=len(t), **tm))
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def run_time(args, save):
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_inducing.py --what time needs an MI355X")
    from bench_vecchia import problem
    rows = []
    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            t = x[np.random.RandomState(7).choice(n, 1000, replace=False)] + 1e-3
            if n <= args.dense_max:
                rows += time_solver("BasicSolver", make_kernel, BasicSolver, {}, x, yerr, y, t, args, {})
                BasicSolver.release_pool()
            VecchiaSolver(make_kernel(), m=64)._default_table(x)              # (kept by the class: the timed calls find it)
            rows += time_solver("VecchiaSolver", make_kernel, VecchiaSolver, dict(m=64), x, yerr, y, t, args, dict(m=64))
            VecchiaSolver.release_pool()
            save(rows)
            for m in args.m:
                if m > n:
                    continue
                t0 = time.perf_counter()
                InducingSolver(make_kernel(), inducing=m)._default_points(x)  # (kept by the class: the timed calls find it)
                select_s = time.perf_counter() - t0
                for method in args.methods:
                    rows += time_solver("InducingSolver", make_kernel, InducingSolver, dict(inducing=m, method=method, jitter=args.jitter),
                                        x, yerr, y, t, args, dict(m=m, method=method, select_s=select_s))
                    InducingSolver.release_pool()
                    save(rows)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="time", choices=["time", "accuracy"])
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[16384, 65536, 262144, 1048576])
    ap.add_argument("--m", type=ints, default=[256, 1024, 4096])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--methods", type=lambda s: s.split(","), default=["fitc"])
    ap.add_argument("--jitter", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dense-max", type=int, default=65536)
    ap.add_argument("--dense-grad-max", type=int, default=16384)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", "inducing", "time.json" if args.what == "time" else "accuracy.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)

    def save(rows):                                   # (after every configuration: a run that is cut short keeps what it measured)
        with open(out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")

    save(run_time(args, save) if args.what == "time" else run_accuracy())


if __name__ == "__main__":
    main()
