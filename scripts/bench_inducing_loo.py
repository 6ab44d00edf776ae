"""Timing of ``InducingSolver.loo_lowrank`` (gh_inducing_loo), leave-one-out cross-validation of the DTC / FITC density.  Needs
an MI355X.  Writes ``profiles/inducing/loo_time.json``.

Wall-clock medians (with minimum and maximum) of ``--reps`` (20) calls after ``--warmup`` (2) of

    loo_values   ``solver.loo_lowrank(r)`` on a computed solver: the seven-tuple's values, no gradient
    loo_grad     ``solver.loo_lowrank(r, which)`` with every kernel parameter: values, gradient, ``v`` and ``diagB``
    dot_solve    ``solver.dot_solve(r)`` on the same solver: by operation count ``loo_values`` is about one of these plus one strip pass
    grad         ``solver.grad(r, which)`` on the same solver: by operation count ``loo_grad`` is between two and three of these
    nll_grad     ``GP.nll_and_grad`` of the same build in the same session, at a parameter vector that changes from call to call:
                 the yardstick -- one ``compute`` and one ``grad``

for N in ``--n`` (16384, 65536) and m in ``--m`` (256, 1024) in ``--dims`` (1, 3): the problems of
``scripts/bench_inducing.py --what time``, FITC, relative jitter 1e-8.  Every call returns host values, so the device work has
ended when the clock stops.  The host's max-min selection is not in these numbers.

At N = ``--dense-n`` (4096), where the generic branch of ``GP`` still fits, also ``GP.loo_log_likelihood`` and
``GP.grad_loo_log_likelihood`` with ``InducingSolver`` (m = 256) of this build and -- ``--parent DIR``, a built checkout of the
parent commit -- of that build, which takes the NumPy branch on ``get_inverse()`` (and whose gradient is not the derivative of
its value): timed by a child process in the same session, ``--parent-reps`` (5) calls after one.

    python scripts/bench_inducing_loo.py [--n 16384,65536] [--m 256,1024] [--dims 1,3] [--reps 20] [--parent DIR] [--out ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.environ.get("BENCH_INDUCING_LOO_CHILD"):
    sys.path.insert(0, ROOT)                          # (the child imports the package of its PYTHONPATH)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import george_amd  # noqa: E402
from george_amd import GP, InducingSolver  # noqa: E402

from bench_vecchia import problem  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), reps=reps), out


def gp_rows(args, reps, warmup, label):
    """``GP.loo_log_likelihood`` and ``GP.grad_loo_log_likelihood`` at N = --dense-n, m = 256, with whatever package is imported"""
    rows = []
    n, m = args.dense_n, 256
    for ndim in (1, 3):
        make_kernel, x, yerr, y = problem(ndim, n)
        gp = GP(make_kernel(), solver=InducingSolver, inducing=m, method="fitc", jitter=args.jitter)
        gp.compute(x, yerr)
        route = "loo_lowrank" if callable(getattr(gp.solver, "loo_lowrank", None)) else "generic"
        for op, fn in (("GP.loo_log_likelihood", lambda: gp.loo_log_likelihood(y)), ("GP.grad_loo_log_likelihood", lambda: gp.grad_loo_log_likelihood(y))):
            t, out = timed(fn, warmup, reps)
            rows.append(dict(t, build=label, route=route, op=op, ndim=ndim, n=n, m=m,
                             value=float(out) if np.ndim(out) == 0 else [float(v) for v in out]))
            print(json.dumps(rows[-1]), flush=True)
        del gp
    return rows


def run(args, save):
    rows = []
    for ndim in args.dims:
        for n in args.n:
            make_kernel, x, yerr, y = problem(ndim, n)
            for m in args.m:
                if m > n:
                    continue
                InducingSolver(make_kernel(), inducing=m)._default_points(x)  # (kept by the class: the timed calls find it)
                base = dict(solver="InducingSolver", method="fitc", jitter=args.jitter, ndim=ndim, n=n, m=m)
                s = InducingSolver(make_kernel(), inducing=m, method="fitc", jitter=args.jitter)
                s.compute(x, yerr)
                ones = np.ones(len(s.kernel), dtype=np.uint32)
                tv, vals = timed(lambda: s.loo_lowrank(y), args.warmup, args.reps)
                tg, _ = timed(lambda: s.loo_lowrank(y, ones), args.warmup, args.reps)
                td, _ = timed(lambda: s.dot_solve(y), args.warmup, args.reps)
                tk, _ = timed(lambda: s.grad(y, ones), args.warmup, args.reps)
                rows.append(dict(tv, op="loo_values", L=vals[0], loo_values_over_dot_solve=tv["ms"] / td["ms"], **base))
                rows.append(dict(tg, op="loo_grad", parameters=len(ones), loo_grad_over_grad=tg["ms"] / tk["ms"], **base))
                rows.append(dict(td, op="dot_solve", **base))
                rows.append(dict(tk, op="grad", **base))
                del s
                gp = GP(make_kernel(), solver=InducingSolver, inducing=m, method="fitc", jitter=args.jitter)
                gp.compute(x, yerr)
                p0 = gp.get_parameter_vector()
                count = [0]

                def nll_grad():
                    count[0] += 1
                    return gp.nll_and_grad(p0 + 1e-6 * (count[0] % 7), y)

                t, _ = timed(nll_grad, args.warmup, args.reps)
                rows.append(dict(t, op="nll_grad", loo_grad_over_nll_grad=tg["ms"] / t["ms"], loo_values_over_nll_grad=tv["ms"] / t["ms"], **base))
                for row in rows[-5:]:
                    print(json.dumps(row), flush=True)
                del gp
                InducingSolver.release_pool()
                save(rows)
    if args.dense_n:
        rows += gp_rows(args, args.reps, args.warmup, "this")
        save(rows)
        if args.parent:
            env = dict(os.environ, PYTHONPATH=os.path.abspath(args.parent), BENCH_INDUCING_LOO_CHILD="1")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dense-n", str(args.dense_n), "--parent-reps", str(args.parent_reps),
                   "--jitter", repr(args.jitter)]
            txt = subprocess.run(cmd, env=env, cwd=os.path.abspath(args.parent), check=True, stdout=subprocess.PIPE).stdout.decode()
            parent = json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][7:])
            assert all(row["route"] == "generic" for row in parent), "the parent build has loo_lowrank: not the parent commit"
            for row in parent:
                mine = [q for q in rows if q.get("build") == "this" and q["op"] == row["op"] and q["ndim"] == row["ndim"]][0]
                row["parent_over_this"] = row["ms"] / mine["ms"]
                print(json.dumps(row), flush=True)
            rows += parent
            save(rows)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ints = lambda s: [int(v) for v in s.split(",") if v]          # noqa: E731
    ap.add_argument("--n", type=ints, default=[16384, 65536])
    ap.add_argument("--m", type=ints, default=[256, 1024])
    ap.add_argument("--dims", type=ints, default=[1, 3])
    ap.add_argument("--jitter", type=float, default=1e-8)
    ap.add_argument("--dense-n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--parent-reps", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="(the child's mode) time the generic branch of the importable package")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inducing", "loo_time.json"))
    args = ap.parse_args()
    if george_amd.device_count() <= 0:
        raise SystemExit("bench_inducing_loo.py needs an MI355X")
    if args.child:
        print("RESULT " + json.dumps(gp_rows(args, args.parent_reps, 1, "parent")), flush=True)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save(rows):                                   # (after every configuration: a run that is cut short keeps what it measured)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")

    save(run(args, save))


if __name__ == "__main__":
    main()
