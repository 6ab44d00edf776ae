"""Does ``VecchiaSolver.grad`` (gh_vecchia_grad) of this build give the bits of another build?  Needs an MI355X.

The triangle walk of ``vecchia_grad_kernel`` is one device function shared with ``vecchia_loo_grad_kernel`` (``v_walk``,
george_amd/csrc/gh_vecchia.hip); this script holds such a change to "not a bit": it runs ``grad`` on the problems of
tests/test_gpu_vecchia_grad.py -- every kernel of ``vecchia_cases.PCASE_NAMES`` at N = 300 with m = 7 and 64, the LDS switch
(P = 64, m = 57 / 58), N = 4099 and 8200, N = 1 / 2 / 64 / 65 -- with this build and, in a child process whose ``PYTHONPATH`` is
``--parent DIR`` (a built checkout of the parent commit), with that one, and compares ``kgrad``, ``alpha`` and ``diagA`` bit for
bit.  Prints one line per problem and ``RESULT {...}``; exit status 1 when a bit differs.

    python scripts/vecchia_grad_bits.py --parent DIR
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problems():
    import vecchia_cases as VC
    out = [(case, 300, m) for case in VC.PCASE_NAMES for m in (7, 64)]
    return out + [(64, 300, 57), (64, 300, 58), (5, 4099, 7), (5, 8200, 7), (64, 1, 64), (64, 2, 64), (64, 64, 64), (64, 65, 64), (1, 1, 64)]


def dump(path):
    """``grad`` of the importable package on every problem, into an .npz"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.append(ROOT)                             # (last: the test helpers' oracle, never the package of another build)
    import vecchia_cases as VC
    import george_amd
    from george_amd import VecchiaSolver
    out = {"package": np.array(os.path.dirname(os.path.abspath(george_amd.__file__)))}
    for case, n, m in problems():
        kernel, x, yerr, r, xs = VC.pcase(case, n)
        s = VecchiaSolver(kernel, m=m)
        s.compute(x, yerr)
        g, alpha, diagA = s.grad(r, np.ones(len(kernel), dtype=np.uint32))
        for name, val in (("kgrad", g), ("alpha", alpha), ("diagA", diagA)):
            out["%s/%d/%d/%s" % (case, n, m, name)] = val
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="directory of a built checkout of the parent commit")
    ap.add_argument("--dump", default=None, help="(the child's mode) write the results of the importable package to this file")
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
        return 0
    if not a.parent:
        ap.error("--parent DIR is needed")
    sys.path.insert(0, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        here, there = os.path.join(tmp, "this.npz"), os.path.join(tmp, "parent.npz")
        dump(here)
        env = dict(os.environ, PYTHONPATH=os.path.abspath(a.parent))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", there], env=env, cwd=os.path.abspath(a.parent), check=True)
        mine, theirs = np.load(here), np.load(there)
    assert str(mine["package"]) != str(theirs["package"]), "both runs imported the same package"
    keys = sorted(k for k in mine.files if k != "package")
    assert keys == sorted(k for k in theirs.files if k != "package")
    differ = [k for k in keys if not (np.array_equal(mine[k], theirs[k]) and np.all(np.isfinite(mine[k])))]
    for case, n, m in problems():
        tag = "%s/%d/%d/" % (case, n, m)
        print("%-16s %s" % (tag, "DIFFERS" if any(k.startswith(tag) for k in differ) else "same bits"))
    print("RESULT " + json.dumps(dict(arrays=len(keys), differ=differ, this=str(mine["package"]), parent=str(theirs["package"]))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
