"""TEST INFRASTRUCTURE ONLY.  Records what tests/test_oracle.py compares against the reference's own
kernel objects (``george.kernels``, imported by oracle/ref_loader.py from the reference sources), so that
those tests also run where the reference is absent.  Writes tests/golden/ref_objects.npz.
Run:  python -m oracle.gen_golden_refobjects
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_loader  # noqa: E402
import zoo  # noqa: E402


def main():
    george = ref_loader.load_reference()
    if george is None:
        raise SystemExit("reference not available (need the reference sources and oracle/_ref built: make -C oracle)")
    from george_amd import program
    out = {}
    for name, kr in zoo.kernel_zoo(george.kernels):
        out[name + "/flat"] = np.frombuffer(bytes(program.flatten(kr)), dtype=np.uint8)
        out[name + "/ndim_size"] = np.array([kr.ndim, kr.full_size], dtype=np.int64)
    rng = np.random.RandomState(5)                      # the draws of test_against_live_reference_when_available
    for name, kr in zoo.kernel_zoo(george.kernels)[::7]:
        t1 = rng.randn(11, kr.ndim)
        out[name + "/live_t1"] = t1
        out[name + "/live_value"] = kr.get_value(t1)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ref_objects.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
