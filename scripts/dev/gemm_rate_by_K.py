"""Rate of the trailing-update GEMM (gemm_f64_mfma_dma_sp<lower>) alone on the chip as a function of K, through gh_dev_gemm:
the SYRK shape (C M x M, lower tiles) at M = 32768 and 57344 and the lower-trapezoid shape (C M x 2048 and M x 8192 columns)
for K = 1024 ... 16384.  Launches timed by HIP events, one process, shapes alternated; best and median per shape, and the
fit  rate(K) = R / (1 + K0 / K)  per shape.  python scripts/dev/gemm_rate_by_K.py [reps] > profiles/two_level/gemm_rate_by_K.md"""
import ctypes as C
import os
import sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from george_amd import _native as N  # noqa: E402
import torch  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KS = (1024, 2048, 4096, 8192, 16384)
SHAPES = [(32768, 32768), (57344, 57344), (57344, 2048), (57344, 8192)]      # (M, columns of C); lower tiles only
dp = C.POINTER(C.c_double)
dev = torch.device("cuda", 0)
mmax = max(m for m, _ in SHAPES)
c = torch.zeros(mmax * mmax, dtype=torch.float64, device=dev)
a = torch.randn(mmax, max(KS), dtype=torch.float64, device=dev)
a *= 1e-3


def tiles(m, n):
    tm, tn = m // 128, n // 128
    return tn * (tn + 1) // 2 + (tm - tn) * tn


def launch(m, n, k):
    # C (m x n, pitch m) -= A[:m, :k] A[:n, :k]^T: the operands are column slices with the pitch of A, as in the factorisation
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    N.check(N.lib.gh_dev_gemm(C.cast(c.data_ptr(), dp), m, C.cast(a.data_ptr(), dp), a.stride(0), C.cast(a.data_ptr(), dp), a.stride(0),
                              m, n, k, -1.0, 1.0, 4, None))
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


ms = {}
for rep in range(REPS + 1):
    for (m, n) in SHAPES:
        for k in KS:
            t = launch(m, n, k)
            if rep:
                ms.setdefault((m, n, k), []).append(t)
print("# `gemm_f64_mfma_dma_sp<lower>` alone on the chip by K (`scripts/dev/gemm_rate_by_K.py`, %d launches per cell, shapes alternated)\n" % REPS)
print("| C (lower tiles) | K | ms best | ms median | TFLOP/s best | TFLOP/s median | best against K = 2048 | spread (max - min) / min |")
print("|---|---|---|---|---|---|---|---|")
for (m, n) in SHAPES:
    rate = {}
    for k in KS:
        v = np.array(ms[(m, n, k)])
        fl = tiles(m, n) * 2.0 * 128 * 128 * k
        rate[k] = fl / v.min() * 1e-9
    for k in KS:
        v = np.array(ms[(m, n, k)])
        fl = tiles(m, n) * 2.0 * 128 * 128 * k
        print("| %d x %d | %d | %.3f | %.3f | %.2f | %.2f | %+.2f %% | %.2f %% |" % (
            m, n, k, v.min(), np.median(v), rate[k], fl / np.median(v) * 1e-9, (rate[k] / rate[2048] - 1) * 100,
            (v.max() - v.min()) / v.min() * 100))
    # 1 / rate = 1 / R + (K0 / R) / K: a straight line in 1 / K
    x = np.array([1.0 / k for k in KS]); y = np.array([1.0 / rate[k] for k in KS])
    s, i = np.polyfit(x, y, 1)
    print("| %d x %d | fit | | | R = %.2f | K0 = %.1f | | |" % (m, n, 1.0 / i, s / i))
sys.stdout.flush()
