#!/bin/bash
# A/B of a compile-time variant of the HODLR units on one box: VARIANT="-DGH_ACA_BATCH_ONES=0" bash scripts/gpu_hodlr_variant_ab.sh
# UNITS: the units that read the flag (default gh_hodlr_aca: GH_ACA_BATCH_ONES and the ACA_* knobs; GH_ACA_TIMES needs "gh_hodlr_aca gh_hodlr").
# Every other object comes from build/ (make -C george_amd/csrc first).
cd /root/repo; export TMPDIR=/tmp
cp george_amd/csrc/libgeorge_amd.so /tmp/lib_default.so
( cd george_amd/csrc && objs="" && \
  for u in ${UNITS:-gh_hodlr_aca}; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $VARIANT -c $u.hip -o /tmp/${u}_var.o 2>/dev/null || exit 1; objs="$objs /tmp/${u}_var.o"; done && \
  for o in build/gh_*.o; do case "$o" in *-hip-*) continue;; esac; u=$(basename $o .o); [ -e /tmp/${u}_var.o ] || objs="$objs $o"; done && \
  hipcc --offload-arch=gfx950 -shared -fPIC $objs -ldl -lpthread -o /tmp/lib_variant.so )
cat > /tmp/t.py <<'PY'
import sys, time; sys.path.insert(0, "/root/repo")
import numpy as np, bench, torch
for n in [int(a) for a in sys.argv[2:]]:
    job = bench.HodlrJob(n, 0)
    for i in range(4): job.step()
    ts = []
    for i in range(15):
        torch.cuda.synchronize(); t0 = time.perf_counter(); ll = job.step(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    print("%s N = %7d: %.3f / %.3f / %.3f ms  ll %.15g" % (sys.argv[1], n, min(ts), float(np.median(ts)), max(ts), ll), flush=True)
    del job
PY
for rnd in 1 2 3; do
  cp /tmp/lib_default.so george_amd/csrc/libgeorge_amd.so; python /tmp/t.py default ${SIZES:-262144} 2>&1 | grep "N ="
  cp /tmp/lib_variant.so george_amd/csrc/libgeorge_amd.so; python /tmp/t.py variant ${SIZES:-262144} 2>&1 | grep "N ="
done
cp /tmp/lib_default.so george_amd/csrc/libgeorge_amd.so
