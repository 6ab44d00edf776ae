#!/bin/bash
cd /root/repo; export TMPDIR=/tmp
cp george_amd/csrc/libgeorge_amd.so /tmp/lib_default.so
# GH_ACA_TIMES is read by the ACA kernels (gh_hodlr_aca.hip) and by compute() (gh_hodlr.hip); every other object comes from build/
( cd george_amd/csrc && objs="" && \
  for u in gh_hodlr_aca gh_hodlr; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -DGH_ACA_TIMES -c $u.hip -o /tmp/${u}_times.o 2>/dev/null || exit 1; objs="$objs /tmp/${u}_times.o"; done && \
  for o in build/gh_*.o; do case "$o" in *-hip-*) continue;; esac; u=$(basename $o .o); [ -e /tmp/${u}_times.o ] || objs="$objs $o"; done && \
  hipcc --offload-arch=gfx950 -shared -fPIC $objs -ldl -lpthread -o libgeorge_amd.so )
python - <<'PY' 2>&1 | grep "aca\|ms"
import sys; sys.path.insert(0, "/root/repo")
import bench
job = bench.HodlrJob(262144, 0)
el, ll = bench.run_timed(job, 6, 0, lambda: None)
print('ms', el / 6 * 1e3, ll)
PY
cp /tmp/lib_default.so george_amd/csrc/libgeorge_amd.so
