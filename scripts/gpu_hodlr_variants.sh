#!/bin/bash
# build variants of the HODLR units that read compile-time knobs (UNITS, default: the ACA kernels and compute()) ON THE BOX and time C4
# with each: VARIANTS="name:flags;name:flags".  Every other object comes from build/ (make -C george_amd/csrc first).
cd /root/repo; mkdir -p gpurun_out/hodlr; export TMPDIR=/tmp
O=gpurun_out/hodlr
cp george_amd/csrc/libgeorge_amd.so /tmp/lib_default.so
IFS=';' read -ra VS <<< "$VARIANTS"
for v in "${VS[@]}"; do
  name="${v%%:*}"; flags="${v#*:}"
  ( cd george_amd/csrc && objs="" && \
    for u in ${UNITS:-gh_hodlr_aca gh_hodlr}; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result $flags -c $u.hip -o /tmp/${u}_$name.o 2>/dev/null || exit 1; objs="$objs /tmp/${u}_$name.o"; done && \
    for o in build/gh_*.o; do case "$o" in *-hip-*) continue;; esac; u=$(basename $o .o); [ -e /tmp/${u}_$name.o ] || objs="$objs $o"; done && \
    hipcc --offload-arch=gfx950 -shared -fPIC $objs -ldl -lpthread -o libgeorge_amd.so )
  echo "== variant $name ($flags)"
  timeout -s KILL 200 python scripts/dev/hodlr_wave_ab.py 262144 2>&1 | grep "^| 262144"
done
cp /tmp/lib_default.so george_amd/csrc/libgeorge_amd.so
