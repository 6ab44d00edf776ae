"""From a rocprofv3 --kernel-trace database of bench.py steps: per step (delimited by the kernel-matrix build), the far trailing
updates (gemm_f64_mfma_dma_sp<lower>, >= 36 workgroups) of the hardware queue that carries most of them -- the main stream's:
launches, busy ms, span from the first start to the last end, idle ms inside that span.
python scripts/dev/main_stream_idle.py <results.db>"""
import sqlite3
import sys

con = sqlite3.connect(sys.argv[1])
cur = con.cursor()
cols = [r[1] for r in cur.execute("pragma table_info(rocpd_kernel_dispatch)")]
qcol = "queue_id" if "queue_id" in cols else ("stream_id" if "stream_id" in cols else None)
rows = list(cur.execute(
    "select d.start, d.end, d.grid_size_x / d.workgroup_size_x, s.kernel_name%s "
    "from rocpd_kernel_dispatch d join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start" % (", d." + qcol if qcol else ", 0")))
builds = [r[0] for r in rows if "kmat_interior" in r[3]]
far = [r for r in rows if "dma_spILb1EE" in r[3] and r[2] >= 36]
byq = {}
for r in far:
    byq[r[4]] = byq.get(r[4], 0) + (r[1] - r[0])
main_q = max(byq, key=byq.get)
print("queue column: %s; lower-sp time by queue (ms): %s; main = %s\n" % (qcol, {k: round(v / 1e6, 1) for k, v in byq.items()}, main_q))
print("| step | launches on the main queue | busy ms | span ms | idle ms inside the span | largest gap ms |\n|---|---|---|---|---|---|")
for i, b in enumerate(builds):
    e = builds[i + 1] if i + 1 < len(builds) else float("inf")
    v = [r for r in far if r[4] == main_q and b <= r[0] < e]
    if not v:
        continue
    busy = sum(r[1] - r[0] for r in v) / 1e6
    span = (max(r[1] for r in v) - v[0][0]) / 1e6
    gaps = [(v[q + 1][0] - v[q][1]) / 1e6 for q in range(len(v) - 1)]
    print("| %d | %d | %.2f | %.2f | %.2f | %.2f |" % (i, len(v), busy, span, span - busy, max(gaps) if gaps else 0.0))
