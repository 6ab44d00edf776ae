// gh_hodlr_aca.hip -- the ACA of the HODLR solver's off-diagonal blocks (gh_hodlr_impl.h has the map of the units): the kernel
// that gives a node a workgroup or a cluster of them, the one that gives it a wavefront, and the launcher of each.
#include <math.h>
#include "gh_hodlr_impl.h"
#include "gh_device_util.h"
#include "gh_spin.h"

// =========================================================================== ACA
// hodlr.h:136-221 for every internal node of one level.  Tcm is column-major scratch
// (Tcm[k*N + i]): for a node, entries at its first-half rows hold V(:,k) (the block's columns),
// at its second-half rows U(:,k).
#ifndef ACA_WAVES_PER_EU
#define ACA_WAVES_PER_EU 4     // one-workgroup nodes: <= 128 registers per lane -- two of these workgroups, or one and 256 registers of other kernels, per SIMD
#endif
#ifndef ACA_WAVES_PER_EU_CL
#define ACA_WAVES_PER_EU_CL 2  // the cooperative launch: the critical chain of phase 1 keeps the registers it wants (no spills)
#endif
#define ACA_NC 64              // candidate rows tested per search pass once the search has started failing
#define ACA_LIDX 4096          // row permutations of one-workgroup nodes live in LDS up to this many rows
#ifndef ACA_CAPD
#define ACA_CAPD 2048          // doubles of U and of V a one-workgroup node mirrors in LDS (its first CAPD / n rows of each factor)
#endif
#define ACA_XC 512             // ... and its coordinates when ndim == 1 (rows, then columns)
#define ACA_DYN_BYTES (ACA_CAPD > 0 ? (2 * ACA_CAPD + 2 * ACA_XC) * 8 : 0)
// One node is worked on by a CLUSTER of G workgroups (blockIdx.x = node * G + g): the top levels
// have 1, 2, 4, ... nodes with blocks of N/2, N/4, ... rows, and one workgroup per node left the
// single workgroup of level 0 with 70 % of the whole HODLR compute() at N = 262144.  Workgroup g
// owns the columns and rows  t = g * 512 + tid (+ G * 512 ...)  of the block; the cluster meets
// at three barriers per ACA step (row chosen / pivot search / norms), each a monotonic counter in
// HBM, and exchanges its partial results (arg-max candidates, partial sums) through `part`.
// Every workgroup reduces the SAME partials in the SAME order, so all of them take identical
// decisions without a broadcast.  Data written by another workgroup of the cluster is read with
// agent-scope atomic loads (a plain load may hit a stale line of this CU's L1).  G = 1 is the
// old one-workgroup-per-node kernel (no counters touched).  The launch keeps nodes * G <= 256 so
// that the whole grid is resident (a spinning cluster member never waits for an unscheduled one);
// a spin that outlasts ~2 s raises `*fail` and bails out instead of hanging the GPU.
struct AcaShared {
  double shd[8];
  int shi[8];
  double coef[ACA_MAXR];
  int s_i;
  // batched candidate search (one-workgroup nodes)
  int cand_k[ACA_NC], cand_i[ACA_NC], cand_tail[ACA_NC], cand_bestn[ACA_NC];
  double cand_best[ACA_NC];
  unsigned long long cand_st[ACA_NC];
  unsigned short lidx[ACA_LIDX];
  double pivv;
};
// stores of values that another workgroup of the cluster will read: agent-scope atomics (write-through,
// visible to the other XCDs' atomic loads once s_waitcnt has seen them complete) -- no release fence
__device__ __forceinline__ void aca_st(double* p, double v, bool shared_w) {
  if (shared_w) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else *p = v;
}
__device__ __forceinline__ double aca_ld(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int aca_ldi(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// cluster barrier number `epoch` (0, 1, 2, ...) on counter `bar`; returns false on time-out
__device__ __forceinline__ bool aca_barrier(unsigned* bar, int G, unsigned& epoch, int* fail, int fence) {
  if (G == 1) { __syncthreads(); return true; }
  __shared__ int ok;
  // Release side without a fence: everything this workgroup wrote for the others went out as
  // agent-scope atomic stores (aca_st), and s_waitcnt makes every lane's stores complete before the
  // arrival is counted.  __threadfence() here writes this XCD's L2 back at every barrier -- three
  // per ACA step, 128 workgroups: 60 us per barrier, 2.8 of the 7 ms of ACA time at N = 262144.
  // (The `fence` argument restores it; its environment switch went in round 4.)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fence) __threadfence();
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = (unsigned)G * (epoch + 1u);
    GhSpin spin(fail);                                      // (gh_spin.h: the 2-s give-up and the abort word)
    int good = 1;
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (!spin.keep_waiting(0u)) { good = 0; break; }
    }
    if (!good) atomicExch(fail, 1);
    // (no acquire fence: everything another cluster member wrote is read with agent-scope atomic
    //  loads, which go past this XCD's caches; a fence here would invalidate the L2 at every barrier)
    ok = good;
  }
  __syncthreads();
  ++epoch;
  return ok != 0;
}
// CL: the CLUSTER instantiation (G > 1: the cooperative launch of the top levels) without the one-workgroup-only machinery --
// batched candidate search, LDS mirrors, LDS row permutation; !CL: one workgroup per node (G == 1) without the cluster protocol.
// One kernel for both needed 225 registers per lane: the cooperative launch -- one 512-thread workgroup on every CU for 1.4 ms,
// two wavefronts per SIMD -- then held 464 of each SIMD's 512 registers, and nothing else of phase 1 (one-workgroup nodes 225,
// leaf Cholesky 256, leaf build 127) could share a SIMD with it (profiles/r06/hodlr_phase1_registers.md).
template <bool FAST, bool CL>
__global__ __launch_bounds__(ACA_THREADS, CL ? ACA_WAVES_PER_EU_CL : ACA_WAVES_PER_EU) void hodlr_aca_kernel(
    const GhNode* __restrict__ prog, int n_prog, GhFast fast, int nd, const double* x, const LvlNode* nodes, double* Tcm, long N,
    int rcap, int* idx, int* ranks, double tol, unsigned long long seed, int level,
    int G_, unsigned* bars, double* part, int pstride, int* sel, int* fail, int multi, int fence, int* trunc,
    const AcaSeg* segs, int nseg, int capd_) {
  int G = CL ? G_ : 1;
  const int capd = CL ? 0 : capd_;
#ifdef ACA_CL_SETPRIO
  if (CL) __builtin_amdgcn_s_setprio(ACA_CL_SETPRIO);       // the critical chain of phase 1 first at every SIMD's arbiter
#endif
  __shared__ AcaShared sh;
  extern __shared__ double aca_dyn[];                  // capd > 0: U mirror | V mirror | coordinates (ACA_DYN_BYTES)
  int bid = blockIdx.x;
  int* dur = nullptr;
  const int* order = nullptr;
  if (segs) {
    int q = 0;
    while (q + 1 < nseg && bid >= segs[q].wg0 + segs[q].nwg) ++q;
    const AcaSeg sg = segs[q];
    nodes = sg.nodes; Tcm = sg.Tcm; idx = sg.idx; ranks = sg.ranks; bars = sg.bars; part = sg.part; sel = sg.sel;
    fail = sg.fail; trunc = sg.trunc; level = sg.level; G = CL ? sg.G : 1;
    bid -= sg.wg0;
    if (!CL) { dur = sg.dur; order = sg.order; }
  }
  const long long t_begin = dur ? wall_clock64() : 0;
  const int node = order ? order[bid] : bid / G, g = order ? 0 : bid % G;
  const LvlNode nodev = nodes[node];
  const int col0 = nodev.start, n_cols = nodev.half;
  const int row0 = nodev.start + nodev.half, n_rows = nodev.size - nodev.half;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int t0 = g * nt + tid, ts = G * nt;            // this thread's first column/row and its stride
  const bool sw = G > 1;                               // values other workgroups read go out as atomics
  unsigned* bar = bars + node;
  double* mypart = part + ((long)node * G + g) * pstride;
  const double* allpart = part + (long)node * G * pstride;
  unsigned epoch = 0;
  const int full_rank = n_rows < n_cols ? n_rows : n_cols;
  int max_rank = full_rank;
  if (max_rank > rcap) max_rank = rcap;
  // one-workgroup nodes keep the row permutation in LDS (the candidate draws are a serial chain of
  // dependent reads and writes: ~1 us each through HBM, 64 of them per search pass)
  const bool lperm = !CL && (G == 1) && n_rows <= ACA_LIDX;
  // Small one-workgroup nodes (levels 8-10 of C4: 1792 of its 2047 blocks) are a chain of ~10 dependent global round trips
  // per ACA step -- 13 us per step for 128-entry vectors.  They mirror the first `kcap` rows of U and V (and, in 1-D, their
  // coordinates) in LDS: every read of a factor entry below comes from the mirror when its row is there, every write goes to
  // both.  Same values, same order of operations: the factors and ranks do not change by a bit.
  const int kcap = (lperm && capd > 0 && n_rows <= capd && n_cols <= capd) ? min(capd / n_rows, capd / n_cols) : 0;
  double* const uc = aca_dyn;
  double* const vc = aca_dyn + capd;
  double* const xs = aca_dyn + 2 * capd;
  const bool xlds = kcap > 0 && nd == 1 && n_rows <= ACA_XC && n_cols <= ACA_XC;
  if (xlds) {
    for (int t = tid; t < n_rows; t += nt) xs[t] = x[row0 + t];
    for (int t = tid; t < n_cols; t += nt) xs[ACA_XC + t] = x[col0 + t];
  }
  auto xrow = [&](int m) -> const double* { return xlds ? (const double*)(xs + m) : x + (long)(row0 + m) * nd; };
  auto xcol = [&](int n) -> const double* { return xlds ? (const double*)(xs + ACA_XC + n) : x + (long)(col0 + n) * nd; };
  if (lperm) { for (int t = tid; t < n_rows; t += nt) sh.lidx[t] = (unsigned short)t; }
  else if (g == 0) { for (int t = tid; t < n_rows; t += nt) idx[row0 + t] = t; }
  int remaining = n_rows, rank = 0;
  int batch = 8;                                       // candidates per search pass: 8, then ACA_NC once a pass has failed
  double norm = 0.0;
  const double tol2 = tol * tol;
  bool converged = false;
  // (nodev.pad: index of the launch's first node in its tree level -- non-zero only for the sub-trees of a split tree)
  unsigned long long st = seed ^ ((unsigned long long)(level + 1) << 40) ^ ((unsigned long long)(node + nodev.pad) * 0x9E3779B97F4A7C15ull);
  __syncthreads();
#ifdef GH_ACA_TIMES
  const long long dbg_t0 = wall_clock64();
  int dbg_passes = 0;
#endif
  bool have_sel = false;                               // clusters: the next candidate row has been drawn and published already
  auto draw_row = [&]() {                              // (workgroup 0, thread 0 of the cluster) hodlr.h:159-176: a random unused row
    st += 0x9E3779B97F4A7C15ull;
    unsigned long long z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const int k = (int)(z % (unsigned long long)remaining);
    int pick;
    if (lperm) { pick = sh.lidx[k]; sh.lidx[k] = sh.lidx[remaining - 1]; }
    else { pick = idx[row0 + k]; idx[row0 + k] = idx[row0 + remaining - 1]; }
    if (sw) __hip_atomic_store(sel + node, pick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else sel[node] = pick;
  };
  while (rank < max_rank) {
    // ---- choose a random unused row with a non-negligible residual (hodlr.h:159-191)
    bool got = false;
    int j = -1;
    double pivot = 0.0;
    // One-workgroup nodes test a BATCH of candidate rows per pass, wavefront w the candidates
    // w, w + 8, ...  Towards the end of a node's ACA every remaining row is below the 1e-14
    // threshold and the search walks through all of them before giving up (hodlr.h:159-191 does
    // too): one row per pass made levels 8 and 9 of C4 cost 2.6 ms for rank-3 blocks, eight per pass
    // 0.75 + 0.6 ms; after the first pass without a hit the batch grows to 64.  Same result as the
    // one-by-one search: the candidates are drawn in the same order, the first that passes wins,
    // and the draws after it are undone (row permutation and generator state restored).
    while (!CL && (multi & 1) && lperm && remaining > 0 && rank <= 32) {
      int NC = remaining < batch ? remaining : batch;
      if (rank + NC > rcap) NC = rcap - rank;
      if (NC < 1) break;
#ifdef GH_ACA_TIMES
      ++dbg_passes;
#endif
      if (tid == 0) {
        for (int c = 0; c < NC; ++c) {
          st += 0x9E3779B97F4A7C15ull;
          unsigned long long z = st;
          z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
          z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
          z ^= z >> 31;
          const int k = (int)(z % (unsigned long long)(remaining - c));
          sh.cand_k[c] = k;
          sh.cand_i[c] = sh.lidx[k];
          sh.cand_tail[c] = sh.lidx[remaining - c - 1];
          sh.lidx[k] = (unsigned short)sh.cand_tail[c];
          sh.cand_st[c] = st;
        }
      }
      __syncthreads();
      const int lane = tid & 63, wave = tid >> 6;
      for (int c = wave; c < NC; c += (nt >> 6)) {
        const int i = sh.cand_i[c];
        double* cw = sh.coef + wave * 32;
        __builtin_amdgcn_wave_barrier();              // (the previous candidate's reads of cw are done)
        for (int k = lane; k < rank; k += 64) cw[k] = k < kcap ? uc[k * n_rows + i] : Tcm[(long)k * N + row0 + i];
        __builtin_amdgcn_s_waitcnt(0);                // (own wavefront's LDS writes, read back below)
        __builtin_amdgcn_wave_barrier();
        double best = -1.0;
        int bestn = -1;
        const double* xi = xrow(i);
        const int kv = rank < kcap ? rank : kcap;
        // (only the candidate's largest entry is kept: storing 8-64 residual rows per pass to keep one was most of this
        //  kernel's write traffic; the chosen row is formed again below, by the whole workgroup)
        for (int n = lane; n < n_cols; n += 64) {
          double v = FAST ? gh_fast_value(fast, xi, xcol(n)) : gh_eval_value(prog, n_prog, xi, xcol(n));
          for (int k = 0; k < kv; ++k) v -= cw[k] * vc[k * n_cols + n];
          for (int k = kv; k < rank; ++k) v -= cw[k] * Tcm[(long)k * N + col0 + n];
          const double a = fabs(v);
          if (a > best) { best = a; bestn = n; }
        }
        for (int off = 32; off > 0; off >>= 1) {          // largest value, smallest column on ties
          const double ov = __shfl_down(best, off, 64);
          const int oi = __shfl_down(bestn, off, 64);
          if (ov > best || (ov == best && oi >= 0 && (bestn < 0 || oi < bestn))) { best = ov; bestn = oi; }
        }
        if (lane == 0) { sh.cand_best[c] = best; sh.cand_bestn[c] = bestn; }
      }
      __syncthreads();
      int chosen = -1;
      for (int c = 0; c < NC; ++c)
        if (sh.cand_best[c] >= 1e-14) { chosen = c; break; }                           // hodlr.h:191
      if (chosen < 0) {
        remaining -= NC;
        // (round 6) The first pass without a hit: before walking the rest of the rows 64 at a time, SCREEN them all -- thread t the
        // rows lidx[t], lidx[t + 512], ..., a whole row each (no cross-lane reduction, V entries and column points as LDS
        // broadcasts), leaving as soon as anybody has found an entry >= 1e-14.  If nobody has, every remaining row would fail
        // its test: the search ends as it would after the walk (rows exhausted, same rank, same factors).  The walk of the one
        // such node of C4's level 8 took 806 us -- twelve passes -- and was the tail of phase 1; its screen is ~50 us.
        if (batch != ACA_NC && remaining > 0 && rank <= 8 && (long)n_rows * n_cols <= 512L * 512L) {    // (a thread walks whole rows: 512 entries here; 0.7 ms for a 2048 x 2048 block)
          if (tid == 0) sh.s_i = 0;
          __syncthreads();
          const int kv = rank < kcap ? rank : kcap;
          for (int q = tid; q < remaining && !*(volatile int*)&sh.s_i; q += nt) {
            const int i = sh.lidx[q];
            double cu[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) cu[k] = k < rank ? (k < kcap ? uc[k * n_rows + i] : Tcm[(long)k * N + row0 + i]) : 0.0;
            const double* xi = xrow(i);
            bool hit = false;
            for (int n = 0; n < n_cols && !hit; ++n) {
              double v = FAST ? gh_fast_value(fast, xi, xcol(n)) : gh_eval_value(prog, n_prog, xi, xcol(n));
#pragma unroll
              for (int k = 0; k < 8; ++k) if (k < rank) v -= cu[k] * (k < kv ? vc[k * n_cols + n] : Tcm[(long)k * N + col0 + n]);
              hit = fabs(v) >= 1e-14;
              if ((n & 31) == 31 && *(volatile int*)&sh.s_i) break;
            }
            if (hit) *(volatile int*)&sh.s_i = 1;
          }
          __syncthreads();
          if (!*(volatile int*)&sh.s_i) remaining = 0;
          __syncthreads();
        }
        batch = ACA_NC;
        __syncthreads();
        continue;
      }
      if (tid == 0) {                                 // undo the draws after the chosen one, last first
        for (int c = NC - 1; c > chosen; --c) {
          sh.lidx[sh.cand_k[c]] = (unsigned short)sh.cand_i[c];
          sh.lidx[remaining - c - 1] = (unsigned short)sh.cand_tail[c];
        }
      }
      st = sh.cand_st[chosen];                        // (every thread keeps the generator state in step)
      remaining -= chosen + 1;
      j = sh.cand_bestn[chosen];
      {
        // the chosen candidate's residual row into row `rank` of the scratch: same expression and order of k as in the
        // search, so the same bits
        const int i = sh.cand_i[chosen];
        for (int k = tid; k < rank; k += nt) sh.coef[k] = k < kcap ? uc[k * n_rows + i] : Tcm[(long)k * N + row0 + i];
        __syncthreads();
        const double* xi = xrow(i);
        const int kv = rank < kcap ? rank : kcap;
        for (int n = tid; n < n_cols; n += nt) {
          double v = FAST ? gh_fast_value(fast, xi, xcol(n)) : gh_eval_value(prog, n_prog, xi, xcol(n));
          for (int k = 0; k < kv; ++k) v -= sh.coef[k] * vc[k * n_cols + n];
          for (int k = kv; k < rank; ++k) v -= sh.coef[k] * Tcm[(long)k * N + col0 + n];
          Tcm[(long)rank * N + col0 + n] = v;
          if (rank < kcap) vc[rank * n_cols + n] = v;
        }
      }
      __syncthreads();
      pivot = rank < kcap ? vc[rank * n_cols + j] : Tcm[(long)rank * N + col0 + j];
      got = true;
      break;
    }
    while (!got && (have_sel || remaining > 0)) {
      if (!have_sel) {
        if (g == 0 && tid == 0) draw_row();
        --remaining;
        if (!aca_barrier(bar, G, epoch, fail, fence)) return;                         // B1: row chosen
      }
      have_sel = false;
      const int i = (G == 1) ? sel[node] : aca_ldi(sel + node);
      for (int k = tid; k < rank; k += nt) sh.coef[k] = aca_ld(Tcm + (long)k * N + row0 + i);   // U(i, 0:rank)
      __syncthreads();
      double best = -1.0, bestv = 0.0;
      int bestn = -1;
      const double* xi = x + (long)(row0 + i) * nd;
      for (int n = t0; n < n_cols; n += ts) {
        double v = FAST ? gh_fast_value(fast, xi, x + (long)(col0 + n) * nd)
                        : gh_eval_value(prog, n_prog, xi, x + (long)(col0 + n) * nd);
        for (int k = 0; k < rank; ++k) v -= sh.coef[k] * Tcm[(long)k * N + col0 + n];
        Tcm[(long)rank * N + col0 + n] = v;           // (rewritten after the pivot is known: owner-only so far)
        if (rank < kcap) vc[rank * n_cols + n] = v;
        const double a = fabs(v);
        if (a > best) { best = a; bestn = n; }
      }
      hw_block_argmax(best, bestn, sh.shd, sh.shi);
      if (G > 1) {
        if (tid == 0) {
          aca_st(mypart + 0, best, true);
          aca_st(mypart + 1, (double)bestn, true);
          aca_st(mypart + 2, bestn >= 0 ? Tcm[(long)rank * N + col0 + bestn] : 0.0, true);   // (this workgroup wrote it)
        }
        if (!aca_barrier(bar, G, epoch, fail, fence)) return;                         // B2: pivot search
        // every workgroup reduces the same G candidates with the same tree (thread q takes member q's):
        // largest value, smallest column on ties.  (A serial loop of 3 G device-scope loads in EVERY
        // thread was most of the 185 us an ACA step of the root node took.)
        double cv = -1.0, cvv = 0.0;
        int cn = -1;
        if (tid < G) {
          cv = aca_ld(allpart + (long)tid * pstride);
          cn = (int)aca_ld(allpart + (long)tid * pstride + 1);
          cvv = aca_ld(allpart + (long)tid * pstride + 2);
          if (cn < 0) cv = -1.0;
        }
        best = cv; bestn = cn;
        hw_block_argmax(best, bestn, sh.shd, sh.shi);
        if (tid < G && cn >= 0 && cn == bestn) sh.pivv = cvv;      // (columns are owned by one workgroup: a unique writer)
        __syncthreads();
        bestv = bestn >= 0 ? sh.pivv : 0.0;
      } else {
        bestv = bestn >= 0 ? Tcm[(long)rank * N + col0 + bestn] : 0.0;
      }
      if (best >= 1e-14) { got = true; j = bestn; pivot = bestv; break; }              // hodlr.h:191
    }
    // rows exhausted: every residual row tested below 1e-14 in absolute value -- keep the factors we
    // have (the reference returns the exact block as a rank-min(rows, cols) "trivial factorisation",
    // hodlr.h:160-176; the two represent the same block to 1e-14 per entry)
    if (!got) { converged = true; break; }
    // ---- normalise the row by its pivot, build the column (hodlr.h:194-199)
    __syncthreads();
    double vn2 = 0.0;
    for (int n = t0; n < n_cols; n += ts) {
      const double v = (rank < kcap ? vc[rank * n_cols + n] : Tcm[(long)rank * N + col0 + n]) / pivot;
      aca_st(Tcm + (long)rank * N + col0 + n, v, sw);
      if (rank < kcap) vc[rank * n_cols + n] = v;
      vn2 += v * v;
    }
    for (int k = tid; k < rank; k += nt) sh.coef[k] = k < kcap ? vc[k * n_cols + j] : aca_ld(Tcm + (long)k * N + col0 + j);    // V(j, 0:rank)
    __syncthreads();
    double un2 = 0.0;
    const double* xj = xcol(j);
    const int kvu = rank < kcap ? rank : kcap;
    for (int m = t0; m < n_rows; m += ts) {
      double u = FAST ? gh_fast_value(fast, xrow(m), xj) : gh_eval_value(prog, n_prog, xrow(m), xj);
      for (int k = 0; k < kvu; ++k) u -= sh.coef[k] * uc[k * n_rows + m];
      for (int k = kvu; k < rank; ++k) u -= sh.coef[k] * Tcm[(long)k * N + row0 + m];
      aca_st(Tcm + (long)rank * N + row0 + m, u, sw);
      if (rank < kcap) uc[rank * n_rows + m] = u;
      un2 += u * u;
    }
    ++rank;
    if (rank >= full_rank) { converged = true; break; }                                // hodlr.h:203
    if (rank >= max_rank) break;                                                       // rank cap: NOT converged
    // cross terms |u_new . u_k|, |v_new . v_k|, k < rank-1, of the norm estimate (hodlr.h:210-214):
    // this workgroup's share of each dot product, four at a time
    const double* ul = Tcm + (long)(rank - 1) * N + row0;
    const double* vl = Tcm + (long)(rank - 1) * N + col0;
    double maxu = 0.0, maxv = 0.0;
    // (round 6) ONE workgroup barrier for all the block sums of a step instead of two per sum: the
    // wavefronts' partial sums of the two squared norms and of the 2 (rank - 1) cross terms go to LDS (sh.coef is free between the
    // column build and the next step), thread k then adds the eight wavefront sums of term k in hw_block_sum's order -- the same
    // bits -- and publishes it.  The root of C4 (rank ~20) went through ~460 block sums, two barriers each.
#ifndef GH_ACA_BATCH_ONES
#define GH_ACA_BATCH_ONES 1
#endif
    const bool batched = (CL || GH_ACA_BATCH_ONES) && rank <= 120;
    if (batched) {
      const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
      double* const ws = sh.coef;                      // [(term * 2 + side) * 8 + wavefront]; term rank - 1 = the squared norms
      __syncthreads();                                 // (every thread is done with the column build's coefficients)
      {
        const double a = hw_wave_sum(un2), b = hw_wave_sum(vn2);
        if (lane == 0) { ws[((rank - 1) * 2) * 8 + wave] = a; ws[((rank - 1) * 2 + 1) * 8 + wave] = b; }
      }
      for (int k0 = 0; k0 < rank - 1; k0 += 4) {
        double du[4] = {0, 0, 0, 0}, dv[4] = {0, 0, 0, 0};
        for (int m = t0; m < n_rows; m += ts) {
          const double u = rank - 1 < kcap ? uc[(rank - 1) * n_rows + m] : ul[m];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (k0 + q < rank - 1) du[q] += (k0 + q < kcap ? uc[(k0 + q) * n_rows + m] : Tcm[(long)(k0 + q) * N + row0 + m]) * u;
        }
        for (int n = t0; n < n_cols; n += ts) {
          const double v = rank - 1 < kcap ? vc[(rank - 1) * n_cols + n] : vl[n];
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (k0 + q < rank - 1) dv[q] += (k0 + q < kcap ? vc[(k0 + q) * n_cols + n] : Tcm[(long)(k0 + q) * N + col0 + n]) * v;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double a = hw_wave_sum(du[q]), b = hw_wave_sum(dv[q]);
          if (lane == 0 && k0 + q < rank - 1) { ws[((k0 + q) * 2) * 8 + wave] = a; ws[((k0 + q) * 2 + 1) * 8 + wave] = b; }
        }
      }
      __syncthreads();
      double ta = 0.0, tb = 0.0;
      if (tid < rank)
        for (int w = 0; w < nw; ++w) { ta += ws[(tid * 2) * 8 + w]; tb += ws[(tid * 2 + 1) * 8 + w]; }
      if (G > 1) {
        if (tid < rank - 1) { aca_st(mypart + 6 + 2 * tid, ta, true); aca_st(mypart + 7 + 2 * tid, tb, true); }
        if (tid == rank - 1) { sh.shd[0] = ta; sh.shd[1] = tb; }      // (published behind the next row's draw, below)
        __syncthreads();
        un2 = sh.shd[0]; vn2 = sh.shd[1];
      } else {
        __syncthreads();                               // (all partial sums read)
        if (tid < rank) { ws[tid] = tid < rank - 1 ? fabs(ta) : ta; ws[1024 + tid] = tid < rank - 1 ? fabs(tb) : tb; }
        __syncthreads();
        for (int k = 0; k < rank - 1; ++k) {
          if (ws[k] > maxu) maxu = ws[k];
          if (ws[1024 + k] > maxv) maxv = ws[1024 + k];
        }
        un2 = ws[rank - 1]; vn2 = ws[1024 + rank - 1];
        __syncthreads();                               // (coef is written again at the next step)
      }
    } else {
    un2 = hw_block_sum(un2, sh.shd);
    vn2 = hw_block_sum(vn2, sh.shd);
    for (int k0 = 0; k0 < rank - 1; k0 += 4) {
      double du[4] = {0, 0, 0, 0}, dv[4] = {0, 0, 0, 0};
      for (int m = t0; m < n_rows; m += ts) {
        const double u = rank - 1 < kcap ? uc[(rank - 1) * n_rows + m] : ul[m];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k0 + q < rank - 1) du[q] += (k0 + q < kcap ? uc[(k0 + q) * n_rows + m] : Tcm[(long)(k0 + q) * N + row0 + m]) * u;
      }
      for (int n = t0; n < n_cols; n += ts) {
        const double v = rank - 1 < kcap ? vc[(rank - 1) * n_cols + n] : vl[n];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k0 + q < rank - 1) dv[q] += (k0 + q < kcap ? vc[(k0 + q) * n_cols + n] : Tcm[(long)(k0 + q) * N + col0 + n]) * v;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double a = hw_block_sum(du[q], sh.shd);
        const double b = hw_block_sum(dv[q], sh.shd);
        if (G > 1) {
          if (tid == 0 && k0 + q < rank - 1) { aca_st(mypart + 6 + 2 * (k0 + q), a, true); aca_st(mypart + 7 + 2 * (k0 + q), b, true); }
        } else {
          if (fabs(a) > maxu) maxu = fabs(a);
          if (fabs(b) > maxv) maxv = fabs(b);
        }
      }
    }
    }
    if (G > 1) {
      // (round 5) the NEXT step's first candidate row is drawn here and published with this barrier: the draw depends on the
      // generator and the row permutation alone, not on the norms, every member has read the current `sel` before it arrived at
      // B2, and a draw made in vain (the block converges below) changes nothing that is read again -- same draws in the same
      // order, one cluster barrier per step fewer (two instead of three)
      if ((multi & 2) && remaining > 0) {
        if (g == 0 && tid == 0) draw_row();
        --remaining;
        have_sel = true;
      }
      if (tid == 0) { aca_st(mypart + 3, un2, true); aca_st(mypart + 4, vn2, true); }     // (slots 0-2 may still be read by a slow member)
      if (!aca_barrier(bar, G, epoch, fail, fence)) return;                           // B3: norms (+ the next row)
      {
        double pu = 0.0, pv = 0.0;
        if (tid < G) { pu = aca_ld(allpart + (long)tid * pstride + 3); pv = aca_ld(allpart + (long)tid * pstride + 4); }
        un2 = hw_block_sum(pu, sh.shd);
        vn2 = hw_block_sum(pv, sh.shd);
      }
      {
        const int lane = tid & 63, wave = tid >> 6;          // wavefront w sums the G shares of the dot products k = w, w + 8, ...
        for (int k = wave; k < rank - 1; k += (nt >> 6)) {
          double a = 0.0, b = 0.0;
          for (int q = lane; q < G; q += 64) { a += aca_ld(allpart + (long)q * pstride + 6 + 2 * k); b += aca_ld(allpart + (long)q * pstride + 7 + 2 * k); }
          a = hw_wave_sum(a);
          b = hw_wave_sum(b);
          if (lane == 0) { sh.coef[k] = fabs(a); sh.coef[ACA_MAXR / 2 + k] = fabs(b); }   // (coef is free here: reloaded at the next step)
        }
      }
      __syncthreads();
      for (int k = 0; k < rank - 1; ++k) {
        if (sh.coef[k] > maxu) maxu = sh.coef[k];
        if (sh.coef[ACA_MAXR / 2 + k] > maxv) maxv = sh.coef[ACA_MAXR / 2 + k];
      }
      __syncthreads();
    }
    const double rowcol = un2 * vn2;
    if (rowcol < tol2 * norm) { converged = true; break; }                             // hodlr.h:206-207
    norm += rowcol;
    if (rank > 1) norm += 2.0 * maxu + 2.0 * maxv;
  }
  if (g == 0 && tid == 0) {
    ranks[node] = rank;
    if (dur) dur[node] = (int)(wall_clock64() - t_begin);
    if (!converged && rank < full_rank) atomicExch(trunc, 1);     // stopped by the cap, not by the tolerance
#ifdef GH_ACA_TIMES                                                // (build-time debugging aid: per-node durations of one-workgroup nodes)
    if (G == 1) { mypart[0] = (double)(wall_clock64() - dbg_t0); mypart[1] = (double)rank; mypart[2] = (double)remaining; mypart[3] = (double)dbg_passes; mypart[4] = (double)dbg_t0; }
#endif
  }
}

// ---------------------------------------------------------------------------------------------------------------
// ACA with ONE WAVEFRONT per node, for the deep levels whose blocks have at most 64 E rows and columns, E = 1, 2, 4 (levels
// 9 and 10 of C4 -- 256 x 256 and 128 x 128 blocks, 1536 of its 2047 nodes; the workgroup kernel above spent 124 of its
// 198 ms of workgroup time on them: a 512-thread workgroup, ~10 workgroup barriers and six block-wide reductions per ACA
// step for vectors of 128 or 256 entries, and one thread drawing up to 64 candidate rows per search pass).  Four nodes per
// 256-thread workgroup, no workgroup barrier anywhere.  Lane l owns rows and columns l + 64 e, e < E, and keeps ITS entries
// of the factors found so far (rank <= AW_RW) in registers: U[k][e], V[k][e].  What another lane's entry is needed for --
// the candidate row's coefficients U(i, :), the pivot column's V(j, :) -- travels by one shuffle per k.  LDS holds only the
// node's coordinates (1-D) and its row permutation: 4.5 KiB per node at E = 4, so these workgroups find room beside the
// cooperative launch, the leaf Cholesky and the one-workgroup nodes that share the chip with them in phase 1.
//
// SAME BITS as hodlr_aca_kernel with G = 1: the same generator and draws, candidates tested in drawing order (the first
// whose largest residual entry reaches 1e-14 wins -- what the workgroup kernel's batched search returns), residuals formed by
// the same expression with k ascending, and every sum reduced by the tree the workgroup kernel uses for <= 512 entries: there
// thread t holds element t alone, wavefront q reduces elements 64 q .. 64 q + 63 with the shfl_down tree and the wavefront
// results are added in order; here lane l holds elements l + 64 e, "virtual wavefront" e reduced by the same tree, then
// added in order.  Ranks, factors, log-determinants do not change by a bit (tests/test_gpu_hodlr.py).
// A node that needs more than AW_RW_OF(E) columns is NOT cut short: the launch raises the level's `trunc` word to 2 and the host
// redoes the level with the workgroup kernel (and remembers it for the handle's next compute()).
// rank capacity of the register mirrors: 8 columns, 6 where a lane holds four entries of each (256 x 256 blocks: 96 instead of 128
// registers of mirrors -- with 8 the kernel spilled 560 bytes per lane)
#define AW_RW_OF(E) ((E) >= 4 ? 6 : 8)
#define AW_NODES 4              // nodes (wavefronts) per workgroup
// (the lane's E entries of a vector as a clang extended vector, not an array: a run-time element index -- the candidate row's
//  slot -- is then an extractelement the backend lowers to selects; on arrays, however the selects were spelt, the optimiser
//  folded them back into a run-time array index and moved U and V to scratch memory)
template <int E> struct AwVec { typedef double type __attribute__((ext_vector_type(E))); };
template <> struct AwVec<1> { typedef double type __attribute__((ext_vector_type(2))); };      // (one entry used)
template <int E>
__device__ __forceinline__ double aw_sum(const typename AwVec<E>::type& x) {
  // (hw_block_sum of the workgroup kernel for <= 64 E entries: t = 0 + wave0 + wave1 + ...)
  double t = 0.0;
#pragma unroll
  for (int e = 0; e < E; ++e) t += __shfl(hw_wave_sum(x[e]), 0, 64);
  return t;
}
template <int E>
__device__ __forceinline__ double aw_pick(const typename AwVec<E>::type& x, int slot) {      // x[slot], slot wave-uniform
  return E == 1 ? x[0] : x[slot];
}
template <bool FAST, int E>
__global__ __launch_bounds__(64 * AW_NODES) void hodlr_aca_wave_kernel(
    const GhNode* __restrict__ prog, int n_prog, GhFast fast, int nd, const double* x, const LvlNode* nodes, int n_nodes, double* Tcm, long N,
    int rcap, int* ranks, double tol, unsigned long long seed, int level, int* trunc) {
  constexpr int MR = 64 * E;                            // rows / columns capacity
  constexpr int AW_RW = AW_RW_OF(E);
  __shared__ double xs_all[AW_NODES][2 * MR];           // 1-D: [0, MR) row coordinates, [MR, 2 MR) column coordinates
  __shared__ unsigned short lidx_all[AW_NODES][MR];     // row permutation
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int node = blockIdx.x * AW_NODES + wave;
  if (node >= n_nodes) return;                          // (no workgroup barrier in this kernel)
  double* const xs = xs_all[wave];
  unsigned short* const lidx = lidx_all[wave];
  const LvlNode nodev = nodes[node];
  const int col0 = nodev.start, n_cols = nodev.half;
  const int row0 = nodev.start + nodev.half, n_rows = nodev.size - nodev.half;
  const bool xlds = nd == 1;
  bool cm[E], rm[E];
#pragma unroll
  for (int e = 0; e < E; ++e) { cm[e] = lane + 64 * e < n_cols; rm[e] = lane + 64 * e < n_rows; }
  if (xlds) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (rm[e]) xs[lane + 64 * e] = x[row0 + lane + 64 * e];
      if (cm[e]) xs[MR + lane + 64 * e] = x[col0 + lane + 64 * e];
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) if (rm[e]) lidx[lane + 64 * e] = (unsigned short)(lane + 64 * e);
  auto xrow = [&](int m) -> const double* { return xlds ? (const double*)(xs + m) : x + (long)(row0 + m) * nd; };
  auto xcol = [&](int n) -> const double* { return xlds ? (const double*)(xs + MR + n) : x + (long)(col0 + n) * nd; };
  auto kval = [&](const double* a, const double* b) -> double { return FAST ? gh_fast_value(fast, a, b) : gh_eval_value(prog, n_prog, a, b); };
  const int full_rank = n_rows < n_cols ? n_rows : n_cols;
  int max_rank = full_rank;
  if (max_rank > rcap) max_rank = rcap;
  int remaining = n_rows, rank = 0;
  double norm = 0.0;
  const double tol2 = tol * tol;
  bool converged = false;
  unsigned long long st = seed ^ ((unsigned long long)(level + 1) << 40) ^ ((unsigned long long)(node + nodev.pad) * 0x9E3779B97F4A7C15ull);
  typedef typename AwVec<E>::type VE;
  VE U[AW_RW], V[AW_RW];
#pragma unroll
  for (int k = 0; k < AW_RW; ++k) { U[k] = (VE)(0.0); V[k] = (VE)(0.0); }
  __builtin_amdgcn_s_waitcnt(0);                        // (the wavefront's own LDS writes above)
  __builtin_amdgcn_wave_barrier();
  while (rank < max_rank) {
    if (rank >= AW_RW) {                                // more columns than the mirrors hold: the level goes to the workgroup kernel
      if (lane == 0) atomicMax(trunc, 2);
      return;
    }
    // ---- a random unused row with a non-negligible residual (hodlr.h:159-191): candidates one by one, in drawing order
    bool got = false;
    VE v = (VE)(0.0);
    while (remaining > 0) {
      st += 0x9E3779B97F4A7C15ull;
      unsigned long long z = st;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      const int kk = (int)(z % (unsigned long long)remaining);
      const int i = __builtin_amdgcn_readfirstlane((int)lidx[kk]);
      __builtin_amdgcn_wave_barrier();                  // (every lane has read lidx[kk] before lane 0 overwrites it)
      if (lane == 0) lidx[kk] = lidx[remaining - 1];
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
      --remaining;
      const int si = i >> 6, li = i & 63;
      double cw[AW_RW];
#pragma unroll
      for (int k = 0; k < AW_RW; ++k) cw[k] = (k < rank) ? __shfl(aw_pick<E>(U[k], si), li, 64) : 0.0;       // U(i, k)
      const double* xi = xrow(i);
      bool hit = false;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        double t = cm[e] ? kval(xi, xcol(lane + 64 * e)) : 0.0;
#pragma unroll
        for (int k = 0; k < AW_RW; ++k) if (k < rank) t -= cw[k] * V[k][e];
        v[e] = t;
        hit = hit || (cm[e] && fabs(t) >= 1e-14);       // hodlr.h:191 on the row's largest entry
      }
      if (__any(hit)) { got = true; break; }
    }
    if (!got) { converged = true; break; }              // rows exhausted (see hodlr_aca_kernel)
    // ---- pivot: largest |entry|, smallest column on ties
    int j;
    double pivot;
    {
      double best = -1.0;
      int bestn = -1;
#pragma unroll
      for (int e = 0; e < E; ++e) { const double a = cm[e] ? fabs(v[e]) : -1.0; if (cm[e] && a > best) { best = a; bestn = lane + 64 * e; } }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bestn, off, 64);
        if (ov > best || (ov == best && oi >= 0 && (bestn < 0 || oi < bestn))) { best = ov; bestn = oi; }
      }
      j = __builtin_amdgcn_readfirstlane(bestn);
      pivot = __shfl(aw_pick<E>(v, j >> 6), j & 63, 64);
    }
    // ---- normalise the row by its pivot, build the column (hodlr.h:194-199)
    VE vn = (VE)(0.0), un = (VE)(0.0), u = (VE)(0.0);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (cm[e]) { v[e] = v[e] / pivot; Tcm[(long)rank * N + col0 + lane + 64 * e] = v[e]; vn[e] = v[e] * v[e]; }
    }
    double cv[AW_RW];
#pragma unroll
    for (int k = 0; k < AW_RW; ++k) cv[k] = (k < rank) ? __shfl(aw_pick<E>(V[k], j >> 6), j & 63, 64) : 0.0;   // V(j, k)
    const double* xj = xcol(j);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      double t = rm[e] ? kval(xrow(lane + 64 * e), xj) : 0.0;
#pragma unroll
      for (int k = 0; k < AW_RW; ++k) if (k < rank) t -= cv[k] * U[k][e];
      u[e] = t;
      if (rm[e]) { Tcm[(long)rank * N + row0 + lane + 64 * e] = t; un[e] = t * t; }
    }
    // (column `rank` of the mirrors: selects with constant register indices -- written as `if (k == rank) V[k][e] = ...` the
    //  compiler turned the chain back into V[rank][e], a run-time index, and moved both arrays to scratch memory)
#pragma unroll
    for (int k = 0; k < AW_RW; ++k) {
      const bool here = (k == rank);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        V[k][e] = here ? (cm[e] ? v[e] : 0.0) : V[k][e];
        U[k][e] = here ? (rm[e] ? u[e] : 0.0) : U[k][e];
      }
    }
    ++rank;
    if (rank >= full_rank) { converged = true; break; }                                // hodlr.h:203
    if (rank >= max_rank) break;                                                       // rank cap: NOT converged
    const double un2 = aw_sum<E>(un), vn2 = aw_sum<E>(vn);
    // cross terms |u_new . u_k|, |v_new . v_k|, k < rank - 1 (hodlr.h:210-214)
    double maxu = 0.0, maxv = 0.0;
#pragma unroll
    for (int k = 0; k < AW_RW - 1; ++k)
      if (k < rank - 1) {
        VE pu = (VE)(0.0), pv = (VE)(0.0);
#pragma unroll
        for (int e = 0; e < E; ++e) { pu[e] = rm[e] ? U[k][e] * u[e] : 0.0; pv[e] = cm[e] ? V[k][e] * v[e] : 0.0; }
        const double a = aw_sum<E>(pu), b = aw_sum<E>(pv);
        if (fabs(a) > maxu) maxu = fabs(a);
        if (fabs(b) > maxv) maxv = fabs(b);
      }
    const double rowcol = un2 * vn2;
    if (rowcol < tol2 * norm) { converged = true; break; }                             // hodlr.h:206-207
    norm += rowcol;
    if (rank > 1) norm += 2.0 * maxu + 2.0 * maxv;
  }
  if (lane == 0) {
    ranks[node] = rank;
    if (!converged && rank < full_rank) atomicMax(trunc, 1);     // stopped by the caller's cap, not by the tolerance
  }
}
// (static + dynamic LDS of a launch with the mirrors is 67 KiB: above the 64 KiB a kernel gets without asking; per device)
static int aca_lds_attr() {
  static thread_local unsigned long long done = 0;
  int dev = 0;
  GH_HIP(hipGetDevice(&dev));
  if (dev < 64 && (done >> dev & 1ull)) return GH_OK;
  GH_HIP(hipFuncSetAttribute((const void*)hodlr_aca_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, ACA_DYN_BYTES));
  GH_HIP(hipFuncSetAttribute((const void*)hodlr_aca_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, ACA_DYN_BYTES));
  if (dev < 64) done |= 1ull << dev;
  return GH_OK;
}

int hodlr_launch_aca(const gh_hodlr* h, const gh_kernel* k, const AcaLaunch& a, hipStream_t st) {
  GH_CHECK(aca_lds_attr());
#define GH_ACA_LAUNCH(F, CLU)                                                                                          \
  hipLaunchKernelGGL((hodlr_aca_kernel<F, CLU>), dim3(a.nwg), dim3(ACA_THREADS), a.ones_only ? ACA_DYN_BYTES : 0, st, k->d_nodes,     \
                     (int)k->nodes.size(), k->fast, a.ndim, a.x, a.nodes, a.Tcm, a.N, a.rc, a.idx, a.ranks, h->opts.tol,              \
                     (unsigned long long)(unsigned)h->opts.seed, a.level, a.G, a.bars, a.part, a.pstride, a.sel, a.fail, a.multi,     \
                     a.fence, a.trunc, a.segs, a.nseg, a.ones_only ? ACA_CAPD : 0)
  if (a.ones_only) { if (k->fast.ok) GH_ACA_LAUNCH(true, false); else GH_ACA_LAUNCH(false, false); }
  else             { if (k->fast.ok) GH_ACA_LAUNCH(true, true); else GH_ACA_LAUNCH(false, true); }
#undef GH_ACA_LAUNCH
  GH_HIP(hipGetLastError());
  return GH_OK;
}

int hodlr_launch_aca_wave(const gh_hodlr* h, const gh_kernel* k, int ndim, const LvlNode* nodes, int nn, int mr, double* Tcm, long N,
                          int rc, int* ranks, int level, int* trunc, hipStream_t st) {
#define GH_ACA_WAVE(F, EE)                                                                                        \
  hipLaunchKernelGGL((hodlr_aca_wave_kernel<F, EE>), dim3((nn + AW_NODES - 1) / AW_NODES), dim3(64 * AW_NODES), 0, st, \
                     k->d_nodes, (int)k->nodes.size(), k->fast, ndim, h->x.d(), nodes, nn, Tcm, N, rc,           \
                     ranks, h->opts.tol, (unsigned long long)(unsigned)h->opts.seed, level, trunc)
  if (k->fast.ok) { if (mr == 64) GH_ACA_WAVE(true, 1); else if (mr == 128) GH_ACA_WAVE(true, 2); else GH_ACA_WAVE(true, 4); }
  else            { if (mr == 64) GH_ACA_WAVE(false, 1); else GH_ACA_WAVE(false, 2); }
#undef GH_ACA_WAVE
  GH_HIP(hipGetLastError());
  return GH_OK;
}
