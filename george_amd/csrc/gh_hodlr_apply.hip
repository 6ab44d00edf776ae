// gh_hodlr_apply.hip -- applying a HODLR factor to right-hand sides (gh_hodlr_impl.h has the map of the units): the batched small
// dense products behind every apply, their launchers, the level and leaf applies, the solves and their entry points.
#include <atomic>
#include "gh_hodlr_impl.h"
#include "gh_device_util.h"

// UL (level-major) <- UA (row-major n x Rtot): column c of row i goes to UL[colbase[c] + i * colld[c]]
__global__ void hodlr_relayout_kernel(const double* UA, long n, int Rtot, const long* colbase, const int* colld, double* UL) {
  const long tot = n * Rtot;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const long i = e / Rtot;
    const int c = (int)(e % Rtot);
    UL[colbase[c] + i * colld[c]] = UA[e];
  }
}

// =============================================================== batched small dense products
// O(job rows, 0:C) (=|-=) A_job (m x kd) * B(job rows, 0:C); A element (r, k) at
// A[a_off + r*a_rs + k*a_cs]; B row b_row+k at B[(b_row+k)*ldb + b_col0 + c].
struct MMArgs {
  const MMJob* jobs;
  const double* A; long a_rs, a_cs;
  const double* B; long ldb, b_col0;
  double* O; long ldo, o_col0;
  int C, subtract, mtiles;
};
__global__ __launch_bounds__(256) void hodlr_mm_kernel(MMArgs a) {
  __shared__ double As[32 * 33];
  __shared__ double Bs[32 * 64];
  const MMJob job = a.jobs[blockIdx.x];
  const int c0 = blockIdx.z * 64, tid = threadIdx.x;
  // 32 x 64 tile on the matrix pipe: wavefront w takes the 16-row block w & 1 and the two 16-column
  // blocks 2 (w >> 1), 2 (w >> 1) + 1; operands are staged in LDS exactly as for the VALU loop this
  // replaced (8 FMAs per staged element and lane -> 2 MFMAs per 4 k)
  const int lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int bi = wave & 1, bj = 2 * (wave >> 1);
  typedef double mm_v4d __attribute__((ext_vector_type(4)));
  const bool rfast = (a.a_rs == 1);
  for (int mt = 0; mt < a.mtiles; ++mt) {
    const int m0 = (blockIdx.y * a.mtiles + mt) * 32;
    if (m0 >= job.m) break;                                   // (uniform)
    mm_v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < job.kd; k0 += 32) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = tid + 256 * q;
        const int r = rfast ? (e & 31) : (e >> 5), k = rfast ? (e >> 5) : (e & 31);
        double v = 0.0;
        if (m0 + r < job.m && k0 + k < job.kd) v = a.A[job.a_off + (long)(m0 + r) * a.a_rs + (long)(k0 + k) * a.a_cs];
        As[r * 33 + k] = v;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = tid + 256 * q;
        const int k = e >> 6, cc = e & 63;
        double v = 0.0;
        if (k0 + k < job.kd && c0 + cc < a.C) v = a.B[(long)(job.b_row + k0 + k) * a.ldb + a.b_col0 + c0 + cc];
        Bs[k * 64 + cc] = v;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const double av = As[(16 * bi + fr) * 33 + 4 * kk + fk];
        const double b0 = Bs[(4 * kk + fk) * 64 + 16 * bj + fr];
        const double b1 = Bs[(4 * kk + fk) * 64 + 16 * bj + 16 + fr];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
      }
      __syncthreads();
    }
    // f64 MFMA C/D map: row = (lane >> 4) + 4 reg, col = lane & 15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + 16 * bi + fk + 4 * r;
      if (row >= job.m) continue;
      double* o = a.O + (long)(job.o_row + row) * a.ldo + a.o_col0 + c0 + 16 * bj + fr;
      if (c0 + 16 * bj + fr < a.C) o[0] = a.subtract ? (o[0] - acc0[r]) : acc0[r];
      if (c0 + 16 * bj + 16 + fr < a.C) o[16] = a.subtract ? (o[16] - acc1[r]) : acc1[r];
    }
  }
}
// ------------------------------------------------------------ narrow right-hand sides (C <= 8)
// The tile kernel above does a full 32 x 64 x 32 block of matrix-pipe work per staged slab whatever
// the real extents: for ONE right-hand side (every log-likelihood evaluation) 63 of its 64 columns
// are padding, and a level pass of a solve cost ~50 us for a few MFLOP.  These do the same three
// steps with plain FMAs on exactly the data there is.
// P[(o_row + r) * Cp + c] = sum_k V(r, k) X(b_row + k, c);  V(r, k) at A[a_off + r + k * R]  (level-major V block)
__global__ __launch_bounds__(256) void hodlr_mv_reduce_kernel(const MMJob* jobs, const double* A, int R, const double* X, long ldx,
                                                              long xcol0, double* P, long Cp, int C) {
  __shared__ double part[8][32][MV_C];
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x, r = tid & 31, pt = tid >> 5;
  for (int r0 = 0; r0 < R; r0 += 32) {
    double acc[MV_C];
#pragma unroll
    for (int c = 0; c < MV_C; ++c) acc[c] = 0.0;
    if (r0 + r < R) {
      for (int k = pt; k < job.kd; k += 8) {
        const double v = A[job.a_off + (long)k * R + r0 + r];
        const double* xr = X + (long)(job.b_row + k) * ldx + xcol0;
#pragma unroll
        for (int c = 0; c < MV_C; ++c) if (c < C) acc[c] += v * xr[c];
      }
    }
#pragma unroll
    for (int c = 0; c < MV_C; ++c) part[pt][r][c] = acc[c];
    __syncthreads();
    if (pt == 0 && r0 + r < R) {
      for (int c = 0; c < C; ++c) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) v += part[q][r][c];
        P[(long)(job.o_row + r0 + r) * Cp + c] = v;
      }
    }
    __syncthreads();
  }
}
// X(o_row + i, c) -= sum_k U(i, k) T(b_row + k, c);  U(i, k) at A[a_off + i * a_rs + k], i < m, k < kd <= 32
__global__ __launch_bounds__(128) void hodlr_mv_update_kernel(const MMJob* jobs, const double* A, long a_rs, const double* T, long Cp,
                                                              double* X, long ldx, long xcol0, int C) {
  __shared__ double ts[32 * MV_C];
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  for (int e = tid; e < job.kd * C; e += 128) ts[(e / C) * MV_C + (e % C)] = T[(long)(job.b_row + e / C) * Cp + (e % C)];
  __syncthreads();
  if (tid >= job.m) return;
  double acc[MV_C];
#pragma unroll
  for (int c = 0; c < MV_C; ++c) acc[c] = 0.0;
  const double* ur = A + job.a_off + (long)tid * a_rs;
  for (int k = 0; k < job.kd; ++k) {
    const double u = ur[k];
#pragma unroll
    for (int c = 0; c < MV_C; ++c) acc[c] += u * ts[k * MV_C + c];
  }
  double* xr = X + (long)(job.o_row + tid) * ldx + xcol0;
#pragma unroll
  for (int c = 0; c < MV_C; ++c) if (c < C) xr[c] -= acc[c];
}
// X rows of leaf b <- Kinv_b X rows (in place: the leaf's rows are staged in LDS first); leaf size <= 256
__global__ __launch_bounds__(256) void hodlr_mv_leaf_kernel(const MMJob* jobs, const double* Kinv, long pitch, double* X, long ldx,
                                                            long xcol0, int C) {
  __shared__ double xs[256 * MV_C];
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = job.m;
  for (int e = tid; e < n * C; e += 256) xs[(e / C) * MV_C + (e % C)] = X[(long)(job.b_row + e / C) * ldx + xcol0 + (e % C)];
  __syncthreads();
  for (int i = wave; i < n; i += 4) {
    const double* row = Kinv + job.a_off + (long)i * pitch;
    double acc[MV_C];
#pragma unroll
    for (int c = 0; c < MV_C; ++c) acc[c] = 0.0;
    for (int k = lane; k < n; k += 64) {
      const double a = row[k];
#pragma unroll
      for (int c = 0; c < MV_C; ++c) acc[c] += a * xs[k * MV_C + c];
    }
#pragma unroll
    for (int c = 0; c < MV_C; ++c) {
      if (c < C) {
        const double v = hw_wave_sum(acc[c]);
        if (lane == 0) X[(long)(job.o_row + i) * ldx + xcol0 + c] = v;
      }
    }
  }
}
// Tsum for narrow right-hand sides: 32 threads per column each add a contiguous slice of the chunks,
// one thread then adds the 32 slice sums in order (the serial walk over up to N/256 chunks by a
// single active lane took 55-60 us at the top levels)
__global__ __launch_bounds__(256) void hodlr_sum_narrow_kernel(const double* P, const int* crange, int R, long Cp, int C, double* Tsum) {
  __shared__ double sl[32][MV_C];
  const int node = blockIdx.x, row = blockIdx.y;
  const int half = row < R ? 1 : 0, k = row < R ? row : row - R;
  const int cb = crange[(node * 2 + half) * 2], ce = crange[(node * 2 + half) * 2 + 1];
  const int c = threadIdx.x & 7, sidx = threadIdx.x >> 3;
  const int per = (ce - cb + 31) / 32;
  const int lo = cb + sidx * per, hi = lo + per < ce ? lo + per : ce;
  double v = 0.0;
  if (c < C) for (int ch = lo; ch < hi; ++ch) v += P[((long)ch * R + k) * Cp + c];
  sl[sidx][c] = v;
  __syncthreads();
  if (threadIdx.x < C) {
    double t = 0.0;
    for (int q = 0; q < 32; ++q) t += sl[q][threadIdx.x];
    Tsum[((long)node * 2 * R + row) * Cp + threadIdx.x] = t;
  }
}
// ---- round 5: the narrow solve (C <= 8 right-hand sides: every log-likelihood) in fewer, better-shaped launches.
// Round 4's solve of C4 (N = 262144, one right-hand side) was 45 launches, 0.57 ms: the leaf kernel walked 32 rows per
// wavefront with one exposed HBM round trip each (110 us for 268 MB), the per-chunk reduce kept R of every 32 lanes busy in a
// serial walk over the chunk's rows (21 us per level for 8 MB), and each level paid four dispatches.
//
// X rows of a leaf <- K_leaf^-1 X rows, thread = OUTPUT ROW: K^-1 is symmetric, so row i of the product is the sum over k of
// column i of row k -- every load of a wavefront is one contiguous 512-byte piece of row k, no reduction across lanes, and
// eight rows' loads are in flight per thread.  The rows k are split over 256 / (padded leaf size) thread groups whose partial
// sums are added in a fixed order.  (K^-1 = L^-T L^-1 is symmetric up to rounding: its (i, k) and (k, i) entries may differ
// in the last bit, as may the sum order from the row form -- the results agree to rounding, tests/test_gpu_hodlr.py.)
__global__ __launch_bounds__(256) void hodlr_mv_leaf_sym_kernel(const MMJob* jobs, const double* Kinv, long pitch, double* X, long ldx,
                                                                long xcol0, int C) {
  __shared__ double xs[256 * MV_C];
  __shared__ double part[256 * MV_C];
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x, n = job.m;
  for (int e = tid; e < n * C; e += 256) xs[(e / C) * MV_C + (e % C)] = X[(long)(job.b_row + e / C) * ldx + xcol0 + (e % C)];
  __syncthreads();
  const int S = n <= 64 ? 4 : (n <= 128 ? 2 : 1), per_row = 256 / S;
  const int i = tid % per_row, sidx = tid / per_row;
  const int kper = (n + S - 1) / S, k_lo = sidx * kper, k_hi = min(n, k_lo + kper);
  double acc[MV_C];
#pragma unroll
  for (int c = 0; c < MV_C; ++c) acc[c] = 0.0;
  if (i < n) {
    const double* col = Kinv + job.a_off + i;
    int k = k_lo;
    for (; k + 8 <= k_hi; k += 8) {
      double a[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) a[q] = col[(long)(k + q) * pitch];
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int c = 0; c < MV_C; ++c) if (c < C) acc[c] += a[q] * xs[(k + q) * MV_C + c];
    }
    for (; k < k_hi; ++k) {
      const double a = col[(long)k * pitch];
#pragma unroll
      for (int c = 0; c < MV_C; ++c) if (c < C) acc[c] += a * xs[k * MV_C + c];
    }
  }
#pragma unroll
  for (int c = 0; c < MV_C; ++c) part[tid * MV_C + c] = acc[c];
  __syncthreads();
  if (sidx == 0 && i < n) {
    for (int c = 0; c < C; ++c) {
      double v = part[i * MV_C + c];
      for (int q = 1; q < S; ++q) v += part[(q * per_row + i) * MV_C + c];
      X[(long)(job.o_row + i) * ldx + xcol0 + c] = v;
    }
  }
}
// One pass over the rows of a chunk for TWO neighbouring levels of the sweep (either part may be absent):
//   update (level l):   X(rows, c) -= sum_k U_l(row, k) T_l(b_row + k, c)                  [hodlr_mv_update_kernel]
//   reduce (level l'):  P[(o_row + r) Cp + c] = sum_rows V_l'(row, r) X(row, c)             [hodlr_mv_reduce_kernel]
// l' is the next shallower level with a positive rank and the SAME chunks (HLevel::chunk_geom): what the reduce reads is what
// the update has just written, kept in LDS.  Reduce: wavefront w takes the columns r = w, w + 4, ... of V, lane = row (and
// row + 64), one wavefront sum per (r, c) -- all lanes busy whatever R is, every load issued before the first sum.
__global__ __launch_bounds__(256) void hodlr_mv_updred_kernel(const MMJob* ujobs, const double* U, long u_rs, const double* T,
                                                              const MMJob* rjobs, const double* V, int R2, double* P,
                                                              long Cp, double* X, long ldx, long xcol0, int C) {
  __shared__ double ts[32 * MV_C];
  __shared__ double xs[128 * MV_C];
  extern __shared__ double us[];                     // [128][up]: the chunk's rows of U_l; up = 17 or 33 (the launch sizes it: 17 KiB
                                                     // instead of 33 lets all 2048 workgroups of a C4 level be resident at once)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int row0, m;
  // the reduce's V values first (they do not depend on the update): wavefront w, columns r = w + 4 q, rows lane and lane + 64
  double v0[8], v1[8];
  MMJob rj = {0, 0, 0, 0, 0};
  if (rjobs) {
    rj = rjobs[blockIdx.x];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = wave + 4 * q;
      v0[q] = (r < R2 && lane < rj.kd) ? V[rj.a_off + (long)lane * R2 + r] : 0.0;
      v1[q] = (r < R2 && lane + 64 < rj.kd) ? V[rj.a_off + (long)(lane + 64) * R2 + r] : 0.0;
    }
  }
  if (ujobs) {
    const MMJob job = ujobs[blockIdx.x];
    row0 = job.o_row; m = job.m;
    double xold[MV_C];                                // (requested with everything else: one round trip for the whole update)
    if (tid < m) {
#pragma unroll
      for (int c = 0; c < MV_C; ++c) xold[c] = c < C ? X[(long)(row0 + tid) * ldx + xcol0 + c] : 0.0;
    }
    for (int e = tid; e < job.kd * C; e += 256) ts[(e / C) * MV_C + (e % C)] = T[(long)(job.b_row + e / C) * Cp + (e % C)];
    // the chunk's rows of U_l through LDS, all 256 threads, element e = (row, k) with k fastest: consecutive lanes read the kd
    // contiguous doubles of a row, then the next row (U is row-major with pitch u_rs here: one thread per row reading its kd
    // values in turn was 64 scattered 8-byte requests per load instruction)
    const int kd = job.kd, up = kd <= 16 ? 17 : 33;
    for (int e0 = tid; e0 < m * kd; e0 += 8 * 256) {           // eight loads in flight per thread (a rolled loop waits for each in turn)
      double uv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + 256 * q, r_ = e / kd, k_ = e - r_ * kd;
        uv[q] = e < m * kd ? U[job.a_off + (long)r_ * u_rs + k_] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + 256 * q, r_ = e / kd, k_ = e - r_ * kd;
        if (e < m * kd) us[r_ * up + k_] = uv[q];
      }
    }
    __syncthreads();
    if (tid < m) {
      double acc[MV_C];
#pragma unroll
      for (int c = 0; c < MV_C; ++c) acc[c] = 0.0;
      for (int k = 0; k < kd; ++k) {
        const double u = us[tid * up + k];
#pragma unroll
        for (int c = 0; c < MV_C; ++c) acc[c] += u * ts[k * MV_C + c];
      }
      double* xr = X + (long)(row0 + tid) * ldx + xcol0;
#pragma unroll
      for (int c = 0; c < MV_C; ++c)
        if (c < C) { const double v = xold[c] - acc[c]; xr[c] = v; xs[tid * MV_C + c] = v; }
    }
  } else {
    row0 = rj.b_row; m = rj.kd;
    for (int e = tid; e < m * C; e += 256) xs[(e / C) * MV_C + (e % C)] = X[(long)(row0 + e / C) * ldx + xcol0 + (e % C)];
  }
  if (!rjobs) return;
  __syncthreads();
  const bool k0 = lane < m, k1 = lane + 64 < m;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int r = wave + 4 * q;
    if (r >= R2) break;                              // (uniform)
    for (int c = 0; c < C; ++c) {
      double t = v0[q] * (k0 ? xs[lane * MV_C + c] : 0.0);
      t += v1[q] * (k1 ? xs[(lane + 64) * MV_C + c] : 0.0);
      t = hw_wave_sum(t);
      if (lane == 0) P[(long)(rj.o_row + r) * Cp + c] = t;
    }
  }
}
// Per node: Tsum = the chunk partials of each half added up (as hodlr_sum_narrow_kernel: 32 slices, then the slice sums in
// order), then Tout = S^-1 Tsum, the 2R x 2R core inverse times 2R x C, in the same workgroup (hodlr.h:247-252).
__global__ __launch_bounds__(256) void hodlr_mv_summm_kernel(const double* P, const int* crange, int R, long Cp, int C, const double* Sinv,
                                                             double* Tout) {
  __shared__ double sl[32][MV_C];
  __shared__ double tsum[64 * MV_C];
  const int node = blockIdx.x, n2 = 2 * R;
  const int c = threadIdx.x & 7, sidx = threadIdx.x >> 3;
  for (int row = 0; row < n2; ++row) {
    const int half = row < R ? 1 : 0, k = row < R ? row : row - R;
    const int cb = crange[(node * 2 + half) * 2], ce = crange[(node * 2 + half) * 2 + 1];
    const int per = (ce - cb + 31) / 32;
    const int lo = cb + sidx * per, hi = lo + per < ce ? lo + per : ce;
    double v = 0.0;
    if (c < C) for (int ch = lo; ch < hi; ++ch) v += P[((long)ch * R + k) * Cp + c];
    sl[sidx][c] = v;
    __syncthreads();
    if (threadIdx.x < MV_C) {
      double t = 0.0;
      for (int q = 0; q < 32; ++q) t += sl[q][threadIdx.x];
      tsum[row * MV_C + threadIdx.x] = threadIdx.x < C ? t : 0.0;
    }
    __syncthreads();
  }
  const double* S = Sinv + (long)node * n2 * n2;
  for (int e = threadIdx.x; e < n2 * MV_C; e += 256) {
    const int i = e >> 3, cc = e & 7;
    if (cc >= C) continue;
    double t = 0.0;
    for (int k = 0; k < n2; ++k) t += S[i * n2 + k] * tsum[k * MV_C + cc];
    Tout[((long)node * n2 + i) * Cp + cc] = t;
  }
}
// Tsum[node][0:R] = sum of the partials of its half-1 chunks, [R:2R] = half-0 chunks (hodlr.h:247-249)
// blockDim = 64 x NS: NS threads per column each add a contiguous slice of the node's chunks, the first
// then adds the NS slice sums in order (fixed order: reproducible).  The top levels have up to N/256
// chunks per half: as one thread per column this walk took 55-60 us per launch.
__global__ __launch_bounds__(64 * SUM_NS) void hodlr_sum_kernel(const double* P, const int* crange /* [node][half][2] */, int R, long Cp, int C, double* Tsum) {
  __shared__ double sl[SUM_NS][64];
  const int node = blockIdx.x, row = blockIdx.y;          // row in [0, 2R)
  const int half = row < R ? 1 : 0, k = row < R ? row : row - R;
  const int cb = crange[(node * 2 + half) * 2], ce = crange[(node * 2 + half) * 2 + 1];
  const int lane = threadIdx.x & 63, sidx = threadIdx.x >> 6;
  const int per = (ce - cb + SUM_NS - 1) / SUM_NS;
  const int lo = cb + sidx * per, hi = lo + per < ce ? lo + per : ce;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    double v = 0.0;
    if (c < C) {
#pragma unroll 8                                  // (loads of 8 chunks in flight; the sum stays in chunk order)
      for (int ch = lo; ch < hi; ++ch) v += P[((long)ch * R + k) * Cp + c];
    }
    sl[sidx][lane] = v;
    __syncthreads();
    if (sidx == 0 && c < C) {
      double t = 0.0;
#pragma unroll
      for (int q = 0; q < SUM_NS; ++q) t += sl[q][lane];
      Tsum[((long)node * 2 * R + row) * Cp + c] = t;
    }
    __syncthreads();
  }
}
// S = [[I, V1^T U1], [V0^T U0, I]]  (hodlr.h:229-232) from Tsum (C == R)
__global__ void hodlr_sbuild_kernel(const double* Tsum, long Cp, int R, double* S) {
  const int node = blockIdx.x, n2 = 2 * R;
  double* s = S + (long)node * n2 * n2;
  for (int e = threadIdx.x; e < n2 * n2; e += blockDim.x) {
    const int r = e / n2, c = e % n2;
    double v = (r == c) ? 1.0 : 0.0;
    if (r < R && c >= R) v = Tsum[((long)node * n2 + r) * Cp + (c - R)];
    else if (r >= R && c < R) v = Tsum[((long)node * n2 + r) * Cp + c];
    s[e] = v;
  }
}
__global__ void hodlr_copyrows_kernel(const double* Y, long ldy, double* X, long ldx, long x_col0, long n, int C) {
  const long tot = n * C;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const long i = e / C;
    const int c = (int)(e % C);
    X[i * ldx + x_col0 + c] = Y[i * ldy + c];
  }
}
// out[blockIdx.x] = sum over this workgroup's contiguous slice of a[i] * b[i] (b == nullptr: of a[i]);
// called twice: 256 slices, then one workgroup over the 256 partials -- fixed order, reproducible
__global__ __launch_bounds__(256) void hodlr_dot_kernel(const double* a, const double* b, long n, double* out) {
  __shared__ double sh[4];
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double v = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) v += b ? a[i] * b[i] : a[i];
  v = hw_block_sum(v, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}
// columns [col0, col0 + cw) of the identity into a zeroed strip of row pitch ld (the whole identity: ld = cw = n, col0 = 0)
__global__ void hodlr_eye_strip_kernel(double* p, long ld, long col0, int cw) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < cw) p[(col0 + t) * ld + t] = 1.0;
}

// rows [0, nrows) x columns [0, 16 ct) of a row-major block into LDS (pitch xp), zero where row >= nrows or
// column >= C; eight independent loads in flight per thread (a rolled load-store loop waits for every load in turn:
// 40 round trips per workgroup)
__device__ __forceinline__ void hodlr_stage_rows_va(double* Xs, int xp, const LeafSrc& ls, int row0, int nrows, int C, int ct) {
  // column c of the image = column k of level l: element (r, c) at VA[colbase[c] + (row0 + r) colR[c]], colbase[c] = offv[l] + k.
  // Lanes take consecutive COLUMNS (LDS writes free of bank conflicts at a pitch that is a multiple of 16 doubles; the reads are
  // the levels' pieces of a row, 24-120 contiguous bytes each, whose neighbours the next row's loads find in the caches)
  const int tid = threadIdx.x, w = 16 * ct;
  const int c = tid & 127, rh = tid >> 7;            // two rows per step
  const bool cok = c < C;
  long cb = 0;                                       // (no table in LDS: the image is exactly half a CU's LDS at CT = 5)
  int cr = 0;
  for (int t = 0; t < ls.nlev; ++t)
    if (cok && ls.R[t] > 0 && ls.off[t] <= c) { cb = ls.offv[t] + (c - ls.off[t]); cr = ls.R[t]; }
  if (c < w) {
#pragma unroll 1
    for (int r0 = 0; r0 < 128; r0 += 16) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + 2 * q + rh;
        v[q] = (cok && r < nrows) ? ls.VA[cb + (long)(row0 + r) * cr] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) Xs[(r0 + 2 * q + rh) * xp + c] = v[q];
    }
  }
}
__device__ __forceinline__ void hodlr_stage_rows(double* Xs, int xp, const double* src, long ld, int nrows, int C, int ct) {
  const int w = 16 * ct, tot = 128 * w;
  for (int e0 = threadIdx.x; e0 < tot; e0 += 8 * 256) {
    double v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = e0 + 256 * q, r = e / w, c = e - r * w;
      const bool ok = e < tot && r < nrows && c < C;
      v[q] = src[ok ? (long)r * ld + c : 0];
      if (!ok) v[q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = e0 + 256 * q, r = e / w, c = e - r * w;
      if (e < tot) Xs[r * xp + c] = v[q];
    }
  }
}

// X_leaf <- K_leaf^-1 X_leaf for every leaf, in place, ONE workgroup per leaf: the leaf's rows of X (<= 128 x
// 16 CT columns) are staged in LDS once, K_leaf^-1 (a 128 x 128 slot, identity- or zero-padded) streams through
// the A operand straight from HBM, the 128 x 16 CT result goes back over the rows it came from.  The generic tile
// kernel took this as 16384 workgroups of one 32 x 64 tile each into a scratch copy (every U row staged four times,
// every K^-1 slab twice) plus a copy back: 505 + 57 us of the C4 sweep for 0.6 GB of traffic.
// Wavefront w: row tiles 2w, 2w+1 (16 rows each) x all CT column tiles.
// rjobs != nullptr (round 5): the chunk products V^T X of the deepest level with a positive rank -- whose chunks are the
// leaves -- are formed here too, from the result tiles while they are in registers (see hodlr_updred_kernel: the result
// layout is the B operand layout of hodlr_red_kernel's k-steps, same order, same bits), saving that level's pass over U.
template <int CT>
__global__ __launch_bounds__(256) void hodlr_leaf_apply_kernel(const MMJob* __restrict__ jobs, const double* __restrict__ Kinv,
                                                               double* __restrict__ X, long ldx, long xcol0, int C,
                                                               const MMJob* __restrict__ rjobs = nullptr, const double* __restrict__ V2 = nullptr,
                                                               int R2 = 0, double* __restrict__ P = nullptr, long ldp = 0, LeafSrc ls = LeafSrc()) {
  // (no padding column: at CT = 5 the image is then exactly 80 KiB and TWO workgroups share a CU's 160 KiB -- with 81 columns
  //  it was 83 KiB, one workgroup = one wavefront per SIMD and nothing to hide the A operand's HBM latency behind; the price is
  //  a two-way bank conflict between the lane groups fk and fk + 2 of a B fragment read)
  constexpr int XP = 16 * CT;
  __shared__ double Xs[128 * XP];
  typedef double la_v4d __attribute__((ext_vector_type(4)));
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  double* const xb = X + (long)job.b_row * ldx + xcol0;
  const int ct = (C + 15) >> 4;                   // column tiles that hold anything (uniform)
  if (ls.VA) hodlr_stage_rows_va(Xs, XP, ls, job.b_row, job.m, C, ct);      // (the factorisation's first pass: X is written here for the first time)
  else hodlr_stage_rows(Xs, XP, xb, ldx, job.m, C, ct);
  __syncthreads();
  la_v4d acc[2][CT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = (la_v4d){0.0, 0.0, 0.0, 0.0};
  // A operand: K^-1(row 32 wave + 16 i + fr, k = 4 kk + fk), read as its mirror image K^-1(k, row) -- the leaf inverse is
  // symmetric (up to the last bit) and in this form the 16 lanes fr of a load are 128 contiguous bytes of row k instead of
  // 16 rows x 8 bytes (round 5: 208 -> see profiles/r05/hodlr_passes.md)
  const double* const ka = Kinv + job.a_off + (long)fk * 128 + 32 * wave + fr;
#pragma unroll 1
  for (int k0 = 0; k0 < 32; k0 += 8) {
    double a[8][2];
#pragma unroll
    for (int q = 0; q < 8; ++q) { a[q][0] = ka[(long)(4 * (k0 + q)) * 128]; a[q][1] = ka[(long)(4 * (k0 + q)) * 128 + 16]; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double* const bp = Xs + (4 * (k0 + q) + fk) * XP + fr;
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        if (j >= ct) continue;
        const double b = bp[16 * j];
        acc[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][0], b, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][1], b, acc[1][j], 0, 0, 0);
      }
    }
  }
  // f64 MFMA C/D map: row = (lane >> 4) + 4 reg, col = lane & 15
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 32 * wave + 16 * i + fk + 4 * r;
      if (row >= job.m) continue;
#pragma unroll
      for (int j = 0; j < CT; ++j)
        if (16 * j + fr < C) xb[(long)row * ldx + 16 * j + fr] = acc[i][j][r];
    }
  if (!rjobs) return;                             // (uniform)
  const MMJob rj = rjobs[blockIdx.x];
  la_v4d acc2[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc2[j] = (la_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 8; ++q) {                   // k-step q = 4 i + r: rows 32 wave + 16 i + 4 r + fk
    const int row = 4 * (8 * wave + q) + fk;
    const double a2 = (fr < R2 && row < rj.kd) ? V2[rj.a_off + (long)row * R2 + fr] : 0.0;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      if (j >= ct) continue;
      // (what hodlr_red_kernel would read back from its LDS image of X: zero outside the leaf's rows and the C columns)
      const double bv = (row < job.m && 16 * j + fr < C) ? acc[q >> 2][j][q & 3] : 0.0;
      acc2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bv, acc2[j], 0, 0, 0);
    }
  }
  __syncthreads();                                // (every wavefront is done with Xs)
  double* const part = Xs;                        // [3][CT][4][64]
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(((wave - 1) * CT + j) * 4 + r) * 64 + lane] = acc2[j][r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = fk + 4 * r, c = 16 * j + fr;
        if (k < R2 && c < C) {
          const double v = ((acc2[j][r] + part[((0 * CT + j) * 4 + r) * 64 + lane]) + part[((1 * CT + j) * 4 + r) * 64 + lane]) +
                           part[((2 * CT + j) * 4 + r) * 64 + lane];
          P[(long)(rj.o_row + k) * ldp + c] = v;
        }
      }
  }
}

// The per-chunk products V_l^T U of the factorisation sweep (R <= 16 columns of V, <= 128 rows of a chunk, C <= 16 CT
// columns of U), ONE workgroup per chunk in the manner of hodlr_leaf_apply_kernel: the chunk's rows of U staged in
// LDS once, V^T as the A operand straight from HBM (row k of the result = column k of V), the K = 128 rows split
// over the four wavefronts and their partial tiles added in a fixed order (bitwise repeatable).
//   O[(o_row + k) * ldo + o_col0 + c] = sum_row A[a_off + k + row * R] * B[(b_row + row) * ldb + b_col0 + c]
template <int CT>
__global__ __launch_bounds__(256) void hodlr_red_kernel(const MMJob* __restrict__ jobs, const double* __restrict__ A, int R,
                                                        const double* __restrict__ B, long ldb, long b_col0,
                                                        double* __restrict__ O, long ldo, long o_col0, int C) {
  constexpr int XP = 16 * CT + 1;
  __shared__ double Xs[128 * XP];
  typedef double rk_v4d __attribute__((ext_vector_type(4)));
  const MMJob job = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const double* const bb = B + (long)job.b_row * ldb + b_col0;
  const int ct = (C + 15) >> 4;                   // column tiles that hold anything (uniform)
  hodlr_stage_rows(Xs, XP, bb, ldb, job.kd, C, ct);
  // this wavefront's eight k steps of the A operand: V^T(fr, 4 kk + fk) = V(row, fr)
  double a[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = 4 * (8 * wave + q) + fk;
    a[q] = (fr < R && row < job.kd) ? A[job.a_off + (long)row * R + fr] : 0.0;
  }
  __syncthreads();
  rk_v4d acc[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc[j] = (rk_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const double* const bp = Xs + (4 * (8 * wave + q) + fk) * XP + fr;
#pragma unroll
    for (int j = 0; j < CT; ++j)
      if (j < ct) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], bp[16 * j], acc[j], 0, 0, 0);
  }
  __syncthreads();                                // (Xs is free: the partial tiles of wavefronts 1-3 go there)
  double* const part = Xs;                        // [3][CT][4][64]
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(((wave - 1) * CT + j) * 4 + r) * 64 + lane] = acc[j][r];
  }
  __syncthreads();
  if (wave == 0) {
    // f64 MFMA C/D map: row = (lane >> 4) + 4 reg, col = lane & 15
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = fk + 4 * r, c = 16 * j + fr;
        if (k < R && c < C) {
          const double v = ((acc[j][r] + part[((0 * CT + j) * 4 + r) * 64 + lane]) + part[((1 * CT + j) * 4 + r) * 64 + lane]) +
                           part[((2 * CT + j) * 4 + r) * 64 + lane];
          O[(long)(job.o_row + k) * ldo + o_col0 + c] = v;
        }
      }
  }
}
// The rank-R updates of the factorisation sweep, U[rows of a chunk, 0:C] -= U_l[rows, 0:R] * T[b_row : b_row+R, 0:C]
// (R <= 16, <= 128 rows, C <= 16 CT), one workgroup per chunk without any LDS: the accumulators start from the
// O tiles themselves (each lane's four rows x one column of a 16 x 16 tile, 128-byte row segments), K = R is
// padded to 16 only (the tile kernel pads to 32 and stages both operands), operands straight from HBM / L2.
//   O[(o_row + r) * ldo + c] -= sum_k A[a_off + r * a_rs + k] * B[(b_row + k) * ldb + c]
template <int CT>
__global__ __launch_bounds__(256) void hodlr_upd_kernel(const MMJob* __restrict__ jobs, const double* __restrict__ A, long a_rs,
                                                        const double* __restrict__ B, long ldb, double* __restrict__ O, long ldo, int C) {
  typedef double uk_v4d __attribute__((ext_vector_type(4)));
  const MMJob job = jobs[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int R = job.kd, nkk = (R + 3) >> 2, ct = (C + 15) >> 4;        // (uniform)
  double a[2][4], b[4][CT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int row = 32 * wave + 16 * i + fr, k = 4 * kk + fk;
      a[i][kk] = (row < job.m && k < R) ? -A[job.a_off + (long)row * a_rs + k] : 0.0;
    }
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int k = 4 * kk + fk, c = 16 * j + fr;
      b[kk][j] = (k < R && c < C) ? B[(long)(job.b_row + k) * ldb + c] : 0.0;
    }
  double* const ob = O + (long)job.o_row * ldo;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    if (32 * wave + 16 * i >= job.m) continue;                         // (uniform)
    uk_v4d acc[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * wave + 16 * i + fk + 4 * r, c = 16 * j + fr;
        acc[j][r] = (j < ct && row < job.m && c < C) ? ob[(long)row * ldo + c] : 0.0;
      }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk >= nkk) continue;
#pragma unroll
      for (int j = 0; j < CT; ++j)
        if (j < ct) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i][kk], b[kk][j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * wave + 16 * i + fk + 4 * r, c = 16 * j + fr;
        if (j < ct && row < job.m && c < C) ob[(long)row * ldo + c] = acc[j][r];
      }
  }
}
// hodlr_upd_kernel for level l and hodlr_red_kernel for the next shallower level l' in ONE pass over a chunk's rows of U
// (round 5).  The reduce of l' reads columns [0, off_l' + R_l') = [0, off_l) of U -- exactly what the update of l has just
// written: here the updated tiles go to HBM and into the LDS image the reduce multiplies from, and the sweep reads U once
// per level instead of twice (C4: upd<4> 52 us + red<4> 66 us per level, both HBM-bound).  The update's arithmetic is
// hodlr_upd_kernel's, the reduce multiplies the same doubles hodlr_red_kernel would have staged from HBM, in the same order:
// bit-identical to the two launches.  Needs the two levels' chunks to be the same rows (HLevel::chunk_geom).
template <int CT>
__global__ __launch_bounds__(256) void hodlr_updred_kernel(const MMJob* __restrict__ ujobs, const double* __restrict__ A, long a_rs,
                                                           const double* __restrict__ B, long ldb, double* __restrict__ O, long ldo, int C,
                                                           const MMJob* __restrict__ rjobs, const double* __restrict__ V2, int R2,
                                                           double* __restrict__ P, long ldp) {
  __shared__ double part[3 * CT * 4 * 64];
  typedef double uk_v4d __attribute__((ext_vector_type(4)));
  const MMJob job = ujobs[blockIdx.x];
  const MMJob rj = rjobs[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int R = job.kd, nkk = (R + 3) >> 2;                             // (uniform; every one of the CT column tiles is computed:
  // columns >= C are zero on both sides, and a `tile j < ceil(C / 16)` test in front of each matrix instruction made hipcc keep
  // both versions of every accumulator -- 256 VGPRs at CT = 4)
  // the reduce's A operand (V_l'^T: this wavefront's eight k steps, q = 4 i + r <-> rows 32 wave + 16 i + 4 r + fk), requested
  // first: it lands under the update
  double a2[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int row = 4 * (8 * wave + q) + fk;
    a2[q] = (fr < R2 && row < rj.kd) ? V2[rj.a_off + (long)row * R2 + fr] : 0.0;
  }
  double b[4][CT];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int j = 0; j < CT; ++j) {
      const int k = 4 * kk + fk, c = 16 * j + fr;
      b[kk][j] = (k < R && c < C) ? B[(long)(job.b_row + k) * ldb + c] : 0.0;
    }
  double* const ob = O + (long)job.o_row * ldo;
  uk_v4d acc2[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) acc2[j] = (uk_v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uk_v4d acc[CT];
    const bool live = 32 * wave + 16 * i < job.m;                      // (uniform)
    // (one 16-row tile at a time, fenced: with both tiles' loads hoisted to the top hipcc needs 256 VGPRs at CT = 4 -- two
    //  wavefronts per SIMD for a kernel that lives on memory latency, 127-136 us per level against 52 + 66 for the two launches)
    double a[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int row = 32 * wave + 16 * i + fr, k = 4 * kk + fk;
      a[kk] = (row < job.m && k < R) ? -A[job.a_off + (long)row * a_rs + k] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * wave + 16 * i + fk + 4 * r, c = 16 * j + fr;
        acc[j][r] = (live && row < job.m && c < C) ? ob[(long)row * ldo + c] : 0.0;
      }
    if (live) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        if (kk >= nkk) continue;
#pragma unroll
        for (int j = 0; j < CT; ++j)
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b[kk][j], acc[j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 32 * wave + 16 * i + fk + 4 * r, c = 16 * j + fr;
          if (row < job.m && c < C) ob[(long)row * ldo + c] = acc[j][r];
        }
    }
    // The reduce, straight from the registers: the update's result layout (lane (fr, fk), register r of tile j = row 4 r + fk,
    // column 16 j + fr of this 16-row tile) IS the matrix instruction's B operand layout for the k-step over rows 4 r .. 4 r + 3
    // (B[k = fk][n = fr]) -- hodlr_red_kernel stages exactly these values through LDS and reads them back into this position.
    // Same k-steps in the same order (q = 4 i + r) on the same wavefront: the same bits.
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < CT; ++j)
        acc2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[4 * i + r], acc[j][r], acc2[j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[(((wave - 1) * CT + j) * 4 + r) * 64 + lane] = acc2[j][r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = fk + 4 * r, c = 16 * j + fr;
        if (k < R2 && c < C) {
          const double v = ((acc2[j][r] + part[((0 * CT + j) * 4 + r) * 64 + lane]) + part[((1 * CT + j) * 4 + r) * 64 + lane]) +
                           part[((2 * CT + j) * 4 + r) * 64 + lane];
          P[(long)(rj.o_row + k) * ldp + c] = v;
        }
      }
  }
}
// The instantiation of a <CT> kernel for C <= 128 columns: CT = the 16-column tiles, 1 .. 5, else 8.  LAUNCH(CT) is the caller's.
#define GH_CT_DISPATCH(C, LAUNCH)   \
  switch (((C) + 15) / 16) {        \
    case 1: LAUNCH(1); break;       \
    case 2: LAUNCH(2); break;       \
    case 3: LAUNCH(3); break;       \
    case 4: LAUNCH(4); break;       \
    case 5: LAUNCH(5); break;       \
    default: LAUNCH(8); break;      \
  }
int hodlr_launch_red(gh_hodlr* h, const MMJob* jobs, int njobs, int R, const double* V, const double* B, long ldb, long b_col0,
                     double* O, long ldo, long o_col0, int C) {
  if (njobs <= 0 || C <= 0 || R <= 0) return GH_OK;
  if (R > 16 || C > 128) return hodlr_launch_mm(h, h->st, jobs, njobs, R, V, 1, R, B, ldb, b_col0, O, ldo, o_col0, C, false, 1);
  // (one instantiation per number of 16-column tiles: the LDS image is 128 x (16 CT + 1) doubles, and with 17-50 KB
  //  instead of 83 several workgroups share a CU at the shallow levels, whose U has few columns yet)
#define GH_RED_LAUNCH(CT) hipLaunchKernelGGL(hodlr_red_kernel<CT>, dim3(njobs), dim3(256), 0, h->st, jobs, V, R, B, ldb, b_col0, O, ldo, o_col0, C)
  GH_CT_DISPATCH(C, GH_RED_LAUNCH)
#undef GH_RED_LAUNCH
  GH_HIP(hipGetLastError());
  return GH_OK;
}

int hodlr_launch_upd(gh_hodlr* h, const MMJob* jobs, int njobs, int R, const double* A, long a_rs, const double* B, long ldb,
                     double* O, long ldo, int C) {
  if (njobs <= 0 || C <= 0 || R <= 0) return GH_OK;
  if (R > 16 || C > 128 || HCH > 128) return hodlr_launch_mm(h, h->st, jobs, njobs, HCH, A, a_rs, 1, B, ldb, 0, O, ldo, 0, C, true, HCH / 32);
#define GH_UPD_LAUNCH(CT) hipLaunchKernelGGL(hodlr_upd_kernel<CT>, dim3(njobs), dim3(256), 0, h->st, jobs, A, a_rs, B, ldb, O, ldo, C)
  GH_CT_DISPATCH(C, GH_UPD_LAUNCH)
#undef GH_UPD_LAUNCH
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// update of level `L` (columns [0, C) of U, C = L->off) + reduce of level `nx` over the same columns in one pass; false when
// the pair cannot share a pass (the caller then launches the two kernels)
bool hodlr_updred_possible(int passes, const HLevel* L, const HLevel* nx, int C, int cpass) {
  return (passes & 2) && nx && !nx->top && !L->top && L->R <= 16 && nx->R <= 16 && C > 0 && C <= 128 && HCH == 128 &&
         nx->off + nx->R == C && C <= cpass && nx->chunk_geom == L->chunk_geom && !L->chunk_geom.empty();
}
int hodlr_launch_updred(gh_hodlr* h, const HLevel* L, const HLevel* nx, const double* A, long a_rs, const double* B, long ldb,
                        double* O, long ldo, int C, const double* V2, double* P, long ldp) {
  const MMJob* uj = (const MMJob*)L->d_upd_jobs.p;
  const MMJob* rj = (const MMJob*)nx->d_red_jobs.p;
#define GH_UR_LAUNCH(CT) hipLaunchKernelGGL(hodlr_updred_kernel<CT>, dim3(L->nchunks), dim3(256), 0, h->st, uj, A, a_rs, B, ldb, O, ldo, C, rj, V2, nx->R, P, ldp)
  GH_CT_DISPATCH(C, GH_UR_LAUNCH)
#undef GH_UR_LAUNCH
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// mtiles: 32-row tiles of a job handled by ONE workgroup (the update passes: 4, i.e. a whole 128-row
// chunk -- 8192 workgroups of one tiny tile each spent their 50 us on being dispatched)
int hodlr_launch_mm(gh_hodlr* h, hipStream_t st, const MMJob* jobs, int njobs, int max_m, const double* A, long a_rs, long a_cs,
                    const double* B, long ldb, long b_col0, double* O, long ldo, long o_col0, int C, bool subtract, int mtiles) {
  if (njobs <= 0 || C <= 0 || max_m <= 0) return GH_OK;
  MMArgs a;
  a.mtiles = mtiles;
  a.jobs = jobs; a.A = A; a.a_rs = a_rs; a.a_cs = a_cs; a.B = B; a.ldb = ldb; a.b_col0 = b_col0;
  a.O = O; a.ldo = ldo; a.o_col0 = o_col0; a.C = C; a.subtract = subtract ? 1 : 0;
  hipLaunchKernelGGL(hodlr_mm_kernel, dim3(njobs, ((max_m + 31) / 32 + mtiles - 1) / mtiles, (C + 63) / 64), dim3(256), 0, st, a);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

int hodlr_launch_sum(gh_hodlr* h, const HLevel* L, int C) {
  hipLaunchKernelGGL(hodlr_sum_kernel, dim3((unsigned)L->node_ids.size(), 2 * L->R), dim3(64 * SUM_NS), 0, h->st, h->P.d(), (const int*)L->d_crange.p, L->R,
                     (long)h->cpass, C, h->Tsum.d());
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int hodlr_launch_sbuild(const double* Tsum, long Cp, int R, double* S, int nb, hipStream_t st) {
  hipLaunchKernelGGL(hodlr_sbuild_kernel, dim3(nb), dim3(256), 0, st, Tsum, Cp, R, S);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int hodlr_launch_eye_strip(double* p, long ld, long col0, int cw, hipStream_t st) {
  hipLaunchKernelGGL(hodlr_eye_strip_kernel, dim3((unsigned)((cw + 255) / 256)), dim3(256), 0, st, p, ld, col0, cw);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// level-major copy UL of the final U (every level's columns contiguous: what the wide solves' tile kernel wants), made on demand
static int ensure_ul(gh_hodlr* h) {
  if (h->ul_valid || h->Rtot <= 0) return GH_OK;
  const long n = h->n, Rtot = h->Rtot;
  hipStream_t st = h->st;
  GH_CHECK(h->UL.ensure((size_t)n * Rtot * sizeof(double)));
  std::vector<long> colbase(Rtot);
  std::vector<int> colld(Rtot);
  for (auto* L : h->levels)
    for (int kk = 0; kk < L->R; ++kk) { colbase[L->off + kk] = (long)n * L->off + kk; colld[L->off + kk] = L->R; }
  // (cached like the job tables: same ranks, same map)
  bool same = h->col_Rtot == Rtot && h->col_sig.size() == h->levels.size();
  for (size_t q = 0; same && q < h->levels.size(); ++q) same = h->col_sig[q] == h->levels[q]->R;
  if (!same) {
    GH_CHECK(upload(h->d_colbase, colbase, st));
    GH_CHECK(upload(h->d_colld, colld, st));
    h->col_Rtot = Rtot;
    h->col_sig.clear();
    for (auto* L : h->levels) h->col_sig.push_back(L->R);
  }
  hipLaunchKernelGGL(hodlr_relayout_kernel, dim3(2048), dim3(256), 0, st, h->UA.d(), (long)n, (int)Rtot,
                     (const long*)h->d_colbase.p, (const int*)h->d_colld.p, h->UL.d());
  GH_HIP(hipGetLastError());
  h->ul_valid = true;
  return GH_OK;
}
// X[:, xcol0 : xcol0+C] <- (level lv)^-1 applied (hodlr.h:244-253 for every node of the level)
// (U == nullptr: the level-major copy UL is used -- solves; else the row-major UA with pitch ldu)
int hodlr_apply_level(gh_hodlr* h, HLevel* L, double* X, long ldx, long xcol0, int C, const double* U, long ldu) {
  if (L->R == 0 || C <= 0) return GH_OK;
  if (!U) GH_CHECK(ensure_ul(h));
  const int R = L->R, nn = (int)L->node_ids.size();
  const double* Vl = h->VA.d() + (long)h->n * L->off;
  if (C <= MV_C && R <= 32) {
    const long Cp = h->cpass;
    const double* Ub = U ? U + L->off : h->UL.d() + (long)h->n * L->off;
    const long u_rs = U ? ldu : R;
    const MMJob* uj = (const MMJob*)(U ? L->d_upd_jobs.p : L->d_updl_jobs.p);
    hipLaunchKernelGGL(hodlr_mv_reduce_kernel, dim3(L->nchunks), dim3(256), 0, h->st, (const MMJob*)L->d_red_jobs.p, Vl, R, X, ldx, xcol0,
                       h->P.d(), Cp, C);
    hipLaunchKernelGGL(hodlr_sum_narrow_kernel, dim3(nn, 2 * R), dim3(256), 0, h->st, h->P.d(), (const int*)L->d_crange.p, R, Cp, C, h->Tsum.d());
    GH_HIP(hipGetLastError());
    if (L->top) GH_CHECK(h->sub.allreduce(h->sub.ctx, L->top_level, h->Tsum.d(), 2 * R, C, Cp, h->st));
    GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_smul_jobs.p, nn, 2 * R, L->sinv.d(), 2 * R, 1,
                       h->Tsum.d(), Cp, 0, h->Tout.d(), Cp, 0, C, false));
    hipLaunchKernelGGL(hodlr_mv_update_kernel, dim3(L->nchunks), dim3(128), 0, h->st, uj, Ub, u_rs, h->Tout.d(), Cp, X, ldx, xcol0, C);
    GH_HIP(hipGetLastError());
    return GH_OK;
  }
  // (a pseudo-level goes in passes of CPASS columns whatever this handle's own pass width: the devices below the
  //  ancestor must agree on the number and the shape of the sums they complete together)
  const int pw = L->top ? CPASS : h->cpass;
  for (int cp = 0; cp < C; cp += pw) {
    const int cw = std::min(pw, C - cp);
    const long Cp = h->cpass;
    // reduce: P[chunk] = V_chunk^T X_chunk
    GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_red_jobs.p, L->nchunks, R, Vl, 1, R,
                       X, ldx, xcol0 + cp, h->P.d(), Cp, 0, cw, false));
    GH_CHECK(hodlr_launch_sum(h, L, cw));
    if (L->top) GH_CHECK(h->sub.allreduce(h->sub.ctx, L->top_level, h->Tsum.d(), 2 * R, cw, Cp, h->st));
    // core: Tout = S^-1 Tsum
    GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_smul_jobs.p, nn, 2 * R, L->sinv.d(), 2 * R, 1,
                       h->Tsum.d(), Cp, 0, h->Tout.d(), Cp, 0, cw, false));
    // update: X_chunk -= U_chunk * Tout[half]
    if (U)
      GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_upd_jobs.p, L->nchunks, HCH, U + L->off, ldu, 1,
                         h->Tout.d(), Cp, 0, X, ldx, xcol0 + cp, cw, true, HCH / 32));
    else
      GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_updl_jobs.p, L->nchunks, HCH, h->UL.d() + (long)h->n * L->off, R, 1,
                         h->Tout.d(), Cp, 0, X, ldx, xcol0 + cp, cw, true, HCH / 32));
  }
  return GH_OK;
}
// X rows of every leaf <- K_leaf^-1 X
// red / red_done: the sweep's first call -- form the chunk products of level `red` over the same columns in the same pass when
// its chunks are the leaves (then *red_done = true and the caller skips that level's reduce)
int hodlr_apply_leaves(gh_hodlr* h, int passes, double* X, long ldx, long xcol0, int C, const HLevel* red, bool* red_done, const LeafSrc* src) {
  const LeafSrc ls = src ? *src : LeafSrc();         // (src: only on the 128-row-leaf path with ONE column pass -- leaf_src_possible())
  if (red_done) *red_done = false;
  if (C <= 0) return GH_OK;
  if (C <= MV_C && h->max_leaf <= 256) {
    hipLaunchKernelGGL(hodlr_mv_leaf_kernel, dim3((unsigned)h->leaves.size()), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p,
                       h->leaf_inv.d(), (long)h->leaf_pitch, X, ldx, xcol0, C);
    GH_HIP(hipGetLastError());
    return GH_OK;
  }
  if (h->leaf_pitch == 128 && h->max_leaf <= 128) {
    // one workgroup per leaf, in place; column passes of <= 128 (80 where that covers the rest: less LDS, fewer MFMAs)
    bool fuse = (passes & 2) && red && red_done && C <= 128 && xcol0 == 0 && red->R > 0 && red->R <= 16 && !red->top &&
                red->off + red->R == C && C <= h->cpass && red->chunk_geom.size() == 2 * h->leaves.size();
    for (size_t q = 0; fuse && q < h->leaves.size(); ++q)
      fuse = red->chunk_geom[2 * q] == h->leaves[q].start && red->chunk_geom[2 * q + 1] == h->leaves[q].size;
    if (fuse) {
      const unsigned nl = (unsigned)h->leaves.size();
      const MMJob* rj = (const MMJob*)red->d_red_jobs.p;
      const double* V2 = h->VA.d() + (long)h->n * red->off;
      if (C <= 80) hipLaunchKernelGGL(hodlr_leaf_apply_kernel<5>, dim3(nl), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p, h->leaf_inv.d(), X, ldx, xcol0, C,
                                      rj, V2, red->R, h->P.d(), (long)h->cpass, ls);
      else hipLaunchKernelGGL(hodlr_leaf_apply_kernel<8>, dim3(nl), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p, h->leaf_inv.d(), X, ldx, xcol0, C,
                              rj, V2, red->R, h->P.d(), (long)h->cpass, ls);
      GH_HIP(hipGetLastError());
      *red_done = true;
      return GH_OK;
    }
    for (int cp = 0; cp < C;) {
      const int cw = std::min(128, C - cp);
      const unsigned nl = (unsigned)h->leaves.size();
      if (cw <= 80) hipLaunchKernelGGL(hodlr_leaf_apply_kernel<5>, dim3(nl), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p, h->leaf_inv.d(), X, ldx, xcol0 + cp, cw,
                                       (const MMJob*)nullptr, (const double*)nullptr, 0, (double*)nullptr, 0L, ls);
      else hipLaunchKernelGGL(hodlr_leaf_apply_kernel<8>, dim3(nl), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p, h->leaf_inv.d(), X, ldx, xcol0 + cp, cw,
                              (const MMJob*)nullptr, (const double*)nullptr, 0, (double*)nullptr, 0L, ls);
      GH_HIP(hipGetLastError());
      cp += cw;
    }
    return GH_OK;
  }
  for (int cp = 0; cp < C; cp += h->cpass) {
    const int cw = std::min(h->cpass, C - cp);
    GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)h->d_leaf_jobs.p, (int)h->leaves.size(), h->max_leaf, h->leaf_inv.d(), h->leaf_pitch, 1,
                       X, ldx, xcol0 + cp, h->Y.d(), h->cpass, 0, cw, false));
    const long tot = h->n * cw;
    hipLaunchKernelGGL(hodlr_copyrows_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 65535)), dim3(256), 0, h->st,
                       h->Y.d(), (long)h->cpass, X, ldx, xcol0 + cp, (long)h->n, cw);
    GH_HIP(hipGetLastError());
  }
  return GH_OK;
}
// full solve on X (n x C): leaves, then levels bottom-up (hodlr.h:107-114)
// gh_debug_set_hodlr_passes (A/B in one process, tests): bit 0 = the narrow solve in shared passes (round 5), bit 1 = the
// factorisation sweep's update of level l and reduce of the next level in one pass over U; default: both
static std::atomic<int> g_hodlr_passes{3};
extern "C" int gh_debug_set_hodlr_passes(int mask) {
  return g_hodlr_passes.exchange(mask < 0 ? 3 : (mask & 3));
}
int hodlr_passes() { return g_hodlr_passes; }
// the narrow solve: leaves (symmetric form), then per level "sum + core product" and ONE pass over the rows that applies this
// level's update and forms the next level's chunk products (separate passes where the two levels' chunks differ)
static int solve_narrow(gh_hodlr* h, double* X, long ldx, int C) {
  hipLaunchKernelGGL(hodlr_mv_leaf_sym_kernel, dim3((unsigned)h->leaves.size()), dim3(256), 0, h->st, (const MMJob*)h->d_leaf_jobs.p,
                     h->leaf_inv.d(), (long)h->leaf_pitch, X, ldx, 0L, C);
  std::vector<HLevel*> Ls;
  for (int l = (int)h->levels.size() - 1; l >= 0; --l) if (h->levels[l]->R > 0) Ls.push_back(h->levels[l]);
  const long Cp = h->cpass;
  auto pass = [&](HLevel* up, HLevel* red) {
    HLevel* g = up ? up : red;
    const size_t lds = up ? (size_t)128 * (up->R <= 16 ? 17 : 33) * sizeof(double) : 0;
    hipLaunchKernelGGL(hodlr_mv_updred_kernel, dim3(g->nchunks), dim3(256), lds, h->st,
                       up ? (const MMJob*)up->d_upd_jobs.p : (const MMJob*)nullptr, up ? h->UA.d() + up->off : (const double*)nullptr,
                       (long)h->Rtot, (const double*)h->Tout.d(),
                       red ? (const MMJob*)red->d_red_jobs.p : (const MMJob*)nullptr, red ? h->VA.d() + (long)h->n * red->off : (const double*)nullptr,
                       red ? red->R : 0, h->P.d(), Cp, X, ldx, 0L, C);
  };
  if (!Ls.empty()) pass(nullptr, Ls[0]);
  for (size_t i = 0; i < Ls.size(); ++i) {
    HLevel* L = Ls[i];
    // (one workgroup per node adds the partials of ALL 2R rows: fine while a half has <= 64 chunks -- the deep levels, many nodes;
    //  the few nodes of the top levels have up to N / 256 chunks per half and keep one workgroup per (node, row) + the product)
    const int nn = (int)L->node_ids.size();
    if ((long)L->nchunks <= 128L * nn) {
      hipLaunchKernelGGL(hodlr_mv_summm_kernel, dim3((unsigned)nn), dim3(256), 0, h->st, h->P.d(), (const int*)L->d_crange.p, L->R, Cp, C,
                         (const double*)L->sinv.d(), h->Tout.d());
    } else {
      hipLaunchKernelGGL(hodlr_sum_narrow_kernel, dim3(nn, 2 * L->R), dim3(256), 0, h->st, h->P.d(), (const int*)L->d_crange.p, L->R, Cp, C, h->Tsum.d());
      GH_CHECK(hodlr_launch_mm(h, h->st, (const MMJob*)L->d_smul_jobs.p, nn, 2 * L->R, L->sinv.d(), 2 * L->R, 1, h->Tsum.d(), Cp, 0, h->Tout.d(), Cp, 0, C, false));
    }
    HLevel* nx = i + 1 < Ls.size() ? Ls[i + 1] : nullptr;
    if (nx && nx->chunk_geom == L->chunk_geom) pass(L, nx);
    else { pass(L, nullptr); if (nx) pass(nullptr, nx); }
  }
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int hodlr_solve_all(gh_hodlr* h, int passes, double* X, long ldx, int C) {
  if ((passes & 1) && C <= MV_C && h->max_leaf <= 256 && h->sub.depth == 0) {
    bool ok = true;
    for (auto* L : h->levels) ok = ok && !L->top && L->R <= 32 && (L->R == 0 || !L->chunk_geom.empty());
    if (ok) return solve_narrow(h, X, ldx, C);
  }
  GH_CHECK(hodlr_apply_leaves(h, passes, X, ldx, 0, C));
  for (int l = (int)h->levels.size() - 1; l >= 0; --l)
    GH_CHECK(hodlr_apply_level(h, h->levels[l], X, ldx, 0, C, nullptr, 0));
  return GH_OK;
}

int hodlr_need(gh_hodlr* h) {
  if (!h) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!h->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  GH_HIP(hipSetDevice(h->opts.device));
  return GH_OK;
}

extern "C" int gh_hodlr_solve(gh_hodlr* h, const double* b, int64_t nrhs, double* out) {
  GH_CHECK(hodlr_need(h));
  if (!b || !out || nrhs <= 0) { gh_set_error("bad argument to solve"); return GH_ERR_BAD_ARG; }
  const size_t tot = (size_t)h->n * nrhs;
  GH_CHECK(h->rhs.ensure(tot * sizeof(double)));
  GH_CHECK(gh_to_device(h->rhs.d(), b, tot, h->st));
  GH_CHECK(hodlr_solve_all(h, g_hodlr_passes, h->rhs.d(), nrhs, (int)nrhs));
  GH_CHECK(gh_from_device(out, h->rhs.d(), tot, h->st));
  GH_HIP(hipStreamSynchronize(h->st));                    // (a device `out` is only enqueued by gh_from_device)
  return GH_OK;
}
extern "C" int gh_hodlr_dot_solve(gh_hodlr* h, const double* y, double* out) {
  GH_CHECK(hodlr_need(h));
  if (!y || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  GH_CHECK(h->rhs.ensure((size_t)h->n * sizeof(double)));
  GH_CHECK(h->work.ensure((size_t)h->n * sizeof(double)));
  GH_CHECK(gh_to_device(h->rhs.d(), y, (size_t)h->n, h->st));
  const double* yd = y;                              // (a device-resident y is read where it is)
  if (!gh_is_device_ptr(y)) { GH_CHECK(gh_to_device(h->work.d(), y, (size_t)h->n, h->st)); yd = h->work.d(); }
  GH_CHECK(hodlr_solve_all(h, g_hodlr_passes, h->rhs.d(), 1, 1));
  GH_CHECK(h->dotp.ensure(256 * sizeof(double)));
  hipLaunchKernelGGL(hodlr_dot_kernel, dim3(256), dim3(256), 0, h->st, yd, h->rhs.d(), (long)h->n, h->dotp.d());
  hipLaunchKernelGGL(hodlr_dot_kernel, dim3(1), dim3(256), 0, h->st, h->dotp.d(), (const double*)nullptr, 256L, h->scal.d());
  GH_HIP(hipGetLastError());
  double v = 0.0;
  GH_HIP(hipMemcpyAsync(&v, h->scal.d(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  *out = v;
  return GH_OK;
}
extern "C" int gh_hodlr_get_inverse(gh_hodlr* h, double* out) {
  GH_CHECK(hodlr_need(h));
  if (!out) { gh_set_error("null output"); return GH_ERR_BAD_ARG; }
  const long n = h->n;
  GH_CHECK(h->rhs.ensure((size_t)n * n * sizeof(double)));
  GH_HIP(hipMemsetAsync(h->rhs.p, 0, (size_t)n * n * sizeof(double), h->st));
  GH_CHECK(hodlr_launch_eye_strip(h->rhs.d(), n, 0, (int)n, h->st));
  GH_CHECK(hodlr_solve_all(h, g_hodlr_passes, h->rhs.d(), n, (int)n));
  GH_CHECK(gh_from_device(out, h->rhs.d(), (size_t)n * n, h->st));
  GH_HIP(hipStreamSynchronize(h->st));                    // (a device `out` is only enqueued by gh_from_device)
  return GH_OK;
}
