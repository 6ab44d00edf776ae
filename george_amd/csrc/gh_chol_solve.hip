// gh_chol_solve.hip -- the dense solver, work on a COMPUTED factor (gh_chol.hip makes it, gh_chol_update.hip moves and edits it).
//
// Solves are blocked substitutions that multiply by the stored 128x128 diagonal inverses: TRSV kernels for one right-hand side
// (one chained launch per sweep), the MFMA GEMM for many.  On top of them: dot_solve, solve, apply_sqrt, get_inverse, predict,
// predict_grad, sample_conditional, grad, fisher, objective, loo, loo_objective, lgo.  The reductions live here too (the log-det's
// launcher is what the other two units call).
#include <math.h>
#include "gh_chol_impl.h"
#include "gh_device_util.h"
#include "gh_spin.h"

// ================================================================= reductions  (wave_sum, block_sum_256: gh_device_util.h)

// out[0] (+)= 2 * sum_i log(A[i][i])   (basic.py:69); one workgroup, fixed order
__global__ __launch_bounds__(256) void logdet_kernel(const double* A, long lda, long n, double* out, int accumulate) {
  __shared__ double sh[4];
  double v = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) v += log(A[i * lda + i]);
  v = block_sum_256(v, sh);
  if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.0) + 2.0 * v;
}
// out[0] = sum_i a[i] * b[i]
// (fail != nullptr: the chained solve's time-out flag travels with the result, out[2] = flag: one copy back instead of two)
__global__ __launch_bounds__(256) void dot_kernel(const double* a, const double* b, long n, double* out, const int* fail) {
  __shared__ double sh[4];
  double v = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) v += a[i] * b[i];
  v = block_sum_256(v, sh);
  if (threadIdx.x == 0) { out[0] = v; if (fail) out[2] = (double)*fail; }
}

// Two-stage versions for long vectors: `part[g]` = the g-th contiguous slice, then one workgroup adds
// the slices in index order (fixed order: bitwise reproducible).  One workgroup walking 65536
// diagonal entries, each in its own cache line, took 195 us; the dot product 97 us.
__global__ __launch_bounds__(256) void logdet_part_kernel(const double* A, long lda, long n, double* part) {
  __shared__ double sh[4];
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double v = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) v += log(A[i * lda + i]);
  v = block_sum_256(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
__global__ __launch_bounds__(256) void dot_part_kernel(const double* a, const double* b, long n, double* part) {
  __shared__ double sh[4];
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double v = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) v += a[i] * b[i];
  v = block_sum_256(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
// out[0] (+)= scale * sum_{g < m} part[g], m <= 64, added in index order by one lane
__global__ void reduce_final_kernel(const double* part, int m, double scale, double* out, int accumulate, const int* fail) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v = 0.0;
  for (int g = 0; g < m; ++g) v += part[g];
  out[0] = (accumulate ? out[0] : 0.0) + scale * v;
  if (fail) out[2] = (double)*fail;
}
#define RED_SLICES 64
int gh_launch_logdet(const double* A, long lda, long n, double* out, double* part, hipStream_t st) {
  const int g = (int)std::min<long>(RED_SLICES, (n + 2047) / 2048);
  if (g <= 1) {
    hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(256), 0, st, A, lda, n, out, 0);
  } else {
    hipLaunchKernelGGL(logdet_part_kernel, dim3(g), dim3(256), 0, st, A, lda, n, part);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(64), 0, st, part, g, 2.0, out, 0, (const int*)nullptr);
  }
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_logdet_accum(const double* A, long lda, long n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(logdet_kernel, dim3(1), dim3(256), 0, st, A, lda, n, out, 1);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
static int launch_dot(const double* a, const double* b, long n, double* out, double* part, hipStream_t st, const int* fail = nullptr) {
  const int g = (int)std::min<long>(RED_SLICES, (n + 4095) / 4096);
  if (g <= 1) {
    hipLaunchKernelGGL(dot_kernel, dim3(1), dim3(256), 0, st, a, b, n, out, fail);
  } else {
    hipLaunchKernelGGL(dot_part_kernel, dim3(g), dim3(256), 0, st, a, b, n, part);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(64), 0, st, part, g, 1.0, out, 0, fail);
  }
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// ======================================================== single-RHS solves
// Forward step j of L z = y (right-looking).  Every workgroup recomputes
// z_j = L_jj^-1 w_j from the current working vector w (128x128 mat-vec from L2), workgroup 0
// publishes it into z, workgroups b >= 1 update their 128 rows: w[i] -= L[i, jblock] . z_j.
__global__ __launch_bounds__(256) void trsv_fwd_step(const double* L, long ld, const double* dinv_j,
                                                     long j0, double* w, double* z) {
  __shared__ double zj[T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double2 wv = *reinterpret_cast<const double2*>(w + j0 + 2 * lane);
  // 8 rows per trip: all eight 1-KiB row loads are in flight before the first reduction
  // (one load per trip left this kernel latency-bound: 52 us per step at N = 16384)
  for (int r0 = wave * 8; r0 < T; r0 += 32) {
    double2 a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = *reinterpret_cast<const double2*>(dinv_j + (r0 + q) * T + 2 * lane);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = wave_sum(a[q].x * wv.x + a[q].y * wv.y);
      if (lane == 0) zj[r0 + q] = v;
    }
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid < T) z[j0 + tid] = zj[tid];
    return;
  }
  const long row0 = j0 + (long)blockIdx.x * T;
  const double zx = zj[2 * lane], zy = zj[2 * lane + 1];
  for (int r0 = wave * 8; r0 < T; r0 += 32) {
    double2 a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = *reinterpret_cast<const double2*>(L + (row0 + r0 + q) * ld + j0 + 2 * lane);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const double v = wave_sum(a[q].x * zx + a[q].y * zy);
      if (lane == 0) w[row0 + r0 + q] -= v;
    }
  }
}
// The whole forward sweep L z = y as ONE launch: workgroup b owns block row b.  It walks the blocks
// L[b, 0..b-1] left to right, folding each z_j into per-lane partial sums as soon as workgroup j
// has published it, then solves its own diagonal block with the stored inverse and publishes z_b.
// The step-per-launch version above costs a launch gap plus two dependent 128x128 mat-vecs per block
// row (25-27 us, 14.3 ms at N = 65536 against 2.2 ms of HBM time for the triangle); here a link of the
// chain is  z_j seen -> 128 FMAs per lane -> reduce -> one mat-vec -> store,  and the L blocks of a
// row stream in ahead of the wait (the next block is loaded into registers before it).  512 threads:
// wavefront w takes rows 16w..16w+15, a lane two columns.  Deadlock freedom: workgroup b only waits
// for workgroups j < b, and a 1-D grid is dispatched in blockIdx order, so whatever it waits for is
// resident or finished (the grid need not fit the chip).  A wait that outlasts ~2 s raises *fail
// instead of hanging.
//
// z ITSELF IS THE MESSAGE (round 3; the flag-per-block-row predecessor, 10.7 us per link, is
// scripts/dev/arms/trsv_chain_flags.hip.inc).  z is pre-filled with a sentinel (all bits set: a NaN no
// arithmetic produces), workgroup j publishes its 128 values as agent-scope atomic stores (write-through
// past its XCD's L2; no fences: a release/acquire pair costs an L2 write-back on one side and an
// invalidate on the other at every link -- chain neighbours sit on different XCDs -- 16-29 us measured),
// and a consumer's first wavefront polls those 128 values directly -- lane l its two -- until none is
// the sentinel, then hands them to the other wavefronts through LDS.  Against the flag version a link
// loses one L2 round trip (flag seen -> THEN z fetched), the producer's s_waitcnt + barrier + flag
// store, the sixteen one-lane stores of a wavefront (now one 128-byte store from lanes 0-15) and 5/6 of
// its cross-lane traffic: the 16 row sums of a wavefront are formed by a transposing butterfly (8 + 4 +
// 2 + 1 exchanges inside a row of 16 lanes, then 2 across rows: 17 instead of 96), which leaves row q's
// total in lane q; y is fetched before the loop (it was a dependent load on the critical path).
// Measured: 3.4 us per link; the solve part of compute()+log_likelihood() 0.68 -> 0.22 ms at N = 8192,
// apply_inverse(y) 9.0 -> 6.6 ms at N = 65536 (two sweeps over 17 GB: 5.2 TB/s, 0.65 of HBM; was 0.39).
__device__ __forceinline__ double2 ld_coherent2(const double* p) {
  double2 v;
  v.x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v.y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v;
}
#define CHAIN_SENTINEL 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ bool chain_ready(double v) { return (unsigned long long)__double_as_longlong(v) != CHAIN_SENTINEL; }
// v[0..15] per lane -> returns, in lane l, the sum over all 64 lanes of v[l & 15]
__device__ __forceinline__ double transpose_sum16(double (&v)[16], int lane) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool up = (lane & 8) != 0;
    const double keep = up ? v[i + 8] : v[i], send = up ? v[i] : v[i + 8];
    v[i] = keep + __shfl_xor(send, 8, 64);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool up = (lane & 4) != 0;
    const double keep = up ? v[i + 4] : v[i], send = up ? v[i] : v[i + 4];
    v[i] = keep + __shfl_xor(send, 4, 64);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const bool up = (lane & 2) != 0;
    const double keep = up ? v[i + 2] : v[i], send = up ? v[i] : v[i + 2];
    v[i] = keep + __shfl_xor(send, 2, 64);
  }
  {
    const bool up = (lane & 1) != 0;
    const double keep = up ? v[1] : v[0], send = up ? v[0] : v[1];
    v[0] = keep + __shfl_xor(send, 1, 64);
  }
  double t = v[0];
  t += __shfl_xor(t, 16, 64);
  t += __shfl_xor(t, 32, 64);
  return t;
}
// The two arithmetic steps of a link, per right-hand side: shared by trsv_fwd_chain_direct and trsv_fwd_chain_multi, so that
// the compiler contracts them into the same multiply-adds in both (gh_chol_append's paths 1 and 2 give the same bits).
// acc[q] += (row q of the block) . z_j, this lane's two columns
__device__ __forceinline__ void chain_fold16(double (&acc)[16], const double2 (&blk)[16], const double2 zj) {
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] += blk[q].x * zj.x + blk[q].y * zj.y;
}
// an empty statement that reads the sixteen sums and may touch memory: arithmetic on them stays in front of it, loads behind it
__device__ __forceinline__ void chain_pin16(double (&a)[16]) {
  asm volatile("" : : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]),
               "v"(a[10]), "v"(a[11]), "v"(a[12]), "v"(a[13]), "v"(a[14]), "v"(a[15]) : "memory");
}
// acc[q] = (row q of the diagonal block's inverse) . w, this lane's two columns
__device__ __forceinline__ void chain_rows16(double (&acc)[16], const double2 (&dv)[16], const double wx, const double wy) {
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = dv[q].x * wx + dv[q].y * wy;
}
__global__ __launch_bounds__(CHAIN_THREADS) void trsv_fwd_chain_direct(const double* L, long ld, const double* dinv,
                                                                       const double* y, double* z, int* fail) {
  __shared__ double zs[2][T];
  __shared__ double ws[T];
  __shared__ int gave_up;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row0 = (long)b * T + wave * 16;
  double acc[16];
  double2 dv[16], blk[16];
  if (tid == 0) gave_up = 0;
  const double yv = y[row0 + (lane & 15)];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    acc[q] = 0.0;
    dv[q] = *reinterpret_cast<const double2*>(dinv + (long)b * T * T + (wave * 16 + q) * T + 2 * lane);
  }
  if (b > 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) blk[q] = *reinterpret_cast<const double2*>(L + (row0 + q) * ld + 2 * lane);
  }
  __syncthreads();
  for (int j = 0; j < b; ++j) {
    if (wave == 0) {
      // The further from the front of the chain, the more patiently: a waiting workgroup first probes ONE value with one
      // lane (one request; every waiting workgroup hammering all 128 was the L2 queue as the critical path), and only the
      // next two in line poll the whole block at once.
      const int dist = b - j;
      GhSpin spin(fail);                                  // (gh_spin.h: the 2-s give-up and the abort word)
      bool ok = true;
      if (dist > 2) {
        while (!chain_ready(__hip_atomic_load(z + (long)j * T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
          for (int q = dist > 64 ? 16 : dist >> 2; q > 0; --q) __builtin_amdgcn_s_sleep(8);   // 0 .. 8k cycles
          if (!spin.keep_waiting(63u)) { ok = false; break; }
        }
      }
      double2 zj = ld_coherent2(z + (long)j * T + 2 * lane);
      while (ok && !__all(chain_ready(zj.x) && chain_ready(zj.y))) {
        if (!spin.keep_waiting(1023u)) { ok = false; break; }
        zj = ld_coherent2(z + (long)j * T + 2 * lane);
      }
      if (!ok && lane == 0) gave_up = 1;
      *reinterpret_cast<double2*>(&zs[j & 1][2 * lane]) = zj;
    }
    __syncthreads();
    if (gave_up) break;
    const double2 zj = *reinterpret_cast<const double2*>(&zs[j & 1][2 * lane]);
    chain_fold16(acc, blk, zj);
    if (j + 1 < b) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        blk[q] = *reinterpret_cast<const double2*>(L + (row0 + q) * ld + (long)(j + 1) * T + 2 * lane);
    }
  }
  // (after a time-out the values published are garbage but NOT the sentinel: the workgroups behind come through, the
  //  host sees *fail)
  const double tot = transpose_sum16(acc, lane);
  if (lane < 16) ws[wave * 16 + lane] = yv - tot;
  __syncthreads();
  const double wx = ws[2 * lane], wy = ws[2 * lane + 1];
  chain_rows16(acc, dv, wx, wy);
  double v = transpose_sum16(acc, lane);
  if (!chain_ready(v)) v = __longlong_as_double(0x7FF8000000000000LL);      // (a NaN with every bit set must not look unpublished)
  if (lane < 16) __hip_atomic_store(z + row0 + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The same sweep for R right-hand sides in one launch (gh_chol_append: R new rows of the factor against its full tiles): the
// factor is read ONCE for all of them.  Same protocol -- the outputs are pre-filled with the sentinel and are the message,
// agent-scope relaxed atomics and no fences, the patient probing by distance (on the first right-hand side), GhSpin -- and,
// per right-hand side, the same operation sequence through chain_fold16 / transpose_sum16 / chain_rows16: the bits of R runs
// of trsv_fwd_chain_direct.  y: R vectors ldy apart, read only, no alias of z; z: R vectors ldz apart.
// Registers at 512 threads (256 per lane): acc[R][16] is 32 R, blk 64; the diagonal block's inverse (64 more) would not fit
// beside them at R = 4, so it waits in LDS (128 KiB; a wavefront stages and reads back its own 16 rows) until blk is dead.
template <int R>
__global__ __launch_bounds__(CHAIN_THREADS) void trsv_fwd_chain_multi(const double* L, long ld, const double* dinv,
                                                                      const double* y, long ldy, double* z, long ldz, int* fail) {
  __shared__ double zs[2][R][T];
  __shared__ double ws[R][T];
  __shared__ double dls[T * T];
  __shared__ int gave_up;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (wave-uniform row addresses: scalar bases, not sixteen 64-bit vector pointers)
  const long row0 = (long)b * T + wave * 16;
  double acc[R][16];
  double2 blk[16];
  if (tid == 0) gave_up = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lane < 16) ws[r][wave * 16 + lane] = y[r * ldy + row0 + lane];      // (waits in LDS: R registers fewer across the loop)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[r][q] = 0.0;
  }
#pragma unroll
  for (int q = 0; q < 16; ++q)
    *reinterpret_cast<double2*>(&dls[(wave * 16 + q) * T + 2 * lane]) =
        *reinterpret_cast<const double2*>(dinv + (long)b * T * T + (wave * 16 + q) * T + 2 * lane);
  __builtin_amdgcn_sched_barrier(0);                      // (staged before the first block is asked for: its 64 registers are free again)
  if (b > 0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) blk[q] = *reinterpret_cast<const double2*>(L + (row0 + q) * ld + 2 * lane);
  }
  __syncthreads();
  for (int j = 0; j < b; ++j) {
    if (wave == 0) {
      const int dist = b - j;
      GhSpin spin(fail);
      bool ok = true;
      if (dist > 2) {
        while (!chain_ready(__hip_atomic_load(z + (long)j * T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
          for (int q = dist > 64 ? 16 : dist >> 2; q > 0; --q) __builtin_amdgcn_s_sleep(8);
          if (!spin.keep_waiting(63u)) { ok = false; break; }
        }
      }
      // one right-hand side after the other (they are published together; polling them side by side costs 6 R registers)
#pragma unroll 1
      for (int r = 0; r < R; ++r) {
        const double* zp = z + r * ldz + (long)j * T + 2 * lane;
        double2 zj = ld_coherent2(zp);
        while (ok && !__all(chain_ready(zj.x) && chain_ready(zj.y))) {
          if (!spin.keep_waiting(1023u)) { ok = false; break; }
          zj = ld_coherent2(zp);
        }
        *reinterpret_cast<double2*>(&zs[j & 1][r][2 * lane]) = zj;
      }
      if (!ok && lane == 0) gave_up = 1;
    }
    __syncthreads();
    if (gave_up) break;
#pragma unroll
    for (int r = 0; r < R; ++r) chain_fold16(acc[r], blk, *reinterpret_cast<const double2*>(&zs[j & 1][r][2 * lane]));
    // (the next block's loads must land in blk itself -- a second copy, which the compiler makes of its own accord by issuing them
    //  ahead of the multiply-adds, does not fit beside acc at R = 4: every sum is complete before the first load is issued)
#pragma unroll
    for (int r = 0; r < R; ++r) chain_pin16(acc[r]);
    if (j + 1 < b) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        blk[q] = *reinterpret_cast<const double2*>(L + (row0 + q) * ld + (long)(j + 1) * T + 2 * lane);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double yv = ws[r][wave * 16 + (lane & 15)];
    const double tot = transpose_sum16(acc[r], lane);
    if (lane < 16) ws[r][wave * 16 + lane] = yv - tot;
  }
  __syncthreads();
  double2 dv[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) dv[q] = *reinterpret_cast<const double2*>(&dls[(wave * 16 + q) * T + 2 * lane]);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    chain_rows16(acc[r], dv, ws[r][2 * lane], ws[r][2 * lane + 1]);
    double v = transpose_sum16(acc[r], lane);
    if (!chain_ready(v)) v = __longlong_as_double(0x7FF8000000000000LL);
    if (lane < 16) __hip_atomic_store(z + r * ldz + row0 + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Backward step j of L^T x = z.  x_j = L_jj^-T w_j; columns c < j0: w[c] -= sum_r L[j0+r][c] x_j[r].
// Workgroup j0/128 (the last one) publishes x_j; workgroup b < j0/128 updates columns [128b, 128b+128).
__global__ __launch_bounds__(256) void trsv_bwd_step(const double* L, long ld, const double* dinv_j,
                                                     long j0, double* w, double* x) {
  __shared__ double xj[T];
  __shared__ double part[2][T];
  const int tid = threadIdx.x, c = tid & 127, h = tid >> 7;
  double acc = 0.0;
#pragma unroll 16
  for (int r = h * 64; r < h * 64 + 64; ++r) acc += dinv_j[r * T + c] * w[j0 + r];
  part[h][c] = acc;
  __syncthreads();
  if (tid < T) xj[tid] = part[0][tid] + part[1][tid];
  __syncthreads();
  const long nb = j0 / T;
  if ((long)blockIdx.x == nb) {
    if (tid < T) x[j0 + tid] = xj[tid];
    return;
  }
  const long col0 = (long)blockIdx.x * T;
  acc = 0.0;
#pragma unroll 16
  for (int r = h * 64; r < h * 64 + 64; ++r) acc += L[(j0 + r) * ld + col0 + c] * xj[r];
  __syncthreads();
  part[h][c] = acc;
  __syncthreads();
  if (tid < T) w[col0 + tid] -= part[0][tid] + part[1][tid];
}

// The backward sweep L^T x = z as one chained launch, the mirror image of trsv_fwd_chain_direct: the
// chain runs from the LAST block to the first, so workgroup w owns block column b = nt-1-w (its
// predecessors in the chain then have smaller workgroup indices and are dispatched first).
//   x_b = L_bb^-T ( z_b - sum_{j>b} L_jb^T x_j )
// Wavefront v takes rows 16v..16v+15 of every block L_jb (row segments of 1 KiB, a lane two
// columns), accumulates its lane's two columns of L_jb^T x_j over all j, and the eight wavefront
// partials meet in LDS once, before the diagonal solve (same scheme again with L_bb^-1).
// x itself is the message, as in trsv_fwd_chain_direct: x pre-filled with the sentinel, the first wavefront of a
// consumer polls the 128 values of x_j and hands them on through LDS (they used to be sixteen broadcast loads from
// L2 per wavefront, after the flag had been seen).
__global__ __launch_bounds__(CHAIN_THREADS) void trsv_bwd_chain_direct(const double* L, long ld, const double* dinv, int nt,
                                                                       const double* zin, double* x, int* fail) {
  __shared__ double red[8][T];
  __shared__ double wv[T];
  __shared__ double xs[2][T];
  __shared__ int gave_up;
  const int w = blockIdx.x, b = nt - 1 - w;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long col0 = (long)b * T + 2 * lane;
  double2 acc = make_double2(0.0, 0.0);
  double2 dv[16], blk[16];
  if (tid == 0) gave_up = 0;
  const double zv = tid < T ? zin[(long)b * T + tid] : 0.0;
#pragma unroll
  for (int q = 0; q < 16; ++q)
    dv[q] = *reinterpret_cast<const double2*>(dinv + (long)b * T * T + (wave * 16 + q) * T + 2 * lane);
  if (b + 1 < nt) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      blk[q] = *reinterpret_cast<const double2*>(L + ((long)(nt - 1) * T + wave * 16 + q) * ld + col0);
  }
  __syncthreads();
  for (int j = nt - 1; j > b; --j) {
    if (wave == 0) {
      const int dist = j - b;
      GhSpin spin(fail);
      bool ok = true;
      if (dist > 2) {
        while (!chain_ready(__hip_atomic_load(x + (long)j * T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
          for (int q = dist > 64 ? 16 : dist >> 2; q > 0; --q) __builtin_amdgcn_s_sleep(8);
          if (!spin.keep_waiting(63u)) { ok = false; break; }
        }
      }
      double2 xj = ld_coherent2(x + (long)j * T + 2 * lane);
      while (ok && !__all(chain_ready(xj.x) && chain_ready(xj.y))) {
        if (!spin.keep_waiting(1023u)) { ok = false; break; }
        xj = ld_coherent2(x + (long)j * T + 2 * lane);
      }
      if (!ok && lane == 0) gave_up = 1;
      *reinterpret_cast<double2*>(&xs[j & 1][2 * lane]) = xj;
    }
    __syncthreads();
    if (gave_up) break;
    const double* xw = &xs[j & 1][wave * 16];              // x_j[16 wave + q]: LDS broadcast reads
#pragma unroll
    for (int q = 0; q < 16; ++q) { const double xr = xw[q]; acc.x += blk[q].x * xr; acc.y += blk[q].y * xr; }
    if (j - 1 > b) {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        blk[q] = *reinterpret_cast<const double2*>(L + ((long)(j - 1) * T + wave * 16 + q) * ld + col0);
    }
  }
  red[wave][2 * lane] = acc.x;
  red[wave][2 * lane + 1] = acc.y;
  __syncthreads();
  if (tid < T) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += red[q][tid];
    wv[tid] = zv - v;
  }
  __syncthreads();
  acc = make_double2(0.0, 0.0);                         // x_b[c] = sum_r dinv_b[r][c] w[r]
#pragma unroll
  for (int q = 0; q < 16; ++q) { const double wr = wv[wave * 16 + q]; acc.x += dv[q].x * wr; acc.y += dv[q].y * wr; }
  __syncthreads();
  red[wave][2 * lane] = acc.x;
  red[wave][2 * lane + 1] = acc.y;
  __syncthreads();
  if (tid < T) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += red[q][tid];
    if (!chain_ready(v)) v = __longlong_as_double(0x7FF8000000000000LL);
    __hip_atomic_store(x + (long)b * T + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ========================================================= small helpers
__global__ void fill_kernel(double* p, long n, double v) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void eye_kernel(double* p, long n, long ld) {   // p must be pre-zeroed
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i * ld + i] = 1.0;
}
// mirror the lower triangle of an n x n matrix into the upper one (out may be != in)
__global__ void symmetrize_kernel(const double* in, long ldi, double* out, long ldo, long n) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n * n) return;
  const long i = idx / n, j = idx % n;
  out[i * ldo + j] = (j <= i) ? in[i * ldi + j] : in[j * ldi + i];
}
__global__ void copy2d_kernel(const double* in, long ldi, double* out, long ldo, long rows, long cols) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * cols) return;
  const long i = idx / cols, j = idx % cols;
  out[i * ldo + j] = in[i * ldi + j];
}

// ================================================= cross-validation: the sum of lpd, the sweeps' time-out note
// out[0] = sum_{i < n} a[i]: one workgroup, or slices added in index order (launch_sum, as launch_dot)
__global__ __launch_bounds__(256) void sum_part_kernel(const double* a, long n, double* part) {
  __shared__ double sh[4];
  const long per = (n + gridDim.x - 1) / gridDim.x;
  const long lo = (long)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  double v = 0.0;
  for (long i = lo + threadIdx.x; i < hi; i += 256) v += a[i];
  v = block_sum_256(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
static int launch_sum(const double* a, long n, double* out, double* part, hipStream_t st) {
  const int g = (int)std::max<long>(1, std::min<long>(RED_SLICES, (n + 4095) / 4096));
  hipLaunchKernelGGL(sum_part_kernel, dim3(g), dim3(256), 0, st, a, n, part);
  hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(64), 0, st, part, g, 1.0, out, 0, (const int*)nullptr);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
// *acc = 1 when one of the chained sweeps just enqueued gave up waiting: several deferred pairs of sweeps share the flag words,
// which every launch clears
__global__ void chain_fail_note_kernel(const int* ff, const int* fb, double* acc) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && (*ff != 0 || *fb != 0)) *acc = 1.0;
}

// ======================================================== the sweeps' launchers
// z = L^-1 w as one chained launch; flags[nt] = the time-out flag (cleared here; the words before it are no longer
// used: the flag-per-block-row kernels are retired, scripts/dev/arms/trsv_chain_flags.hip.inc).  w is read only and
// must not be z (z is pre-filled with the sentinel).
int gh_launch_trsv_fwd_chain(const double* L, long ld, const double* dinv, int64_t nt, const double* w, double* z,
                             unsigned* flags, hipStream_t st) {
  GH_HIP(hipMemsetAsync(flags + nt, 0, sizeof(unsigned), st));
  GH_HIP(hipMemsetAsync(z, 0xFF, (size_t)nt * T * sizeof(double), st));
  hipLaunchKernelGGL(trsv_fwd_chain_direct, dim3((unsigned)nt), dim3(CHAIN_THREADS), 0, st, L, ld, dinv, w, z, (int*)(flags + nt));
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_trsv_bwd_chain(const double* L, long ld, const double* dinv, int64_t nt, const double* w, double* x,
                             unsigned* flags, hipStream_t st) {
  GH_HIP(hipMemsetAsync(flags + nt, 0, sizeof(unsigned), st));
  GH_HIP(hipMemsetAsync(x, 0xFF, (size_t)nt * T * sizeof(double), st));
  hipLaunchKernelGGL(trsv_bwd_chain_direct, dim3((unsigned)nt), dim3(CHAIN_THREADS), 0, st, L, ld, dinv, (int)nt, w, x, (int*)(flags + nt));
  GH_HIP(hipGetLastError());
  return GH_OK;
}
// gh_chol_append's new rows against the full tiles: four and two right-hand sides per pass over the factor while they last (multi),
// the rest one by one
int gh_launch_trsv_fwd_chain_rows(const double* L, long ld, const double* dinv, int64_t nt0, const double* Y, long ldy, double* Z, long ldz,
                                  int64_t m, bool multi, int* fail, hipStream_t st) {
  const dim3 grid((unsigned)nt0), block(CHAIN_THREADS);
  int64_t i = 0;
  if (multi) {
    for (; m - i >= 4; i += 4)
      hipLaunchKernelGGL(trsv_fwd_chain_multi<4>, grid, block, 0, st, L, ld, dinv, Y + i * ldy, ldy, Z + i * ldz, ldz, fail);
    for (; m - i >= 2; i += 2)
      hipLaunchKernelGGL(trsv_fwd_chain_multi<2>, grid, block, 0, st, L, ld, dinv, Y + i * ldy, ldy, Z + i * ldz, ldz, fail);
  }
  for (; i < m; ++i)
    hipLaunchKernelGGL(trsv_fwd_chain_direct, grid, block, 0, st, L, ld, dinv, Y + i * ldy, Z + i * ldz, fail);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_chain_timeout(const char* who, bool forward_failed, bool backward_failed) {
  if (!forward_failed && !backward_failed) return GH_OK;
  if (!who) gh_set_error("%s solve: a workgroup waited more than 2 s for its predecessor", forward_failed ? "forward" : "backward");
  else if (!strcmp(who, "append")) gh_set_error("append: a workgroup of the forward sweep waited more than 2 s for its predecessor");
  else gh_set_error("%s: a chained solve waited more than 2 s for its predecessor", who);
  return GH_ERR_HIP;
}
// A/B arm: one launch per block row instead of the chained sweeps (read once per process)
static bool gh_trsv_stepwise() {
  static const bool stepwise = getenv("GEORGE_AMD_TRSV_STEPS") != nullptr;
  return stepwise;
}

// ======================================================== the protocols of the entry points
// What every entry point on a computed factor with a kernel does first, in this order: the handle, the arguments (bad_arg: the
// message), the kernel's dimension, its upload.
static int enter_computed(gh_chol* s, gh_kernel* k, bool args_ok, const char* bad_arg) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!args_ok) { gh_set_error("%s", bad_arg); return GH_ERR_BAD_ARG; }
  if (k->ndim != s->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  return k->upload();
}
// the main stream takes over from the stream the factorisation ended on (the solves and the products run on the main stream)
static int join_tail(gh_chol* s) {
  if (s->tail && s->tail != s->st && s->ev_sync[1]) {
    GH_HIP(hipEventRecord(s->ev_sync[1], s->tail));
    GH_HIP(hipStreamWaitEvent(s->st, s->ev_sync[1], 0));
  }
  return GH_OK;
}
// load a length-n vector (host or device) into a zero-padded device vector of length np
static int load_vec(gh_chol* s, GhBuf& buf, const double* src) {
  GH_CHECK(buf.ensure((size_t)s->np * sizeof(double)));
  if (s->np > s->n) GH_HIP(hipMemsetAsync(buf.d() + s->n, 0, (size_t)(s->np - s->n) * sizeof(double), s->st));
  return gh_to_device(buf.d(), src, (size_t)s->n, s->st);
}
// z = L^-1 w  (w is destroyed)
// (defer: enqueue only; the caller reads the time-out flag back itself, fwd_fail() / bwd_fail())
static int trsv_forward(gh_chol* s, double* w, double* z, bool defer = false) {
  const int64_t nt = s->np / T;
  if (!gh_trsv_stepwise()) {
    GH_CHECK(chain_ensure(s, nt));
    GH_CHECK(gh_launch_trsv_fwd_chain(s->A.d(), (long)s->np, s->dinv.d(), nt, w, z, fwd_flags(s), s->st));
    if (defer) return GH_OK;
    int failed = 0;
    GH_HIP(hipMemcpyAsync(&failed, fwd_fail(s), sizeof(int), hipMemcpyDeviceToHost, s->st));
    GH_HIP(hipStreamSynchronize(s->st));
    return gh_chain_timeout(nullptr, failed != 0, false);
  }
  for (int64_t j = 0; j < nt; ++j) {
    hipLaunchKernelGGL(trsv_fwd_step, dim3((unsigned)(nt - j)), dim3(256), 0, s->st,
                       s->A.d(), (long)s->np, s->dinv.d() + j * T * T, (long)(j * T), w, z);
  }
  GH_HIP(hipGetLastError());
  return GH_OK;
}
// x = L^-T w  (w is destroyed)
static int trsv_backward(gh_chol* s, double* w, double* x, bool defer = false) {
  const int64_t nt = s->np / T;
  if (!gh_trsv_stepwise()) {
    GH_CHECK(chain_ensure(s, nt));
    GH_CHECK(gh_launch_trsv_bwd_chain(s->A.d(), (long)s->np, s->dinv.d(), nt, w, x, bwd_flags(s), s->st));
    if (defer) return GH_OK;
    int failed = 0;
    GH_HIP(hipMemcpyAsync(&failed, bwd_fail(s), sizeof(int), hipMemcpyDeviceToHost, s->st));
    GH_HIP(hipStreamSynchronize(s->st));
    return gh_chain_timeout(nullptr, false, failed != 0);
  }
  for (int64_t j = nt - 1; j >= 0; --j) {
    hipLaunchKernelGGL(trsv_bwd_step, dim3((unsigned)(j + 1)), dim3(256), 0, s->st,
                       s->A.d(), (long)s->np, s->dinv.d() + j * T * T, (long)(j * T), w, x);
  }
  GH_HIP(hipGetLastError());
  return GH_OK;
}

extern "C" int gh_chol_dot_solve(gh_chol* s, const double* y, double* out) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!y || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  // y^T K^-1 y = || L^-1 y ||^2 : one forward sweep (the reference does both, basic.py:102)
  const bool stepwise = gh_trsv_stepwise();
  // (the chained kernel only READS its right-hand side: a device-resident y of full padded length is used where it lies)
  const bool direct = !stepwise && s->np == s->n && gh_is_device_ptr(y);
  if (!direct) GH_CHECK(load_vec(s, s->v0, y));
  GH_CHECK(s->v1.ensure((size_t)s->np * sizeof(double)));
  const long e = s->opts.profile ? s->next_ev() : -1;
  if (e >= 0) GH_HIP(hipEventRecord(s->ev_pool[e].a, s->st));
  GH_CHECK(trsv_forward(s, direct ? const_cast<double*>(y) : s->v0.d(), s->v1.d(), !stepwise));
  const int* fail = stepwise ? nullptr : fwd_fail(s);
  GH_CHECK(launch_dot(s->v1.d(), s->v1.d(), (long)s->np, s->scal.d() + 1, s->scal.d() + 72, s->st, fail));
  if (e >= 0) GH_HIP(hipEventRecord(s->ev_pool[e].b, s->st));
  double back[3] = {0.0, 0.0, 0.0};                     // [0] quadratic form, [1] (failure word of compute()), [2] the chain's time-out flag
  GH_HIP(hipMemcpyAsync(back, s->scal.d() + 1, 3 * sizeof(double), hipMemcpyDeviceToHost, s->st));
  GH_HIP(hipStreamSynchronize(s->st));
  if (e >= 0) { float ms = 0; GH_HIP(hipEventElapsedTime(&ms, s->ev_pool[e].a, s->ev_pool[e].b)); s->prof.ms_solve = ms; }
  GH_CHECK(gh_chain_timeout(nullptr, !stepwise && back[2] != 0.0, false));
  *out = back[0];
  return GH_OK;
}

// B (np x rp, row-major, zero padded) <- L^-1 B  (forward) and optionally L^-T (backward)
// Two-level blocking: 128-row steps (multiplication by the stored diagonal inverse + a small
// update) inside super-blocks of SB = 8 tiles, then ONE K = 128*SB update of everything below (above)
// the super-block -- the right-hand side is swept N/(128*SB) times instead of N/128 times.
// `tri`: B is the identity being overwritten by L^-1 (forward only): block row j is non-zero in
// columns [0, (j+1)*128) only, so every product is clipped to those columns.
// (_on: on any factor L of pitch np with its diagonal-block inverses dinv; trsm_multi below is the handle's own)
static int trsm_multi_on(hipStream_t st, const double* L, const double* dinv, int64_t np, double* B, int64_t rp, bool forward, bool backward,
                         bool tri) {
  // (tiles per super-block; measured at N = 32768 with 4096 right-hand sides, both sweeps: 2 -> 167 ms, 4 -> 158.5,
  //  8 -> 151.6, 16 -> 149.5; no difference at N = 8192; the switch that overrode it went in round 4)
  const int64_t SB = 8;
  const int64_t nt = np / T;
  auto mm = [&](double* Cp, const double* Ap, int64_t lda, bool a_km, const double* Bp, int64_t M, int64_t N, int64_t K,
                double alpha, double beta) -> int {
    if (M <= 0 || N <= 0) return GH_OK;
    return gh_launch_gemm(gemm_desc(Cp, rp, Ap, lda, a_km, Bp, rp, false, M, N, K, alpha, beta), st);
  };
  if (forward) {
    for (int64_t J = 0; J < nt; J += SB) {
      const int64_t Je = std::min<int64_t>(J + SB, nt);
      for (int64_t j = J; j < Je; ++j) {
        double* Bj = B + j * T * rp;
        const int64_t nc = tri ? (j + 1) * T : rp;
        GH_CHECK(mm(Bj, dinv + j * T * T, T, true, Bj, T, nc, T, 1.0, 0.0));                        // B_j <- L_jj^-1 B_j
        GH_CHECK(mm(B + (j + 1) * T * rp, L + (j + 1) * T * np + j * T, np, true, Bj,
                    (Je - j - 1) * T, nc, T, -1.0, 1.0));                                           // rows of the super-block
      }
      const int64_t nc = tri ? Je * T : rp;
      GH_CHECK(mm(B + Je * T * rp, L + Je * T * np + J * T, np, true, B + J * T * rp,
                  (nt - Je) * T, nc, (Je - J) * T, -1.0, 1.0));                                     // everything below
    }
  }
  if (backward) {
    for (int64_t Je = nt; Je > 0; Je -= SB) {
      const int64_t J = std::max<int64_t>(Je - SB, 0);
      for (int64_t j = Je - 1; j >= J; --j) {
        double* Bj = B + j * T * rp;
        GH_CHECK(mm(Bj, dinv + j * T * T, T, false, Bj, T, rp, T, 1.0, 0.0));                       // B_j <- L_jj^-T B_j
        GH_CHECK(mm(B + J * T * rp, L + j * T * np + J * T, np, false, Bj, (j - J) * T, rp, T, -1.0, 1.0));
      }
      GH_CHECK(mm(B, L + J * T * np, np, false, B + J * T * rp, J * T, rp, (Je - J) * T, -1.0, 1.0));   // everything above
    }
  }
  return GH_OK;
}
static int trsm_multi(gh_chol* s, double* B, int64_t rp, bool forward, bool backward, bool tri = false) {
  return trsm_multi_on(s->st, s->A.d(), s->dinv.d(), s->np, B, rp, forward, backward, tri);
}

extern "C" int gh_chol_solve(gh_chol* s, const double* b, int64_t nrhs, double* out) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!b || !out || nrhs <= 0) { gh_set_error("bad argument to solve"); return GH_ERR_BAD_ARG; }
  const int64_t n = s->n, np = s->np;
  if (nrhs == 1) {
    GH_CHECK(load_vec(s, s->v0, b));
    GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
    GH_CHECK(s->v2.ensure((size_t)np * sizeof(double)));
    GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d()));
    GH_CHECK(trsv_backward(s, s->v1.d(), s->v2.d()));
    GH_CHECK(gh_from_device(out, s->v2.d(), (size_t)n, s->st));
    GH_HIP(hipStreamSynchronize(s->st));                  // (a device `out` is only enqueued by gh_from_device)
    return GH_OK;
  }
  const int64_t rp = gh_round_up(nrhs, T);
  GH_CHECK(s->rhs.ensure((size_t)np * rp * sizeof(double)));
  GH_HIP(hipMemsetAsync(s->rhs.d(), 0, (size_t)np * rp * sizeof(double), s->st));
  GH_CHECK(gh_copy_rows(s->rhs.d(), rp, b, nrhs, nrhs, n, true, s->st));
  GH_CHECK(trsm_multi(s, s->rhs.d(), rp, true, true));
  GH_CHECK(gh_copy_rows(out, nrhs, s->rhs.d(), rp, nrhs, n, false, s->st));
  GH_HIP(hipStreamSynchronize(s->st));
  return GH_OK;
}

extern "C" int gh_chol_apply_sqrt(gh_chol* s, const double* r, int64_t nrows, double* out) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!r || !out || nrows <= 0) { gh_set_error("bad argument to apply_sqrt"); return GH_ERR_BAD_ARG; }
  // out = r @ U with U = L^T (basic.py:114):  out[s][j] = sum_{k <= j} r[s][k] L[j][k]
  const int64_t n = s->n, np = s->np, rr = gh_round_up(nrows, T);
  GH_CHECK(s->rhs.ensure((size_t)rr * np * sizeof(double)));
  GH_CHECK(s->work.ensure((size_t)rr * np * sizeof(double)));
  GH_HIP(hipMemsetAsync(s->rhs.d(), 0, (size_t)rr * np * sizeof(double), s->st));
  GH_CHECK(gh_copy_rows(s->rhs.d(), np, r, n, n, nrows, true, s->st));
  GhGemm g = gemm_desc(s->work.d(), np, s->rhs.d(), np, true, s->A.d(), np, true, rr, np, np, 1.0, 0.0);
  g.khi_col = true;
  GH_CHECK(gh_launch_gemm(g, s->st));
  GH_CHECK(gh_copy_rows(out, n, s->work.d(), np, n, nrows, false, s->st));
  GH_HIP(hipStreamSynchronize(s->st));
  return GH_OK;
}

// Linv (np x np) <- L^-1: forward substitution on the identity, exploiting the lower-triangular right-hand side (tri = true).
// Handle-free (declared in gh_chol_impl.h): the inducing-point solver inverts its two m x m factors with it.
int gh_chol_linv(hipStream_t st, const double* L, const double* dinv, int64_t np, double* Linv) {
  GH_HIP(hipMemsetAsync(Linv, 0, (size_t)np * np * sizeof(double), st));
  hipLaunchKernelGGL(eye_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, Linv, (long)np, (long)np);
  GH_HIP(hipGetLastError());
  return trsm_multi_on(st, L, dinv, np, Linv, np, true, false, true);
}
static int linv_into(gh_chol* s, double* Linv) { return gh_chol_linv(s->st, s->A.d(), s->dinv.d(), s->np, Linv); }
// W (np x np) <- K^-1, lower triangle valid.  Uses K^-1 = L^-T L^-1:
//   Linv = L^-1 (forward substitution on the identity), K^-1 = Linv^T Linv (k >= max(i, j)).
static int inverse_lower(gh_chol* s, double* W /* np*np */, double* Linv /* np*np scratch */) {
  const int64_t np = s->np;
  GH_CHECK(linv_into(s, Linv));
  GhGemm q = gemm_desc(W, np, Linv, np, false, Linv, np, false, np, np, np, 1.0, 0.0);
  q.lower = true; q.klo_max = true;
  return gh_launch_gemm(q, s->st);
}

extern "C" int gh_chol_get_inverse(gh_chol* s, double* out) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!out) { gh_set_error("null output"); return GH_ERR_BAD_ARG; }
  const int64_t n = s->n, np = s->np;
  GH_CHECK(s->work.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(s->work2.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(inverse_lower(s, s->work.d(), s->work2.d()));
  // full symmetric n x n result (work2 is free again)
  double* full = s->work2.d();
  const long tot = (long)n * n;
  hipLaunchKernelGGL(symmetrize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s->st, s->work.d(), (long)np, full, (long)n, (long)n);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_from_device(out, full, (size_t)tot, s->st));
  GH_HIP(hipStreamSynchronize(s->st));                    // (a device `out` is only enqueued by gh_from_device)
  return GH_OK;
}

// Everything of gh_chol_predict but its synchronisation, enqueued on the main stream.  keep_cov: the covariance is formed in
// s->work (mp x mp, pitch mp; the caller's cov may then be NULL) for a caller that goes on with it on the device
// (gh_chol_sample_conditional); *dmu_out: the mean on the device (in s->scratch), *xs_dev_out: the test points there (xsd owns
// them when they came from the host).  mu may be NULL with keep_cov.
static int predict_enqueue(gh_chol* s, gh_kernel* k, const double* r, const double* xs, int64_t m,
                           double* mu, double* var, double* cov, bool keep_cov, GhBuf& xsd, double** dmu_out,
                           const double** xs_dev_out) {
  const int64_t n = s->n, np = s->np, mp = gh_round_up(m, T);
  hipStream_t st = s->st;
  // z = L^-1 r
  GH_CHECK(load_vec(s, s->v0, r));
  GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
  GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d()));
  // V = L^-1 K(x, xs)   (np x mp): built on the device, forward substitution only, because
  // K*s K^-1 K*s^T = V^T V and K*s K^-1 r = V^T z  (gp.py:532-545 does both sweeps on the host)
  const double* xs_dev = nullptr;
  GH_CHECK(gh_stage_points(xs, m, s->ndim, xsd, st, &xs_dev));
  GH_CHECK(s->rhs.ensure((size_t)np * mp * sizeof(double)));
  GH_CHECK(gh_launch_kmat(k, s->x.d(), n, xs_dev, m, nullptr, s->rhs.d(), mp, np, mp, 0, 0, false, false, st));
  GH_CHECK(trsm_multi(s, s->rhs.d(), mp, true, false));
  // column reductions
  const int64_t nchunks = std::min<int64_t>(64, np / T);
  const int64_t rows_per = gh_round_up((np + nchunks - 1) / nchunks, 1);
  GH_CHECK(s->scratch.ensure((size_t)(2 * nchunks * mp + 2 * mp) * sizeof(double)));
  double* pmu = s->scratch.d();
  double* pvar = pmu + nchunks * mp;
  double* dmu = pvar + nchunks * mp;
  double* dvar = dmu + mp;
  if (var) GH_CHECK(gh_launch_kdiag(k, xs_dev, xs_dev, m, dvar, st));           // gp.py:539
  // (the m columns in use start as many 256-thread workgroups as the mp padded ones: mp rounds m up to 128)
  GH_CHECK(gh_launch_colreduce(s->rhs.d(), s->v1.d(), s->rhs.d(), s->rhs.d(), mp, np, rows_per, nchunks, m, pmu, pvar, mp, dmu,
                               var ? dvar : nullptr, 256, st));
  if (mu) GH_CHECK(gh_from_device(mu, dmu, (size_t)m, st));
  if (var) GH_CHECK(gh_from_device(var, dvar, (size_t)m, st));
  if (cov || keep_cov) {
    // cov = K(xs, xs) - V^T V      (gp.py:543-545)
    GH_CHECK(s->work.ensure((size_t)mp * mp * sizeof(double)));
    GH_CHECK(gh_launch_kmat(k, xs_dev, m, xs_dev, m, nullptr, s->work.d(), mp, mp, mp, 0, 0, true, false, st));
    GH_CHECK(gh_launch_gemm(gemm_desc(s->work.d(), mp, s->rhs.d(), mp, false, s->rhs.d(), mp, false, mp, mp, np, -1.0, 1.0), st));
    if (cov) GH_CHECK(gh_copy_rows(cov, m, s->work.d(), mp, m, m, false, st));
  }
  if (dmu_out) *dmu_out = dmu;
  if (xs_dev_out) *xs_dev_out = xs_dev;
  return GH_OK;
}

extern "C" int gh_chol_predict(gh_chol* s, gh_kernel* k, const double* r, const double* xs, int64_t m,
                               double* mu, double* var, double* cov) {
  GH_CHECK(enter_computed(s, k, k && r && xs && mu && m > 0, "bad argument to predict"));
  GhBuf xsd;
  GH_CHECK(predict_enqueue(s, k, r, xs, m, mu, var, cov, false, xsd, nullptr, nullptr));
  GH_HIP(hipStreamSynchronize(s->st));
  return GH_OK;
}

// Input derivatives of the prediction on a computed handle (no reference counterpart; the formulas are in the header).  mu and var
// come out of predict_enqueue's own launches, bit for bit gh_chol_predict's.  Then alpha = L^-T z by the backward sweep and, only
// for dvar, W = L^-T V by trsm_multi backward IN PLACE in s->rhs -- predict's column reductions, the last readers of V, are ahead
// of it on the stream, so no second np x mp buffer exists -- and the fused evaluate-and-reduce kernel of gh_predgrad.hip.  The
// results gather in s->work and leave in one batch of copies before the only synchronisation this function adds to predict's.
// With dmu alone (mu, var and dvar all NULL) nothing needs V: the two sweeps for alpha, the kernel, one synchronisation.
extern "C" int gh_chol_predict_grad(gh_chol* s, gh_kernel* k, const double* r, const double* xs, int64_t m,
                                    double* mu, double* var, double* dmu, double* dvar) {
  GH_CHECK(enter_computed(s, k, k && r && xs && dmu && m > 0, "bad argument to predict_grad"));
  hipStream_t st = s->st;
  const int64_t n = s->n, np = s->np, mp = gh_round_up(m, T), nd = s->ndim;
  // [var (mp) | dmu (m nd) | dvar (m nd) | partial rows]; the mean stays where predict_enqueue leaves it (s->scratch)
  const size_t head = (size_t)(mp + 2 * m * nd);
  GH_CHECK(s->work.ensure((head + gh_predgrad_work_doubles(n, m, (int)nd, dvar != nullptr)) * sizeof(double)));
  double* var_dev = s->work.d();
  double* dmu_dev = var_dev + mp;
  double* dvar_dev = dmu_dev + m * nd;
  double* partial = dvar_dev + m * nd;
  GhBuf xsd;
  double* mu_dev = nullptr;
  const double* xs_dev = nullptr;
  const bool stepwise = gh_trsv_stepwise();
  const bool values = mu || var || dvar;                 // anything that needs V = L^-1 K(x, xs)
  if (values) {
    GH_CHECK(predict_enqueue(s, k, r, xs, m, nullptr, var ? var_dev : nullptr, nullptr, false, xsd, &mu_dev, &xs_dev));
  } else {
    // dmu alone needs alpha only: the forward sweep of predict_enqueue (the same launch: the same z, alpha and dmu bits) and
    // neither K(x, xs) nor a substitution with mp right-hand sides -- 0.3 instead of 2 ms at N = 4096, 7 instead of 38 at 65 536
    GH_CHECK(load_vec(s, s->v0, r));
    GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
    GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d(), true));
    GH_CHECK(gh_stage_points(xs, m, s->ndim, xsd, st, &xs_dev));
  }
  GH_CHECK(s->v2.ensure((size_t)np * sizeof(double)));
  GH_CHECK(trsv_backward(s, s->v1.d(), s->v2.d(), true));                       // alpha = L^-T z
  if (dvar) GH_CHECK(trsm_multi(s, s->rhs.d(), mp, false, true));               // W = L^-T V
  GH_CHECK(gh_launch_predgrad(k, s->x.d(), n, xs_dev, m, s->v2.d(), dvar ? s->rhs.d() : nullptr, mp, dmu_dev,
                              dvar ? dvar_dev : nullptr, partial, st));
  auto out = [&](double* dst, const double* src, size_t count) -> int {
    GH_HIP(hipMemcpyAsync(dst, src, count * sizeof(double), gh_is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    return GH_OK;
  };
  if (mu) GH_CHECK(out(mu, mu_dev, (size_t)m));
  if (var) GH_CHECK(out(var, var_dev, (size_t)m));
  GH_CHECK(out(dmu, dmu_dev, (size_t)(m * nd)));
  if (dvar) GH_CHECK(out(dvar, dvar_dev, (size_t)(m * nd)));
  int failed = 0, failed_fwd = 0;                        // the sweeps' time-out flags (the forward one: only where it was deferred)
  if (!stepwise) GH_HIP(hipMemcpyAsync(&failed, bwd_fail(s), sizeof(int), hipMemcpyDeviceToHost, st));
  if (!stepwise && !values) GH_HIP(hipMemcpyAsync(&failed_fwd, fwd_fail(s), sizeof(int), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  return gh_chain_timeout(nullptr, failed_fwd != 0, failed != 0);
}

// Posterior draws on a computed handle: mu and cov exactly as gh_chol_predict forms them (the same launches), cov left on the
// device and factored there by the pivoted Cholesky of gh_pstrf.hip, draws = mu + z L^T as one GEMM.  The default threshold
// is on the PRIOR's scale, m eps max diag K(xs, xs): the rounding error of cov = K** - V^T V is that of its two terms, however
// small the posterior variances are.  DESIGN.md section 4, "Sampling".
extern "C" int gh_chol_sample_conditional(gh_chol* s, gh_kernel* k, const double* r, const double* xs, int64_t m,
                                          const double* z, int64_t nz, double tol, double* mu, double* draws, double* fac,
                                          int64_t* rank) {
  GH_CHECK(enter_computed(s, k, k && r && xs && z && draws && rank && m > 0 && nz > 0, "bad argument to sample_conditional"));
  hipStream_t st = s->st;
  const int64_t mp = gh_round_up(m, T);
  GhBuf xsd;
  double* dmu = nullptr;
  const double* xs_dev = nullptr;
  GH_CHECK(predict_enqueue(s, k, r, xs, m, mu, nullptr, nullptr, true, xsd, &dmu, &xs_dev));
  // [prior diagonal (mp) | tol (1, padded to 32 doubles) | the work arrays of gh_sample_enqueue]
  const size_t head = (size_t)(mp + 32) * sizeof(double), wb = gh_sample_work_bytes(m, nz, 1);
  GH_CHECK(s->samp.ensure(head + wb));
  double* diag = s->samp.d();
  double* tol_dev = diag + mp;
  if (tol < 0.0) {
    GH_CHECK(gh_launch_kdiag(k, xs_dev, xs_dev, m, diag, st));
    GH_CHECK(gh_launch_prior_tol(diag, m, tol_dev, st));
  }
  GhSample q{};
  q.cov = s->work.d(); q.lda = mp; q.stride = mp * mp; q.m = m; q.nbatch = 1;
  q.tol = tol; q.tol_dev = tol < 0.0 ? tol_dev : nullptr; q.mu = dmu;
  q.z = z; q.nz = nz; q.draws = draws; q.fac = fac; q.rank = rank;
  q.work = (char*)s->samp.p + head; q.work_bytes = s->samp.bytes - head;
  const int rc = gh_sample_enqueue(q, st);
  GH_HIP(hipStreamSynchronize(st));
  return rc;
}

extern "C" int gh_chol_grad(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r,
                            double* grad, double* alpha, double* diagA) {
  GH_CHECK(enter_computed(s, k, k && which && r && grad, "bad argument to grad"));
  const int64_t n = s->n, np = s->np;
  hipStream_t st = s->st;
  // alpha = K^-1 r                       (gp.py:429)
  GH_CHECK(load_vec(s, s->v0, r));
  GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
  GH_CHECK(s->v2.ensure((size_t)np * sizeof(double)));
  GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d()));
  GH_CHECK(trsv_backward(s, s->v1.d(), s->v2.d()));
  // K^-1 (lower)                         (gp.py:436)
  GH_CHECK(s->work.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(s->work2.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(inverse_lower(s, s->work.d(), s->work2.d()));
  // 1/2 sum_ij A_ij dK_ij/dtheta, A = alpha alpha^T - K^-1   (gp.py:437,465-466), fused
  GH_CHECK(s->v0.ensure((size_t)std::max<int64_t>(np, GH_MAX_GRAD) * sizeof(double)));
  double* dgrad = s->v0.d();                       // v0 is free again
  double* ddiag = s->v1.d();                       // so is v1
  GH_CHECK(gh_launch_kgrad_reduce(k, which, s->x.d(), n, s->v2.d(), s->work.d(), np, dgrad, ddiag, s->scratch, st));
  if (k->size > 0) GH_CHECK(gh_from_device(grad, dgrad, (size_t)k->size, st));
  if (alpha) GH_CHECK(gh_from_device(alpha, s->v2.d(), (size_t)n, st));
  if (diagA) GH_CHECK(gh_from_device(diagA, ddiag, (size_t)n, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

// ============================================================ information of the hyper-parameters
// (no reference counterpart.)  F_ab = 1/2 tr(K^-1 D_a K^-1 D_b) in its symmetric form: with W_a = L^-1 D_a L^-T,
// F_ab = 1/2 sum_ij W_a[i,j] W_b[i,j].  K^-1 is never formed; work2 = L^-1, work = the intermediate T_a = L^-1 D_a (lower
// tiles), and a plane first holds D_a, then W_a (lower tiles).  Both products are triangular in k: N^3 / 3 + N^3 / 6
// multiply-adds per kernel parameter, N^3 / 6 per diagonal one (its T_a is a column scaling of L^-1).  Resident when every
// plane fits, else in blocks: one block resident, every later plane formed into one scratch plane and contracted against
// the block -- a pair's per-tile sums and their final tree are the same launches' arithmetic either way, so the bits do
// not depend on the blocking.  DESIGN.md section 4, "Information of the hyper-parameters".
// plane <- W of one parameter.  A kernel parameter's plane holds D already when have_d (a resident call evaluates all of them
// in one launch: one gh_eval_grad per pair of points); a diagonal parameter (kernel_param < 0) has drow, np entries.
static int fisher_form_plane(gh_chol* s, gh_kernel* k, int kernel_param, bool have_d, const double* drow, double* plane) {
  const int64_t np = s->np;
  hipStream_t st = s->st;
  double* Linv = s->work2.d();
  double* Tm = s->work.d();
  if (kernel_param >= 0) {
    if (!have_d) {
      GhFisherSel sel{};
      sel.n = 1; sel.idx[0] = (short)kernel_param;
      GH_CHECK(gh_launch_fisher_planes(k, sel, s->x.d(), s->n, np, plane, st));
    }
    GhGemm g = gemm_desc(Tm, np, Linv, np, true, plane, np, false, np, np, np, 1.0, 0.0);   // T = L^-1 D (lower tiles; L^-1 lower-triangular: k <= row)
    g.lower = true; g.khi_row = true;
    GH_CHECK(gh_launch_gemm(g, st));
  } else {
    GH_CHECK(gh_launch_fisher_scale(Linv, np, drow, Tm, st));
  }
  GhGemm g = gemm_desc(plane, np, Tm, np, true, Linv, np, true, np, np, np, 1.0, 0.0);     // W = T L^-T (lower tiles; k <= column)
  g.lower = true; g.khi_col = true;
  return gh_launch_gemm(g, st);
}

extern "C" int gh_chol_fisher(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* diag_rows, int32_t n_diag,
                              int64_t max_bytes, double* fisher) {
  GH_CHECK(enter_computed(s, k, k && fisher && n_diag >= 0 && n_diag <= GH_FISHER_MAX_DIAG && (n_diag == 0 || diag_rows) && (k->size <= 0 || which),
                          "bad argument to fisher"));
  const int64_t n = s->n, np = s->np;
  hipStream_t st = s->st;
  const int ptot = n_diag + k->size;
  if (ptot == 0) return GH_OK;
  // the active planes: the diagonal ones, then the selected kernel parameters
  GhFisherMap map{};
  int kpar[GH_MAX_GRAD + GH_FISHER_MAX_DIAG];          // kernel parameter of an active plane, -1 - p for diagonal row p
  int Q = 0;
  for (int p = 0; p < n_diag; ++p) { kpar[Q] = -1 - p; map.out[Q++] = (short)p; }
  for (int p = 0; p < k->size; ++p) if (which[p]) { kpar[Q] = p; map.out[Q++] = (short)(n_diag + p); }
  map.q = Q; map.ptot = ptot;
  if (Q == 0) {                                        // everything masked: zeros
    GH_CHECK(s->scratch.ensure((size_t)ptot * ptot * sizeof(double)));
    GH_HIP(hipMemsetAsync(s->scratch.d(), 0, (size_t)ptot * ptot * sizeof(double), st));
    GH_CHECK(gh_from_device(fisher, s->scratch.d(), (size_t)ptot * ptot, st));
    GH_HIP(hipStreamSynchronize(st));
    return GH_OK;
  }
  // how many planes beside L^-1 and T: the caller's budget and what the device can give (what the handle's own work
  // buffers hold now is re-used)
  const size_t pb = (size_t)np * np * sizeof(double);
  int64_t fit = Q;
  if (max_bytes > 0) fit = std::min<int64_t>(fit, max_bytes / (int64_t)pb - 2);
  size_t mfree = 0, mtot = 0;
  GH_HIP(hipMemGetInfo(&mfree, &mtot));
  const size_t have = mfree + s->work.bytes + s->work2.bytes + s->fish.bytes + gh_pool_parked_bytes();
  fit = std::min<int64_t>(fit, (int64_t)(have / pb) - 2);
  if (Q > 1 && fit < 2) {
    gh_set_error("fisher: not even two planes of %zu bytes fit beside L^-1 and the intermediate (max_bytes %lld, device %zu)",
                 pb, (long long)max_bytes, have);
    return GH_ERR_NOMEM;
  }
  if (fit < 1) { gh_set_error("fisher: no room for a plane of %zu bytes", pb); return GH_ERR_NOMEM; }
  const bool resident = fit >= Q;
  const int blk = resident ? Q : (int)fit - 1;         // planes of a block; blocked: one more plane is the scratch
  const int nslots = resident ? Q : blk + 1;
  GH_CHECK(s->work.ensure(pb));
  GH_CHECK(s->work2.ensure(pb));
  GH_CHECK(s->fish.ensure((size_t)nslots * pb));
  const int64_t tm = np / T, nblk = tm * (tm + 1) / 2;
  const int64_t npairs = (int64_t)Q * (Q + 1) / 2;
  // scratch: [diagonal rows (n_diag np) | partial (nblk npairs) | pair sums | F (ptot^2)]
  const size_t n_rows = (size_t)n_diag * np, n_part = (size_t)(nblk * npairs);
  GH_CHECK(s->scratch.ensure((n_rows + n_part + (size_t)npairs + (size_t)ptot * ptot) * sizeof(double)));
  double* drows = s->scratch.d();
  double* partial = drows + n_rows;
  double* pairsum = partial + n_part;
  double* F = pairsum + npairs;
  GH_HIP(hipMemsetAsync(F, 0, (size_t)ptot * ptot * sizeof(double), st));
  if (n_diag > 0) {
    GH_HIP(hipMemsetAsync(drows, 0, n_rows * sizeof(double), st));
    GH_CHECK(gh_copy_rows(drows, np, diag_rows, n, n, n_diag, true, st));
  }
  GH_CHECK(linv_into(s, s->work2.d()));
  auto slot = [&](int i) { return s->fish.d() + (size_t)i * np * np; };
  auto form = [&](int a, double* plane) -> int {
    return fisher_form_plane(s, k, kpar[a], resident, kpar[a] < 0 ? drows + (size_t)(-1 - kpar[a]) * np : nullptr, plane);
  };
  if (resident && Q > n_diag) {                        // every kernel plane's D in one launch: the slots behind the diagonal ones
    GhFisherSel sel{};
    for (int a = n_diag; a < Q; ++a) sel.idx[sel.n++] = (short)kpar[a];
    GH_CHECK(gh_launch_fisher_planes(k, sel, s->x.d(), n, np, slot(n_diag), st));
  }
  const double* pa[GH_MAX_GRAD + GH_FISHER_MAX_DIAG];
  int ia[GH_MAX_GRAD + GH_FISHER_MAX_DIAG];
  for (int b0 = 0; b0 < Q; b0 += blk) {
    const int b1 = std::min(b0 + blk, Q);
    for (int a = b0; a < b1; ++a) {
      GH_CHECK(form(a, slot(a - b0)));
      pa[a - b0] = slot(a - b0); ia[a - b0] = a;
    }
    GH_CHECK(gh_launch_fisher_pairs(pa, ia, b1 - b0, nullptr, nullptr, 0, Q, np, partial, st));
    for (int c = b1; c < Q; ++c) {                     // (blocked only: a resident call has one block)
      const double* pc = slot(blk);
      GH_CHECK(form(c, slot(blk)));
      GH_CHECK(gh_launch_fisher_pairs(pa, ia, b1 - b0, &pc, &c, 1, Q, np, partial, st));
    }
  }
  GH_CHECK(gh_launch_kgrad_final(partial, nblk, (int)npairs, pairsum, st));
  GH_CHECK(gh_launch_fisher_mirror(pairsum, map, F, st));
  GH_CHECK(gh_from_device(fisher, F, (size_t)ptot * ptot, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

// ============================================================ fused objective
// nll and its gradient (gp.py:470-480; the optimiser loop of docs/tutorials/hyper.rst:131-152) as
// ONE call: build K -> factor -> log-det -> z = L^-1 r (used for r^T K^-1 r = |z|^2 AND, through
// the backward sweep, for alpha) -> K^-1 -> 1/2 sum A_ij dK_ij/dtheta.  Nothing is synchronised
// until the very end; only scalars and N-vectors reach the host.  `grad == NULL`: the
// log-likelihood pieces only (compute + dot_solve without the second sweep and the inverse).
extern "C" int gh_chol_objective(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                                 const double* yerr, const double* r, const uint32_t* which,
                                 double* logdet, double* quad, double* grad, double* alpha, double* diagA) {
  if (!r || !logdet || !quad) { gh_set_error("bad argument to objective"); return GH_ERR_BAD_ARG; }
  if (grad && !which) { gh_set_error("objective: gradient requested without a parameter mask"); return GH_ERR_BAD_ARG; }
  ComputeCtx c;
  GH_CHECK(gh_chol_compute_enqueue(s, k, x, n, ndim, yerr, c));
  hipStream_t st = s->st;
  GH_CHECK(join_tail(s));
  const int64_t np = s->np;
  const bool want_alpha = grad || alpha || diagA;
  GH_CHECK(load_vec(s, s->v0, r));
  GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
  const bool stepwise = gh_trsv_stepwise();
  GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d(), true));
  GH_CHECK(launch_dot(s->v1.d(), s->v1.d(), (long)np, s->scal.d() + 1, s->scal.d() + 72, st, stepwise ? nullptr : fwd_fail(s)));   // -> scal[3]
  double* dgrad = nullptr;
  double* ddiag = nullptr;
  if (want_alpha) {
    GH_CHECK(s->v2.ensure((size_t)np * sizeof(double)));
    GH_CHECK(trsv_backward(s, s->v1.d(), s->v2.d(), true));                          // alpha (v1 is consumed)
  }
  if (grad || diagA) {
    GH_CHECK(s->work.ensure((size_t)np * np * sizeof(double)));
    GH_CHECK(s->work2.ensure((size_t)np * np * sizeof(double)));
    GH_CHECK(inverse_lower(s, s->work.d(), s->work2.d()));
    GH_CHECK(s->v0.ensure((size_t)std::max<int64_t>(np, GH_MAX_GRAD) * sizeof(double)));
    dgrad = s->v0.d();
    ddiag = s->v1.d();
    static const uint32_t none[GH_MAX_GRAD] = {0};
    GH_CHECK(gh_launch_kgrad_reduce(k, grad ? which : none, s->x.d(), n, s->v2.d(), s->work.d(), np, dgrad, ddiag, s->scratch, st));
  }
  double host[4] = {0.0, 0.0, 0.0, 0.0};                // log-det, quadratic form, failure word (bits), forward chain's time-out flag
  int fail_b = 0;
  GH_CHECK(read_scalars(s, host, 4, st));
  if (!stepwise && want_alpha) GH_HIP(hipMemcpyAsync(&fail_b, bwd_fail(s), sizeof(int), hipMemcpyDeviceToHost, st));
  if (grad && k->size > 0) GH_CHECK(gh_from_device(grad, dgrad, (size_t)k->size, st));
  if (alpha) GH_CHECK(gh_from_device(alpha, s->v2.d(), (size_t)n, st));
  if (diagA) GH_CHECK(gh_from_device(diagA, ddiag, (size_t)n, st));
  GH_HIP(hipStreamSynchronize(st));
  GH_CHECK(gh_chol_compute_finish(s, c, host[0], info_from_bits(host[2]), logdet));
  GH_CHECK(gh_chain_timeout("objective", !stepwise && host[3] != 0.0, fail_b != 0));
  *quad = host[1];
  return GH_OK;
}

// ============================================================ cross-validation: leave-one-out, leave-group-out
// (no reference counterpart: src/george/gp.py has no cross-validation.)  With c_i = (K^-1)_ii and alpha = K^-1 r the prediction of
// y_i from all other points has residual alpha_i / c_i and variance 1 / c_i (GPML 5.4.2), and the gradient of the log
// pseudo-likelihood is sum_ij B_ij dK_ij/dtheta with B = 1/2 (v alpha^T + alpha v^T) - S S^T, S = K^-1 diag(sqrt(w)), v = K^-1 u:
// ONE triangular N^3 product for any number of parameters ("Leave-one-out cross-validation").  Leave-group-out replaces
// every c_i by the diagonal BLOCK C_gg of a group (include/george_amd.h has the formulas; DESIGN.md section 4, "Leave-group-out
// cross-validation").  Both are one sequence of steps with their own middle (loo_enqueue, lgo_enqueue; kernels: gh_cv.hip):
//   value path:    cv_alpha -> work = L^-1 -> the middle: c or C_gg, per point or per slot -> cv_fetch -> cv_finish.   K^-1 is never formed.
//   gradient path: cv_alpha -> work = K^-1 (work2 = L^-1) -> the middle, u -> cv_solve (v) -> the middle: work2 = S -> cv_contract
//                  -> cv_fetch -> cv_finish.
// Everything is enqueued on s->st; results stay on the device (s->lv, s->v0 = grad, s->v1 = diagB, s->scal[1] = sum of lpd,
// s->scal[3] != 0: a chained sweep timed out) until cv_fetch().
enum { LV_RESID = 0, LV_VAR, LV_LPD, LV_SW, LV_C, LV_ALPHA, LV_V, LV_COUNT };
static int loo_note_fail(gh_chol* s) {
  if (gh_trsv_stepwise()) return GH_OK;
  hipLaunchKernelGGL(chain_fail_note_kernel, dim3(1), dim3(64), 0, s->st, (const int*)fwd_fail(s), (const int*)bwd_fail(s), s->scal.d() + 3);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
// lv[to] = K^-1 v0 (v0 and v1 are consumed): two deferred sweeps, their time-outs noted in scal[3]
static int cv_solve(gh_chol* s, int to) {
  GH_CHECK(trsv_forward(s, s->v0.d(), s->v1.d(), true));
  GH_CHECK(trsv_backward(s, s->v1.d(), s->lv.d() + to * s->np, true));
  return loo_note_fail(s);
}
// the buffers of the sequence, scal[3] cleared, alpha = K^-1 r
static int cv_alpha(gh_chol* s, const double* r) {
  const int64_t np = s->np;
  GH_CHECK(s->lv.ensure((size_t)LV_COUNT * np * sizeof(double)));
  GH_CHECK(s->v0.ensure((size_t)std::max<int64_t>(np, GH_MAX_GRAD) * sizeof(double)));
  GH_CHECK(s->v1.ensure((size_t)np * sizeof(double)));
  GH_HIP(hipMemsetAsync(s->scal.d() + 3, 0, sizeof(double), s->st));
  GH_CHECK(load_vec(s, s->v0, r));
  return cv_solve(s, LV_ALPHA);
}
// work <- M = S S^T (lower tiles), S in work2; then the contraction: v0 = grad over `which` (NULL: no parameter), v1 = diagB
static int cv_contract(gh_chol* s, gh_kernel* k, const uint32_t* which) {
  const int64_t np = s->np;
  GhGemm g = gemm_desc(s->work.d(), np, s->work2.d(), np, true, s->work2.d(), np, true, np, np, np, 1.0, 0.0);
  g.lower = true;
  GH_CHECK(gh_launch_gemm(g, s->st));
  static const uint32_t none[GH_MAX_GRAD] = {0};
  static_assert(LV_V == LV_ALPHA + 1, "gh_launch_kgrad_reduce_loo reads v one leading dimension (np) behind alpha");
  return gh_launch_kgrad_reduce_loo(k, which ? which : none, s->x.d(), s->n, s->lv.d() + LV_ALPHA * np, s->work.d(), np,
                                    s->v0.d(), s->v1.d(), s->scratch, s->st);       // (v0, v1 are free again)
}
// the sum of the n_lpd terms of lpd, then the read-back: host <- (log-det), sum of lpd, (failure word), the chains' time-out flag, and
// the copies out (host or device destinations; lpd, grad, v, diagB may be NULL).  `host` must live until cv_finish().
static int cv_fetch(gh_chol* s, gh_kernel* k, int64_t n_lpd, double* host, double* resid, double* var, double* lpd, double* grad,
                    double* v, double* diagB) {
  const int64_t n = s->n, np = s->np;
  hipStream_t st = s->st;
  const double* lv = s->lv.d();
  GH_CHECK(launch_sum(lv + LV_LPD * np, (long)n_lpd, s->scal.d() + 1, s->scal.d() + 72, st));
  GH_CHECK(read_scalars(s, host, 4, st));
  GH_CHECK(gh_from_device(resid, lv + LV_RESID * np, (size_t)n, st));
  GH_CHECK(gh_from_device(var, lv + LV_VAR * np, (size_t)n, st));
  if (lpd) GH_CHECK(gh_from_device(lpd, lv + LV_LPD * np, (size_t)n_lpd, st));
  if (grad && k->size > 0) GH_CHECK(gh_from_device(grad, s->v0.d(), (size_t)k->size, st));
  if (v) GH_CHECK(gh_from_device(v, lv + LV_V * np, (size_t)n, st));
  if (diagB) GH_CHECK(gh_from_device(diagB, s->v1.d(), (size_t)n, st));
  return GH_OK;
}
// the call's ONE synchronisation; with `c`, the end of the compute that the call began with
static int cv_finish(gh_chol* s, const char* who, const double* host, double* lpd_sum, const ComputeCtx* c = nullptr, double* logdet = nullptr) {
  GH_HIP(hipStreamSynchronize(s->st));
  if (c) GH_CHECK(gh_chol_compute_finish(s, *c, host[0], info_from_bits(host[2]), logdet));
  GH_CHECK(gh_chain_timeout(who, host[3] != 0.0, false));
  *lpd_sum = host[1];
  return GH_OK;
}

// leave-one-out up to the contraction: c_i as the column sums of squares of L^-1, or as the diagonal of K^-1
static int loo_enqueue(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r, bool grad_path) {
  const int64_t n = s->n, np = s->np;
  hipStream_t st = s->st;
  GH_CHECK(cv_alpha(s, r));
  double* lv = s->lv.d();
  GH_CHECK(s->work.ensure((size_t)np * np * sizeof(double)));
  if (!grad_path) {
    // c_i = sum_{k >= i} (L^-1)_ki^2: the diagonal of K^-1 = L^-T L^-1 without the product
    GH_CHECK(linv_into(s, s->work.d()));
    const int64_t nchunks = std::min<int64_t>(64, np / T);
    GH_CHECK(s->scratch.ensure((size_t)nchunks * np * sizeof(double)));
    GH_CHECK(gh_launch_loo_colsumsq(s->work.d(), np, nchunks, s->scratch.d(), lv + LV_C * np, st));
    return gh_launch_loo_point(lv + LV_ALPHA * np, lv + LV_C * np, 1, n, np, lv + LV_RESID * np, nullptr, lv + LV_VAR * np,
                               lv + LV_LPD * np, lv + LV_SW * np, st);
  }
  GH_CHECK(s->work2.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(inverse_lower(s, s->work.d(), s->work2.d()));
  GH_CHECK(gh_launch_loo_point(lv + LV_ALPHA * np, s->work.d(), np + 1, n, np, lv + LV_RESID * np, s->v0.d(), lv + LV_VAR * np,
                               lv + LV_LPD * np, lv + LV_SW * np, st));
  GH_CHECK(cv_solve(s, LV_V));                                                                  // v = K^-1 u, u in v0
  GH_CHECK(gh_launch_loo_mirror_scale(s->work.d(), np, lv + LV_SW * np, s->work2.d(), st));     // work2 <- S = K^-1 diag(sqrt(w))
  return cv_contract(s, k, which);
}

extern "C" int gh_chol_loo(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r, double* lpd_sum, double* resid,
                           double* var, double* lpd, double* grad, double* v, double* diagB) {
  const bool have_args = k && r && lpd_sum && resid && var;
  GH_CHECK(enter_computed(s, k, have_args && !(grad && !which),
                          have_args ? "loo: gradient requested without a parameter mask" : "bad argument to loo"));
  GH_CHECK(loo_enqueue(s, k, grad ? which : nullptr, r, grad || v || diagB));
  double host[4] = {0.0, 0.0, 0.0, 0.0};
  GH_CHECK(cv_fetch(s, k, s->n, host, resid, var, lpd, grad, v, diagB));
  return cv_finish(s, "loo", host, lpd_sum);
}

// build K -> factor -> log-det -> the sequence of gh_chol_loo, ONE synchronisation: the analogue of gh_chol_objective for the
// leave-one-out objective.  The same launches as gh_chol_compute followed by gh_chol_loo: the same bits.
extern "C" int gh_chol_loo_objective(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                                     const double* r, const uint32_t* which, double* logdet, double* lpd_sum,
                                     double* resid, double* var, double* grad, double* v, double* diagB) {
  if (!r || !logdet || !lpd_sum || !resid || !var) { gh_set_error("bad argument to loo_objective"); return GH_ERR_BAD_ARG; }
  if (grad && !which) { gh_set_error("loo_objective: gradient requested without a parameter mask"); return GH_ERR_BAD_ARG; }
  ComputeCtx c;
  GH_CHECK(gh_chol_compute_enqueue(s, k, x, n, ndim, yerr, c));
  GH_CHECK(join_tail(s));
  GH_CHECK(loo_enqueue(s, k, grad ? which : nullptr, r, grad || v || diagB));
  double host[4] = {0.0, 0.0, 0.0, 0.0};
  GH_CHECK(cv_fetch(s, k, s->n, host, resid, var, nullptr, grad, v, diagB));
  return cv_finish(s, "loo_objective", host, lpd_sum, &c, logdet);
}

// ---- leave-group-out: the groups are packed into slots of 128 permuted positions, every slot one block-diagonal, identity-padded
// 128 x 128 matrix for the batched Cholesky.
//   value path:    the slots' Gram matrices of L^-1 -> R = chol, R^-1 -> slot kernel.
//   gradient path: the slots' matrices gathered from K^-1 -> R, R^-1 -> slot kernel (+ W) -> v -> T = chol(W) -> S = K^-1[:, J] T.
// s->lgo, in doubles: Cs | Ri | X (the Gram partials, or W) | cov | the failure word | the tables.  s->lv holds resid and var by
// point, lpd by group.
struct LgoPlan {
  std::vector<int> idx, grp, minj, pos0;
  std::vector<long long> start, covoff;
  int nslots = 0;
};
// nullptr, or what is wrong with the grouping
static const char* lgo_check_groups(int64_t n, const int64_t* order, const int64_t* start, int64_t ngroups) {
  if (ngroups < 1 || ngroups > n) return "lgo: the number of groups must be between 1 and n";
  if (start[0] != 0 || start[ngroups] != n) return "lgo: start must rise from 0 to n";
  for (int64_t g = 0; g < ngroups; ++g) {
    if (start[g + 1] < start[g] || start[g + 1] > n) return "lgo: start must rise from 0 to n";
    if (start[g + 1] == start[g]) return "lgo: a group is empty";
    if (start[g + 1] - start[g] > GH_LGO_SLOT) return "lgo: a group has more than 128 points";
  }
  std::vector<char> seen((size_t)n, 0);
  for (int64_t p = 0; p < n; ++p) {
    if (order[p] < 0 || order[p] >= n || seen[(size_t)order[p]]) return "lgo: order is not a permutation of 0 .. n-1";
    seen[(size_t)order[p]] = 1;
  }
  return nullptr;
}
// consecutive groups share a slot while they fit: at most 2 ceil(n / 128) + 1 slots
static void lgo_plan(int64_t n, const int64_t* order, const int64_t* start, int64_t ngroups, LgoPlan& p) {
  p.start.assign(start, start + ngroups + 1);
  p.covoff.assign((size_t)ngroups + 1, 0);
  int64_t used = GH_LGO_SLOT;                      // of the current slot (none yet)
  for (int64_t g = 0; g < ngroups; ++g) {
    const int64_t m = start[g + 1] - start[g];
    p.covoff[(size_t)g + 1] = p.covoff[(size_t)g] + m * m;
    if (used + m > GH_LGO_SLOT) {
      p.idx.resize(p.idx.size() + GH_LGO_SLOT, -1);
      p.grp.resize(p.grp.size() + GH_LGO_SLOT, -1);
      p.pos0.push_back((int)start[g]);
      p.minj.push_back((int)n);
      used = 0;
    }
    const size_t at = p.idx.size() - GH_LGO_SLOT + (size_t)used;
    for (int64_t q = 0; q < m; ++q) {
      p.idx[at + (size_t)q] = (int)order[start[g] + q];
      p.grp[at + (size_t)q] = (int)g;
      p.minj.back() = std::min(p.minj.back(), (int)order[start[g] + q]);
    }
    used += m;
  }
  p.nslots = (int)p.pos0.size();
}

// what gh_chol_lgo reads back beside the outputs of cv_fetch()
struct LgoOut { const long long* info = nullptr; const double* cov = nullptr; int64_t ncov = 0; };
// leave-group-out up to the contraction.  The tables go up before anything else.
static int lgo_enqueue(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r, const int64_t* order, const int64_t* start,
                       int64_t ngroups, bool want_cov, bool grad_path, LgoOut& out) {
  const int64_t n = s->n, np = s->np, SS = (int64_t)GH_LGO_SLOT * GH_LGO_SLOT;
  hipStream_t st = s->st;
  LgoPlan plan;
  lgo_plan(n, order, start, ngroups, plan);
  const int64_t ns = plan.nslots, ncov = want_cov ? plan.covoff[(size_t)ngroups] : 0;
  int64_t rows_per = 0;
  const int64_t nx = grad_path ? 1 : gh_lgo_gram_chunks(n, plan.nslots, &rows_per);
  // the layout of s->lgo
  const int64_t o_cs = 0, o_ri = o_cs + ns * SS, o_x = o_ri + ns * SS, o_cov = o_x + nx * ns * SS, o_info = o_cov + gh_round_up(ncov, 2);
  const int64_t o_ll = o_info + 2, o_int = o_ll + 2 * (ngroups + 1);
  const size_t n_int = (size_t)(2 * ns * GH_LGO_SLOT + 2 * ns);
  GH_CHECK(s->lgo.ensure((size_t)o_int * sizeof(double) + n_int * sizeof(int)));
  double* base = s->lgo.d();
  long long* d_info = (long long*)(base + o_info);
  long long* d_ll = (long long*)(base + o_ll);
  int* d_int = (int*)(base + o_int);
  GH_HIP(hipMemsetAsync(d_info, 0, sizeof(long long), st));
  GH_HIP(hipMemcpyAsync(d_ll, plan.start.data(), (size_t)(ngroups + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemcpyAsync(d_ll + ngroups + 1, plan.covoff.data(), (size_t)(ngroups + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemcpyAsync(d_int, plan.idx.data(), (size_t)ns * GH_LGO_SLOT * sizeof(int), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemcpyAsync(d_int + ns * GH_LGO_SLOT, plan.grp.data(), (size_t)ns * GH_LGO_SLOT * sizeof(int), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemcpyAsync(d_int + 2 * ns * GH_LGO_SLOT, plan.minj.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemcpyAsync(d_int + 2 * ns * GH_LGO_SLOT + ns, plan.pos0.data(), (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
  GhLgoSlots t;
  t.idx = d_int; t.grp = d_int + ns * GH_LGO_SLOT; t.minj = d_int + 2 * ns * GH_LGO_SLOT; t.pos0 = t.minj + ns;
  t.start = d_ll; t.covoff = d_ll + ngroups + 1; t.nslots = plan.nslots;
  double* Cs = base + o_cs;
  double* Ri = base + o_ri;
  double* X = base + o_x;
  double* dcov = want_cov ? base + o_cov : nullptr;
  out.info = d_info; out.cov = dcov; out.ncov = ncov;

  GH_CHECK(cv_alpha(s, r));
  double* lv = s->lv.d();
  GH_CHECK(s->work.ensure((size_t)np * np * sizeof(double)));
  if (!grad_path) {
    GH_CHECK(linv_into(s, s->work.d()));
    GH_CHECK(gh_launch_lgo_gram(s->work.d(), np, n, t, X, Cs, st));
  } else {
    GH_CHECK(s->work2.ensure((size_t)np * np * sizeof(double)));
    GH_CHECK(inverse_lower(s, s->work.d(), s->work2.d()));
    GH_CHECK(gh_launch_lgo_gather(s->work.d(), np, t, Cs, st));
    GH_HIP(hipMemsetAsync(s->v0.d(), 0, (size_t)np * sizeof(double), st));       // u by point, zero in the padding
  }
  GH_CHECK(gh_launch_potf2_batched(Cs, GH_LGO_SLOT, SS, Ri, SS, d_info, plan.nslots, st));
  GH_CHECK(gh_launch_lgo_slots(Cs, Ri, t, lv + LV_ALPHA * np, lv + LV_RESID * np, lv + LV_VAR * np, grad_path ? s->v0.d() : nullptr,
                               lv + LV_LPD * np, dcov, grad_path ? X : nullptr, st));
  if (!grad_path) return GH_OK;
  GH_CHECK(cv_solve(s, LV_V));                                                                  // v = K^-1 u, u in v0
  // X <- T = chol(W) (its inverse, into Ri, is not used); work2 <- S = K^-1[:, J] T
  GH_CHECK(gh_launch_potf2_batched(X, GH_LGO_SLOT, SS, Ri, SS, d_info, plan.nslots, st));
  GH_CHECK(gh_launch_lgo_block_scale(s->work.d(), np, n, t, X, s->work2.d(), st));
  return cv_contract(s, k, which);
}

extern "C" int gh_chol_lgo(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r, const int64_t* order, const int64_t* start,
                           int64_t ngroups, double* lpd_sum, double* resid, double* var, double* lpd, double* cov, double* grad,
                           double* v, double* diagB) {
  const bool have_args = k && r && order && start && lpd_sum && resid && var;
  const char* bad = !have_args ? "bad argument to lgo" : (grad && !which) ? "lgo: gradient requested without a parameter mask" : nullptr;
  if (!bad && s && s->computed) bad = lgo_check_groups(s->n, order, start, ngroups);
  GH_CHECK(enter_computed(s, k, !bad, bad ? bad : ""));
  LgoOut o;
  GH_CHECK(lgo_enqueue(s, k, grad ? which : nullptr, r, order, start, ngroups, cov != nullptr, grad || v || diagB, o));
  double host[4] = {0.0, 0.0, 0.0, 0.0}, sum = 0.0;
  long long slot_info = 0;
  GH_CHECK(cv_fetch(s, k, ngroups, host, resid, var, lpd, grad, v, diagB));
  GH_HIP(hipMemcpyAsync(&slot_info, o.info, sizeof(long long), hipMemcpyDeviceToHost, s->st));
  if (cov) GH_CHECK(gh_from_device(cov, o.cov, (size_t)o.ncov, s->st));
  GH_CHECK(cv_finish(s, "lgo", host, &sum));
  if (slot_info != 0) { gh_set_error("lgo: a group's block of K^-1 is not positive definite"); return GH_ERR_NOT_PD; }
  *lpd_sum = sum;
  return GH_OK;
}
