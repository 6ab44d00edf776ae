// gh_cv.hip -- the device pieces of cross-validation: gh_chol_loo, gh_chol_loo_objective and gh_chol_lgo (gh_chol_solve.hip).
// Leave-one-out, from c_i = (K^-1)_ii:
//   colsumsq_kernel         value path: c as the column sums of squares of L^-1, per row chunk
//   colsumsq_final_kernel   ... the chunks added in index order
//   loo_point_kernel        resid, var, lpd, sqrt(w) (and u) per point from alpha and c
//   loo_mirror_scale_kernel gradient path: S = K^-1 diag(sqrt(w)), full, from the lower triangle of K^-1
// Leave-group-out: every c_i becomes the diagonal block C_gg of a group.  The groups are packed into "slots" of at most 128 permuted
// positions (whole groups only); every slot is one identity-padded, block-diagonal 128 x 128 matrix C_slot of K^-1 entries that the
// batched Cholesky of gh_potf2.hip factors and inverts.
//   lgo_gram_kernel         value path: per slot and row chunk, sum_k L^-1[k][J_a] L^-1[k][J_b] on the fp64 matrix pipe
//   lgo_gram_final_kernel   ... the chunks added in index order, cross-group entries masked, identity padding
//   lgo_gather_kernel       gradient path: C_slot read straight from the lower triangle of K^-1
//   lgo_slot_kernel         one workgroup per slot: u, var, lpd (and cov, W = 1/2 (C^-1 + u u^T)) from R = chol(C_slot), R^-1
//   lgo_block_scale_kernel  S[:, p] = sum_q K^-1[:, J_q] T[q][p]: loo_mirror_scale_kernel with a block-diagonal right factor
// No atomics anywhere: two calls give the same bits.  Rows i >= n of the padded matrices are never added to anything.
// DESIGN.md section 4, "Leave-one-out cross-validation" and "Leave-group-out cross-validation".
#include <algorithm>
#include "gh_common.h"
#include "gh_device_util.h"

// ================================================= leave-one-out
#define LT 64                 // tile edge of the leave-one-out kernels
// Column sums of squares of a LOWER-triangular row-major matrix (L^-1): part[s][c] = sum over the rows r >= c of the s-th row
// chunk of V[r][c]^2.  A workgroup takes 64 columns of one chunk, a wavefront every fourth row: each load instruction reads
// 512 contiguous bytes, four rows are in flight per trip.  Rows above the tile's first column hold zeros and are not read.
// The four wavefronts' sums meet in LDS in a fixed order; colsumsq_final_kernel adds the chunks in index order: no atomics,
// bitwise reproducible.
__global__ __launch_bounds__(256) void colsumsq_kernel(const double* V, long ld, long np, long rows_per, double* part) {
  __shared__ double sh[4][LT];
  const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
  const long c0 = (long)blockIdx.x * LT, c = c0 + lc;
  long r0 = (long)blockIdx.y * rows_per;
  const long r1 = r0 + rows_per < np ? r0 + rows_per : np;
  if (r0 < c0) r0 = c0;
  double acc = 0.0;
  long r = r0 + lr;
  for (; r + 12 < r1; r += 16) {
    double a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = V[(r + 4 * q) * ld + c];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc += (r + 4 * q >= c) ? a[q] * a[q] : 0.0;
  }
  for (; r < r1; r += 4) {
    const double a = V[r * ld + c];
    acc += (r >= c) ? a * a : 0.0;
  }
  sh[lr][lc] = acc;
  __syncthreads();
  if (lr == 0) part[(long)blockIdx.y * np + c] = (sh[0][lc] + sh[1][lc]) + (sh[2][lc] + sh[3][lc]);
}
__global__ void colsumsq_final_kernel(const double* part, long nchunks, long np, double* c) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double v = 0.0;
  for (long s = 0; s < nchunks; ++s) v += part[s * np + i];
  c[i] = v;
}
// The per-point quantities from alpha and c_i = (K^-1)_ii (c[i * cstride]: a vector, or the diagonal of a matrix):
//   resid = u = alpha / c,  var = 1 / c,  lpd = 1/2 log c - 1/2 alpha^2 / c - 1/2 log 2 pi,  sw = sqrt(w),  w = 1/2 (1 + alpha^2 / c) / c.
// Padded rows i >= n get zeros everywhere: nothing of them reaches the sum of lpd or S = K^-1 diag(sqrt(w)).
// `u` is a second copy of resid that the solve for v = K^-1 u consumes.
__global__ void loo_point_kernel(const double* alpha, const double* c, long cstride, long n, long np,
                                 double* resid, double* u, double* var, double* lpd, double* sw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  double ui = 0.0, vi = 0.0, li = 0.0, si = 0.0;
  if (i < n) {
    const double ci = c[i * cstride], a = alpha[i];
    ui = a / ci;
    vi = 1.0 / ci;
    const double q = a * ui;
    li = 0.5 * log(ci) - 0.5 * q - 0.91893853320467274178;
    si = sqrt(0.5 * (1.0 + q) / ci);
  }
  resid[i] = ui;
  if (u) u[i] = ui;
  var[i] = vi;
  lpd[i] = li;
  sw[i] = si;
}
// S = Kinv diag(sw) as a FULL matrix from the lower triangle of Kinv, one pass: a workgroup reads the 64 x 64 tile (ti, tj),
// tj <= ti, into LDS and writes tile (ti, tj) of S as it lies and tile (tj, ti) transposed, column k scaled by sw[k].  Reads and
// both writes are coalesced (a row of 64 doubles per wavefront); the transposed LDS reads walk a pitch of 65: no bank conflicts.
__global__ __launch_bounds__(256) void loo_mirror_scale_kernel(const double* W, long ld, const double* sw, double* S) {
  __shared__ double t[LT][LT + 1];
  int ti, tj;
  tri_index(blockIdx.x, ti, tj);
  const long r0 = (long)ti * LT, c0 = (long)tj * LT;
  const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
#pragma unroll 4
  for (int rr = lr; rr < LT; rr += 4) t[rr][lc] = W[(r0 + rr) * ld + c0 + lc];
  __syncthreads();
  const double sc = sw[c0 + lc];
  if (ti != tj) {
    const double sr = sw[r0 + lc];
#pragma unroll 4
    for (int rr = lr; rr < LT; rr += 4) {
      S[(r0 + rr) * ld + c0 + lc] = t[rr][lc] * sc;
      S[(c0 + rr) * ld + r0 + lc] = t[lc][rr] * sr;
    }
  } else {
#pragma unroll 4
    for (int rr = lr; rr < LT; rr += 4) S[(r0 + rr) * ld + c0 + lc] = (lc <= rr ? t[rr][lc] : t[lc][rr]) * sc;
  }
}

int gh_launch_loo_colsumsq(const double* Linv, int64_t np, int64_t nchunks, double* part, double* c, hipStream_t st) {
  const int64_t rows_per = (np + nchunks - 1) / nchunks;
  hipLaunchKernelGGL(colsumsq_kernel, dim3((unsigned)(np / LT), (unsigned)nchunks), dim3(256), 0, st,
                     Linv, (long)np, (long)np, (long)rows_per, part);
  hipLaunchKernelGGL(colsumsq_final_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, (const double*)part, (long)nchunks,
                     (long)np, c);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_loo_point(const double* alpha, const double* c, int64_t cstride, int64_t n, int64_t np, double* resid, double* u,
                        double* var, double* lpd, double* sw, hipStream_t st) {
  hipLaunchKernelGGL(loo_point_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, st, alpha, c, (long)cstride, (long)n, (long)np,
                     resid, u, var, lpd, sw);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_loo_mirror_scale(const double* W, int64_t np, const double* sw, double* S, hipStream_t st) {
  const long tm = (long)(np / LT);
  hipLaunchKernelGGL(loo_mirror_scale_kernel, dim3((unsigned)(tm * (tm + 1) / 2)), dim3(256), 0, st, W, (long)np, sw, S);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// ================================================= leave-group-out
namespace {
constexpr int LG = GH_LGO_SLOT;                   // slot edge = the tile of the batched Cholesky
constexpr int GK = 16;                            // rows of L^-1 per step of the Gram kernel
constexpr int GPITCH = LG + 16;                     // LDS pitch of a step: rows k and k + 1 of a fragment read lie 32 banks apart
constexpr int SR = 32;                            // rows of K^-1 per workgroup of the block scale
typedef double v4d __attribute__((ext_vector_type(4)));

// Workgroup (slot, chunk): the 128 x 128 Gram matrix of the slot's gathered columns over the chunk's rows.  A step stages 16 rows
// x 128 gathered columns in LDS (a contiguous group reads contiguous memory); wavefront w owns the tile rows 2w, 2w + 1 and all 8
// tile columns: 16 accumulators, 2 + 8 fragment reads for 16 matrix instructions.  Rows before the slot's smallest column hold
// zeros (L^-1 is lower triangular) and are skipped; rows >= n are not read.
__global__ __launch_bounds__(256) void lgo_gram_kernel(const double* __restrict__ Linv, long ld, long n, GhLgoSlots t, long rows_per,
                                                       double* __restrict__ part) {
  __shared__ double sh[GK][GPITCH];
  const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int col = tid & (LG - 1), rsel = tid >> 7;
  const long j = t.idx[slot * LG + col];
  long k0 = (long)blockIdx.y * rows_per;
  const long k1 = k0 + rows_per < n ? k0 + rows_per : n;
  const long kmin = (long)(t.minj[slot] / GK) * GK;
  if (k0 < kmin) k0 = kmin;
  v4d acc[2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = v4d{0.0, 0.0, 0.0, 0.0};
  for (; k0 < k1; k0 += GK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GK / 2; ++q) {
      const long k = k0 + rsel + 2 * q;
      sh[rsel + 2 * q][col] = (j >= 0 && k < k1) ? Linv[k * ld + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GK / 4; ++kk) {
      double a[2], b[8];
#pragma unroll
      for (int x = 0; x < 2; ++x) a[x] = sh[4 * kk + fq][16 * (2 * wave + x) + fr];
#pragma unroll
      for (int y = 0; y < 8; ++y) b[y] = sh[4 * kk + fq][16 * y + fr];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
    }
  }
  double* out = part + ((long)blockIdx.y * t.nslots + slot) * (LG * LG);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * (2 * wave + x) + fq + 4 * r) * LG + 16 * y + fr] = acc[x][y][r];
}

// what a slot matrix holds where it holds no entry of a group: the identity
__device__ __forceinline__ bool lgo_same_group(const GhLgoSlots& t, int slot, int a, int b) {
  const int ga = t.grp[slot * LG + a];
  return ga >= 0 && ga == t.grp[slot * LG + b];
}
__global__ __launch_bounds__(256) void lgo_gram_final_kernel(const double* __restrict__ part, long nchunks, GhLgoSlots t,
                                                             double* __restrict__ Cs) {
  const int slot = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x, a = e / LG, b = e % LG;
  double v = (a == b) ? 1.0 : 0.0;
  if (lgo_same_group(t, slot, a, b)) {
    v = 0.0;
    for (long c = 0; c < nchunks; ++c) v += part[(c * t.nslots + slot) * (LG * LG) + e];
  }
  Cs[(long)slot * (LG * LG) + e] = v;
}
// element (J_a, J_b) of the symmetric K^-1 is read from its lower triangle at (max, min)
__global__ __launch_bounds__(256) void lgo_gather_kernel(const double* __restrict__ Kinv, long ld, GhLgoSlots t, double* __restrict__ Cs) {
  const int slot = blockIdx.x, e = blockIdx.y * 256 + threadIdx.x, a = e / LG, b = e % LG;
  double v = (a == b) ? 1.0 : 0.0;
  if (lgo_same_group(t, slot, a, b)) {
    const long ja = t.idx[slot * LG + a], jb = t.idx[slot * LG + b];
    v = ja >= jb ? Kinv[ja * ld + jb] : Kinv[jb * ld + ja];
  }
  Cs[(long)slot * (LG * LG) + e] = v;
}

// One workgroup per slot, from R = chol(C_slot) (its diagonal) and Ri = R^-1 (lower, zeros above; block diagonal like C_slot):
//   tt = Ri alpha_J,  u = Ri^T tt = C_slot^-1 alpha_J,  var_a = sum_k Ri[k][a]^2 = (C_slot^-1)_aa,
//   lpd_g = sum_{a in g} (log R_aa - 1/2 alpha_a u_a - 1/2 log 2 pi), added by the group's first thread in position order,
// scattered to the caller's point order (resid, var, u_pt) and group order (lpd).  With cov or Ws also
//   cov[a][b] = sum_{k >= max(a, b)} Ri[k][a] Ri[k][b]   (group blocks, row-major, at covoff[g])
//   Ws = 1/2 (cov + u u^T) inside a group, the identity elsewhere: block-diagonal SPD for the second factorisation.
__global__ __launch_bounds__(256) void lgo_slot_kernel(const double* __restrict__ R, const double* __restrict__ Rinv, GhLgoSlots t,
                                                       const double* __restrict__ alpha, double* __restrict__ resid,
                                                       double* __restrict__ var, double* __restrict__ u_pt, double* __restrict__ lpd,
                                                       double* __restrict__ cov, double* __restrict__ Ws) {
  __shared__ double a_s[LG], t_s[LG], u_s[LG], e_s[LG];
  __shared__ int j_s[LG], g_s[LG];
  const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* Ri = Rinv + (long)slot * (LG * LG);
  const double* Rc = R + (long)slot * (LG * LG);
  if (tid < LG) {
    const int j = t.idx[slot * LG + tid];
    j_s[tid] = j;
    g_s[tid] = t.grp[slot * LG + tid];
    a_s[tid] = j >= 0 ? alpha[j] : 0.0;
  }
  __syncthreads();
  for (int a = wave; a < LG; a += 4) {
    double v = 0.0;
    for (int b = lane; b <= a; b += 64) v += Ri[a * LG + b] * a_s[b];
    v = wave_sum(v);
    if (lane == 0) t_s[a] = v;
  }
  __syncthreads();
  if (tid < LG) {
    double uu = 0.0, vv = 0.0;
    for (int b = tid; b < LG; ++b) {
      const double x = Ri[b * LG + tid];
      uu += x * t_s[b];
      vv += x * x;
    }
    u_s[tid] = uu;
    e_s[tid] = 0.0;
    const int j = j_s[tid];
    if (j >= 0) {
      resid[j] = uu;
      var[j] = vv;
      if (u_pt) u_pt[j] = uu;
      e_s[tid] = log(Rc[tid * (LG + 1)]) - 0.5 * a_s[tid] * uu - 0.91893853320467274178;
    }
  }
  __syncthreads();
  if (tid < LG && g_s[tid] >= 0 && (tid == 0 || g_s[tid - 1] != g_s[tid])) {
    double sum = 0.0;
    for (int b = tid; b < LG && g_s[b] == g_s[tid]; ++b) sum += e_s[b];
    lpd[g_s[tid]] = sum;
  }
  if (!cov && !Ws) return;
  const int b = tid & (LG - 1), gb = g_s[b];
  const long pos0 = t.pos0[slot];
  for (int a = tid >> 7; a < LG; a += 2) {
    const bool same = gb >= 0 && gb == g_s[a];
    double c = 0.0;
    if (same)
      for (int k = a > b ? a : b; k < LG; ++k) c += Ri[k * LG + a] * Ri[k * LG + b];
    if (Ws) Ws[(long)slot * (LG * LG) + a * LG + b] = same ? 0.5 * (c + u_s[a] * u_s[b]) : (a == b ? 1.0 : 0.0);
    if (cov && same) {
      const long g0 = t.start[gb], m = t.start[gb + 1] - g0;
      cov[t.covoff[gb] + (pos0 + a - g0) * m + (pos0 + b - g0)] = c;
    }
  }
}

// Workgroup (slot, 32 rows): the rows' gathered entries K^-1[i][J_q] (mirror-aware: the lower triangle holds them at (max, min); rows
// i >= n are taken as zero) go to LDS, thread (p, half) accumulates 16 rows of column p over q against T[q][p], T = chol(W_slot)
// with zeros above its diagonal and between groups.  Only a slot's real columns are written, at their permuted position: S has n
// columns in group-sorted order.
__global__ __launch_bounds__(256) void lgo_block_scale_kernel(const double* __restrict__ Kinv, long ld, long n, GhLgoSlots t,
                                                              const double* __restrict__ Tm, double* __restrict__ S) {
  __shared__ double cg[SR][LG + 1];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const long i0 = (long)blockIdx.y * SR;
  for (int e = tid; e < SR * LG; e += 256) {
    const int r = e / LG, q = e % LG;
    const long i = i0 + r, j = t.idx[slot * LG + q];
    cg[r][q] = (j >= 0 && i < n) ? (i >= j ? Kinv[i * ld + j] : Kinv[j * ld + i]) : 0.0;
  }
  __syncthreads();
  const int p = tid & (LG - 1), half = tid >> 7;
  if (t.idx[slot * LG + p] < 0) return;
  const double* Tp = Tm + (long)slot * (LG * LG) + p;
  double acc[SR / 2];
#pragma unroll
  for (int r = 0; r < SR / 2; ++r) acc[r] = 0.0;
  for (int q = 0; q < LG; ++q) {
    const double tq = Tp[q * LG];
#pragma unroll
    for (int r = 0; r < SR / 2; ++r) acc[r] += cg[half + 2 * r][q] * tq;
  }
  const long pos = t.pos0[slot] + p;
#pragma unroll
  for (int r = 0; r < SR / 2; ++r) S[(i0 + half + 2 * r) * ld + pos] = acc[r];
}
}  // namespace

int gh_lgo_gram_chunks(int64_t n, int nslots, int64_t* rows_per) {
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(16, 512 / std::max(1, nslots)));
  *rows_per = gh_round_up((n + want - 1) / want, GK);
  return (int)((n + *rows_per - 1) / *rows_per);
}
int gh_launch_lgo_gram(const double* Linv, int64_t np, int64_t n, const GhLgoSlots& t, double* part, double* Cs, hipStream_t st) {
  int64_t rows_per = 0;
  const int nchunks = gh_lgo_gram_chunks(n, t.nslots, &rows_per);
  hipLaunchKernelGGL(lgo_gram_kernel, dim3((unsigned)t.nslots, (unsigned)nchunks), dim3(256), 0, st, Linv, (long)np, (long)n, t,
                     (long)rows_per, part);
  hipLaunchKernelGGL(lgo_gram_final_kernel, dim3((unsigned)t.nslots, LG * LG / 256), dim3(256), 0, st, (const double*)part,
                     (long)nchunks, t, Cs);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_lgo_gather(const double* Kinv, int64_t np, const GhLgoSlots& t, double* Cs, hipStream_t st) {
  hipLaunchKernelGGL(lgo_gather_kernel, dim3((unsigned)t.nslots, LG * LG / 256), dim3(256), 0, st, Kinv, (long)np, t, Cs);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_lgo_slots(const double* R, const double* Rinv, const GhLgoSlots& t, const double* alpha, double* resid, double* var,
                        double* u_pt, double* lpd, double* cov, double* Ws, hipStream_t st) {
  hipLaunchKernelGGL(lgo_slot_kernel, dim3((unsigned)t.nslots), dim3(256), 0, st, R, Rinv, t, alpha, resid, var, u_pt, lpd, cov, Ws);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
int gh_launch_lgo_block_scale(const double* Kinv, int64_t np, int64_t n, const GhLgoSlots& t, const double* Tm, double* S,
                              hipStream_t st) {
  if (np > n) GH_HIP(hipMemset2DAsync(S + n, (size_t)np * sizeof(double), 0, (size_t)(np - n) * sizeof(double), (size_t)np, st));
  hipLaunchKernelGGL(lgo_block_scale_kernel, dim3((unsigned)t.nslots, (unsigned)(np / SR)), dim3(256), 0, st, Kinv, (long)np, (long)n,
                     t, Tm, S);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
