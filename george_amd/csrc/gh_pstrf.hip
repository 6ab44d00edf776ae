// gh_pstrf.hip -- diagonally pivoted Cholesky with rank truncation (LAPACK dpstrf's job), batched, and the draws behind it.
//
// Why: a predictive covariance K** - K* K^-1 K*^T is numerically SEMIdefinite (smallest eigenvalue around -1e-14 at the
// hyper.rst shape), so a plain Cholesky fails on it and the reference samples through an SVD on the host
// (utils.py:11-33, np.random.multivariate_normal).  The factor below needs no positive definiteness: it stops at the
// numerical rank.  DESIGN.md section 4, "Sampling".
//
// Definition (george_amd.utils.pivoted_cholesky is the same, line for line, in NumPy).  No physical swaps:
//   d = diag(A); every index free; rank = 0
//   for j = 0 .. m-1:
//     p = the free index with the largest d (ties: the lowest index);   stop unless d[p] > tol
//     c = A[p, :] - L[:, :j] L[p, :j]                                   (A is symmetric: row p is its column p, contiguous)
//     stop unless c[p] > 0 and finite;   c[i] = 0 exactly for every i no longer free
//     L[p, j] = sqrt(c[p]);  L[i, j] = c[i] / sqrt(c[p]) for free i != p
//     d -= L[:, j]^2;  p leaves the free set;  piv[j] = p;  rank = j + 1
// L L^T approximates A directly (L is lower triangular in PIVOT order: L[piv[i], j] == 0 exactly for i < j), columns >= rank
// are exactly zero, and every entry of A - L L^T is at most tol in exact arithmetic.
//
// Schedule.  One 512-thread workgroup per member; thread t owns rows t, t + 512, ... (its d entries never leave it); the
// factor's columns are kept column-major in a work array (P[k][i]: the left-looking dot products read it coalesced) and
// written to the caller's row-major L as they are made.  Steps are ordered by barriers inside the workgroup and by launches
// on the caller's stream: no inter-workgroup waits.
//   * m <= GH_PSTRF_WHOLE (512): the whole member in ONE launch for the whole batch, d in LDS, left-looking over all earlier
//     columns, A read in place -- m^2 rank / 2 multiply-adds, and rank is a few tens for a predictive covariance.
//   * larger m: pivots in panels of 128.  A is copied into a work matrix padded to the 128-tile; inside a panel the pivot row
//     needs only the panel's own columns, because after each FULL panel the Schur complement is updated in place on the
//     matrix pipe, W -= P_panel P_panel^T (gh_launch_gemm, K = 128, both operands column-major).  After each panel the host
//     reads the members' (rank, stopped) words -- one small copy and one synchronisation per 128 pivots -- and skips the GEMM
//     of a member that has stopped: a rank-33 covariance of any size costs one panel launch.
// Two calls give the same bits: every sum runs in a fixed order.
#include <math.h>
#include <algorithm>
#include <limits.h>
#include <string.h>
#include "gh_common.h"

#define GH_PSTRF_WHOLE 512       // largest m factored by one launch
#define GH_PSTRF_PANEL 128       // pivots per launch above it
#define PT 512                   // threads of the factor workgroup
static constexpr int T = GH_TILE;
static constexpr double GH_EPS = 2.220446049250313e-16;

struct PstrfArgs {
  const double* A; long lda, stride_a;    // pivot rows are read from here (the caller's A, or the padded work matrix)
  long m;
  double* P; long pitch, pstride;         // factor columns, column-major: column j - (first column kept) at P + (...) * pitch
  double* d; long dstride;                // panel form: the running diagonal (-inf: no longer free)
  double* L; long ldl, stride_l;
  long long* piv; long long* rank; double* resid;
  long long* state;                       // per member: [0] rank so far (-1: non-finite diagonal), [1] stopped, [2] tol (bits)
  double tol; const double* tol_dev;      // tol_dev (per member) is used in place of tol when given; < 0: m eps max(d_0, 0)
};

// the larger value wins; of equal values the lower index
__device__ __forceinline__ void amax_take(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// (value, index) of the largest entry over the workgroup, every thread gets it.  sv / si: PT / 64 words each; a barrier
// separates the last reads of one call from the writes of the next (the callers' own barriers in between).
__device__ __forceinline__ void block_amax(double& v, int& i, double* sv, int* si) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(v, off, 64);
    const int oi = __shfl_down(i, off, 64);
    amax_take(v, i, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = sv[0]; i = si[0];
#pragma unroll
  for (int w = 1; w < PT / 64; ++w) amax_take(v, i, sv[w], si[w]);
}

// Pivots j0 .. j1 - 1 of every member (blockIdx.x).  WHOLE: j0 == 0, j1 == m <= GH_PSTRF_WHOLE, d in LDS, the dot products
// run over all earlier columns.  Otherwise one panel (j1 - j0 <= 128): A has had the earlier panels' update, the dot products
// run over the panel's own columns, d and the (rank, stopped, tol) words live in global memory between the launches.
template <bool WHOLE>
__global__ __launch_bounds__(PT) void pstrf_kernel(PstrfArgs a, int j0, int j1) {
  __shared__ double s_row[WHOLE ? GH_PSTRF_WHOLE : GH_PSTRF_PANEL];      // L[p, kb : j]
  __shared__ double s_d[WHOLE ? GH_PSTRF_WHOLE : 1];
  __shared__ double s_rv[PT / 64];
  __shared__ int s_ri[PT / 64];
  __shared__ double s_cpp;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long m = a.m, pitch = a.pitch;
  const double* A = a.A + (long)b * a.stride_a;
  double* P = a.P + (long)b * a.pstride;
  double* L = a.L + (long)b * a.stride_l;
  double* d = WHOLE ? s_d : a.d + (long)b * a.dstride;
  long long* piv = a.piv + (long)b * m;
  long long* state = a.state + 4L * b;
  const double ninf = -INFINITY;
  double tol;
  long rank;
  bool stopped = false;
  if (j0 == 0) {
    int bad = 0;
    double bv = ninf; int bi = INT_MAX;
    for (long i = tid; i < m; i += PT) {
      const double v = A[i * a.lda + i];
      d[i] = v;
      if (!isfinite(v)) bad = 1;
      if (v > bv) { bv = v; bi = (int)i; }
    }
    bad = __syncthreads_or(bad);
    if (bad) {                                     // a non-finite diagonal: rank -1, NaN in L
      const double qnan = __longlong_as_double(0x7FF8000000000000LL);
      for (long e = tid; e < m * m; e += PT) L[(e / m) * a.ldl + e % m] = qnan;
      if (tid == 0) {
        state[0] = -1; state[1] = 1; state[2] = 0;
        a.rank[b] = -1;
        if (a.resid) a.resid[b] = qnan;
      }
      return;
    }
    block_amax(bv, bi, s_rv, s_ri);
    tol = a.tol_dev ? a.tol_dev[b] : a.tol;
    if (tol < 0.0) tol = ((double)m * GH_EPS) * fmax(bv, 0.0);
    rank = 0;
    if (tid == 0) state[2] = __double_as_longlong(tol);
    __syncthreads();                               // (s_rv / s_ri are written again below)
  } else {
    rank = (long)state[0];
    if (state[1]) return;                          // (the same word for every thread)
    tol = __longlong_as_double(state[2]);
  }
  const int kb = WHOLE ? 0 : j0;                   // first column the dot products see
  for (int j = j0; j < j1; ++j) {
    double bv = ninf; int bi = INT_MAX;
    for (long i = tid; i < m; i += PT) {           // (ascending, strict: the lowest index of a thread's largest)
      const double v = d[i];
      if (v > bv) { bv = v; bi = (int)i; }
    }
    block_amax(bv, bi, s_rv, s_ri);
    if (!(bv > tol)) { stopped = true; break; }
    const long p = bi;
    const int nk = j - kb;
    for (int k = tid; k < nk; k += PT) s_row[k] = P[(long)k * pitch + p];
    __syncthreads();
    const double* Ap = A + p * a.lda;
    double* Pj = P + (long)nk * pitch;
    for (long i = tid; i < m; i += PT) {
      double c = Ap[i];
      const double* Pi = P + i;
      for (int k = 0; k < nk; ++k) c -= Pi[(long)k * pitch] * s_row[k];
      Pj[i] = c;                                   // (read back by this thread only)
      if (i == p) s_cpp = c;
    }
    __syncthreads();
    const double cpp = s_cpp;
    if (!(cpp > 0.0 && isfinite(cpp))) { stopped = true; break; }
    const double s = sqrt(cpp);
    for (long i = tid; i < m; i += PT) {
      const double di = d[i];
      const bool fr = di != ninf && i != p;
      const double val = i == p ? s : (fr ? Pj[i] / s : 0.0);
      Pj[i] = val;
      if (val != 0.0) L[i * a.ldl + j] = val;      // (L was zeroed before the first launch)
      d[i] = fr ? di - val * val : ninf;
    }
    if (tid == 0) piv[j] = p;
    rank = j + 1;
    __syncthreads();                               // column j is complete (s_row, s_cpp and s_rv may be written again)
  }
  __syncthreads();
  // the largest remaining diagonal entry over the free indices (0 when none is left); the member's words
  double rv = ninf; int ri = INT_MAX;
  for (long i = tid; i < m; i += PT) {
    const double v = d[i];
    if (v > rv) { rv = v; ri = (int)i; }
  }
  block_amax(rv, ri, s_rv, s_ri);
  if (tid == 0) {
    state[0] = rank;
    state[1] = (stopped || rank == m) ? 1 : 0;
    a.rank[b] = rank;
    if (a.resid) a.resid[b] = rv == ninf ? 0.0 : rv;
  }
}

// dst[b][r][c] = r < srows && c < scols ? src[b][r][c] : fill, over rows x cols of every member
__global__ __launch_bounds__(256) void pstrf_copy_kernel(double* dst, long dld, long dstride, const double* src, long sld,
                                                         long sstride, long srows, long scols, long rows, long cols, long nbatch,
                                                         double fill) {
  const long tot = nbatch * rows * cols;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
    const long b = e / (rows * cols), q = e % (rows * cols), r = q / cols, c = q % cols;
    dst[b * dstride + r * dld + c] = (r < srows && c < scols) ? src[b * sstride + r * sld + c] : fill;
  }
}
// dst[b][r][c] = c < m ? mu[b][c] : 0 (mu == nullptr: 0) over rows x cols of every member: the draws before their GEMM
__global__ __launch_bounds__(256) void sample_rows_kernel(double* dst, long dld, long dstride, const double* mu, long m, long rows,
                                                          long cols, long nbatch) {
  const long tot = nbatch * rows * cols;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long)gridDim.x * 256) {
    const long b = e / (rows * cols), q = e % (rows * cols), r = q / cols, c = q % cols;
    dst[b * dstride + r * dld + c] = (mu && c < m) ? mu[b * m + c] : 0.0;
  }
}
// a[i][i] += jitter
__global__ __launch_bounds__(256) void add_diag_kernel(double* a, long ld, long n, double jitter) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) a[i * ld + i] += jitter;
}
// tol[0] = m eps max(max_i diag[i], 0): the default threshold on the PRIOR's scale
__global__ __launch_bounds__(256) void prior_tol_kernel(const double* diag, long m, double* tol) {
  __shared__ double sh[4];
  double v = 0.0;
  for (long i = threadIdx.x; i < m; i += 256) v = fmax(v, diag[i]);
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) tol[0] = ((double)m * GH_EPS) * fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

static unsigned copy_grid(long tot) { return (unsigned)std::min<long>((tot + 255) / 256, 8192); }
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

static int pstrf_copy(double* dst, long dld, long dstride, const double* src, long sld, long sstride, long srows, long scols,
                      long rows, long cols, long nbatch, double fill, hipStream_t st) {
  const long tot = nbatch * rows * cols;
  if (tot <= 0) return GH_OK;
  hipLaunchKernelGGL(pstrf_copy_kernel, dim3(copy_grid(tot)), dim3(256), 0, st, dst, dld, dstride, src, sld, sstride, srows, scols,
                     rows, cols, nbatch, fill);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

size_t gh_pstrf_work_bytes(int64_t m, int64_t nbatch) {
  const size_t mp = (size_t)gh_round_up(m, T), B = (size_t)nbatch;
  const bool whole = m <= GH_PSTRF_WHOLE;
  size_t tot = al256(B * 4 * sizeof(long long)) + al256(B * mp * sizeof(double));           // state, d
  tot += al256(B * (whole ? (size_t)m : (size_t)GH_PSTRF_PANEL) * mp * sizeof(double));         // P
  if (!whole) tot += al256(B * mp * mp * sizeof(double));                                     // W
  return tot;
}

int gh_launch_pstrf(const GhPstrf& p, hipStream_t st) {
  const long m = p.m, B = p.nbatch;
  if (B <= 0) return GH_OK;
  if (m < 1 || m > INT_MAX / 2 || p.lda < m || p.ldl < m || !p.A || !p.L || !p.piv || !p.rank || !p.work ||
      p.rows_l < m || p.cols_l < m || p.cols_l > p.ldl ||
      (B > 1 && (p.stride_a < (m - 1) * p.lda + m || p.stride_l < (p.rows_l - 1) * p.ldl + p.cols_l))) {
    gh_set_error("pstrf: bad argument (m %ld, lda %ld, ldl %ld, nbatch %ld)", m, (long)p.lda, (long)p.ldl, B);
    return GH_ERR_BAD_ARG;
  }
  if (p.work_bytes < gh_pstrf_work_bytes(m, B)) { gh_set_error("pstrf: work array too small"); return GH_ERR_BAD_ARG; }
  const long mp = gh_round_up(m, T);
  const bool whole = m <= GH_PSTRF_WHOLE;
  char* w = (char*)p.work;
  long long* state = (long long*)w;              w += al256((size_t)B * 4 * sizeof(long long));
  double* d = (double*)w;                        w += al256((size_t)B * mp * sizeof(double));
  const long kc = whole ? m : GH_PSTRF_PANEL;
  double* P = (double*)w;                        w += al256((size_t)B * kc * mp * sizeof(double));
  double* W = whole ? nullptr : (double*)w;
  // L = 0 over the region the caller reads (its padding included), piv = -1
  GH_CHECK(pstrf_copy(p.L, p.ldl, p.stride_l, nullptr, 0, 0, 0, 0, p.rows_l, p.cols_l, B, 0.0, st));
  GH_HIP(hipMemsetAsync(p.piv, 0xFF, (size_t)B * m * sizeof(long long), st));
  PstrfArgs a;
  a.m = m; a.P = P; a.pitch = mp; a.pstride = kc * mp; a.d = d; a.dstride = mp;
  a.L = p.L; a.ldl = p.ldl; a.stride_l = p.stride_l;
  a.piv = p.piv; a.rank = p.rank; a.resid = p.resid; a.state = state; a.tol = p.tol; a.tol_dev = p.tol_dev;
  if (whole) {
    a.A = p.A; a.lda = p.lda; a.stride_a = p.stride_a;
    hipLaunchKernelGGL(pstrf_kernel<true>, dim3((unsigned)B), dim3(PT), 0, st, a, 0, (int)m);
    GH_HIP(hipGetLastError());
    return GH_OK;
  }
  // panels: the matrix padded to the tile (the GEMM's shapes), zero outside m x m
  GH_CHECK(pstrf_copy(W, mp, mp * mp, p.A, p.lda, p.stride_a, m, m, mp, mp, B, 0.0, st));
  GH_HIP(hipMemsetAsync(P, 0, (size_t)B * kc * mp * sizeof(double), st));
  a.A = W; a.lda = mp; a.stride_a = mp * mp;
  std::vector<long long> hs((size_t)B * 4);
  for (long j0 = 0; j0 < m; j0 += GH_PSTRF_PANEL) {
    const long j1 = std::min<long>(j0 + GH_PSTRF_PANEL, m);
    hipLaunchKernelGGL(pstrf_kernel<false>, dim3((unsigned)B), dim3(PT), 0, st, a, (int)j0, (int)j1);
    GH_HIP(hipGetLastError());
    if (j1 == m) break;
    GH_HIP(hipMemcpyAsync(hs.data(), state, hs.size() * sizeof(long long), hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    bool any = false;
    for (long b = 0; b < B; ++b) {
      if (hs[4 * b + 1]) continue;                 // stopped (or failed): its matrix is not read again
      any = true;
      GhGemm g{};
      g.C = W + b * mp * mp; g.ldc = mp;
      g.A = P + b * kc * mp; g.lda = mp; g.B = g.A; g.ldb = mp;
      g.M = mp; g.N = mp; g.K = GH_PSTRF_PANEL; g.alpha = -1.0; g.beta = 1.0; g.a_km = false; g.b_km = false;
      GH_CHECK(gh_launch_gemm(g, st));
    }
    if (!any) break;
  }
  return GH_OK;
}

extern "C" int gh_dev_pstrf(double* a, int64_t lda, int64_t stride_a, int64_t m, int32_t nbatch, double tol,
                            double* l, int64_t ldl, int64_t stride_l, int64_t* piv, int64_t* rank, double* resid_diag,
                            void* stream) {
  if (nbatch < 0) { gh_set_error("pstrf: negative batch"); return GH_ERR_BAD_ARG; }
  if (nbatch == 0) return GH_OK;
  if (m < 1) { gh_set_error("pstrf: m must be at least 1"); return GH_ERR_BAD_ARG; }
  hipStream_t st = (hipStream_t)stream;
  GhPooledBuf work;
  GhPstrf p{};
  p.A = a; p.lda = lda; p.stride_a = stride_a; p.m = m; p.nbatch = nbatch; p.tol = tol; p.tol_dev = nullptr;
  p.L = l; p.ldl = ldl; p.stride_l = stride_l; p.rows_l = m; p.cols_l = m;
  p.piv = (long long*)piv; p.rank = (long long*)rank; p.resid = resid_diag;
  const size_t wb = gh_pstrf_work_bytes(m, nbatch);
  GH_CHECK(work.ensure(wb));
  p.work = work.p; p.work_bytes = work.bytes;
  const int rc = gh_launch_pstrf(p, st);
  (void)hipStreamSynchronize(st);                  // (the work array goes back to the block cache: nothing may still use it)
  if (rc != GH_OK) return rc;
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// ================================================================================ draws behind the factor
// draws[b] (nz, m) = mu[b] + z[b][:, :rank] L_b[:, :rank]^T.  Columns >= rank of L are exactly zero, so the product runs over
// all m columns as ONE GEMM per member on 128-padded copies: Z (nzp x mp), L (mp x mp, what the factor kernel writes) and the
// draws (nzp x mp, preset to the mean rows).  A member with a NaN covariance has NaN in L, hence NaN draws, and rank -1.
size_t gh_sample_work_bytes(int64_t m, int64_t nz, int64_t nbatch) {
  const size_t mp = (size_t)gh_round_up(m, T), nzp = (size_t)gh_round_up(nz, T), B = (size_t)nbatch;
  size_t tot = al256(B * mp * mp * sizeof(double)) + 2 * al256(B * nzp * mp * sizeof(double));      // L, Z, draws
  tot += al256(B * (size_t)m * sizeof(long long)) + al256(B * sizeof(long long));                    // piv, rank
  tot += al256(B * (size_t)nz * m * sizeof(double)) + al256(B * (size_t)m * m * sizeof(double));    // z in / draws out, fac out
  return tot + gh_pstrf_work_bytes(m, nbatch);
}

int gh_sample_enqueue(const GhSample& q, hipStream_t st) {
  const long m = q.m, nz = q.nz, B = q.nbatch;
  if (B <= 0) return GH_OK;
  if (m < 1 || nz < 1 || !q.cov || !q.z || !q.draws || !q.rank || !q.work) { gh_set_error("sample: bad argument"); return GH_ERR_BAD_ARG; }
  if (q.work_bytes < gh_sample_work_bytes(m, nz, B)) { gh_set_error("sample: work array too small"); return GH_ERR_BAD_ARG; }
  const long mp = gh_round_up(m, T), nzp = gh_round_up(nz, T);
  char* w = (char*)q.work;
  double* L = (double*)w;                w += al256((size_t)B * mp * mp * sizeof(double));
  double* Z = (double*)w;                w += al256((size_t)B * nzp * mp * sizeof(double));
  double* D = (double*)w;                w += al256((size_t)B * nzp * mp * sizeof(double));
  long long* piv = (long long*)w;        w += al256((size_t)B * m * sizeof(long long));
  long long* rank = (long long*)w;       w += al256((size_t)B * sizeof(long long));
  double* zio = (double*)w;              w += al256((size_t)B * nz * m * sizeof(double));
  double* fio = (double*)w;              w += al256((size_t)B * m * m * sizeof(double));
  // the normals, padded
  const double* zsrc = q.z;
  if (!gh_is_device_ptr(q.z)) {
    GH_HIP(hipMemcpyAsync(zio, q.z, (size_t)B * nz * m * sizeof(double), hipMemcpyHostToDevice, st));
    zsrc = zio;
  }
  GH_CHECK(pstrf_copy(Z, mp, nzp * mp, zsrc, m, nz * m, nz, m, nzp, mp, B, 0.0, st));
  // the factor
  GhPstrf p{};
  p.A = q.cov; p.lda = q.lda; p.stride_a = q.stride; p.m = m; p.nbatch = B; p.tol = q.tol; p.tol_dev = q.tol_dev;
  p.L = L; p.ldl = mp; p.stride_l = mp * mp; p.rows_l = mp; p.cols_l = mp;
  p.piv = piv; p.rank = rank; p.resid = nullptr;
  p.work = w; p.work_bytes = q.work_bytes - (size_t)(w - (char*)q.work);
  GH_CHECK(gh_launch_pstrf(p, st));
  // the draws
  {
    const long tot = B * nzp * mp;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(copy_grid(tot)), dim3(256), 0, st, D, mp, nzp * mp, q.mu, m, nzp, mp, B);
    GH_HIP(hipGetLastError());
  }
  for (long b = 0; b < B; ++b) {
    GhGemm g{};
    g.C = D + b * nzp * mp; g.ldc = mp;
    g.A = Z + b * nzp * mp; g.lda = mp; g.B = L + b * mp * mp; g.ldb = mp;
    g.M = nzp; g.N = mp; g.K = mp; g.alpha = 1.0; g.beta = 1.0; g.a_km = true; g.b_km = true;
    GH_CHECK(gh_launch_gemm(g, st));
  }
  // results, in the caller's layout (through a packed device copy when the caller's array is host memory)
  if (gh_is_device_ptr(q.draws)) {
    GH_CHECK(pstrf_copy(q.draws, m, nz * m, D, mp, nzp * mp, nz, m, nz, m, B, 0.0, st));
  } else {
    GH_CHECK(pstrf_copy(zio, m, nz * m, D, mp, nzp * mp, nz, m, nz, m, B, 0.0, st));
    GH_HIP(hipMemcpyAsync(q.draws, zio, (size_t)B * nz * m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (q.fac) {
    if (gh_is_device_ptr(q.fac)) {
      GH_CHECK(pstrf_copy(q.fac, m, m * m, L, mp, mp * mp, m, m, m, m, B, 0.0, st));
    } else {
      GH_CHECK(pstrf_copy(fio, m, m * m, L, mp, mp * mp, m, m, m, m, B, 0.0, st));
      GH_HIP(hipMemcpyAsync(q.fac, fio, (size_t)B * m * m * sizeof(double), hipMemcpyDeviceToHost, st));
    }
  }
  GH_HIP(hipMemcpyAsync(q.rank, rank, (size_t)B * sizeof(long long),
                        gh_is_device_ptr(q.rank) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  return GH_OK;
}

int gh_launch_prior_tol(const double* diag, int64_t m, double* tol_dev, hipStream_t st) {
  hipLaunchKernelGGL(prior_tol_kernel, dim3(1), dim3(256), 0, st, diag, (long)m, tol_dev);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// prior draws at t: K(t, t) + jitter I, factored and multiplied as above (gp.py sample(t): get_matrix + TINY on the diagonal +
// multivariate_gaussian_samples).  Null stream of the current device, as gh_kernel_value_symmetric.
extern "C" int gh_kernel_sample(gh_kernel* k, const double* t, int64_t m, double jitter, const double* z, int64_t nz, double tol,
                                double* draws, double* fac, int64_t* rank) {
  if (!k) { gh_set_error("invalid kernel"); return GH_ERR_BAD_ARG; }
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd kernels need an MI355X"); return GH_ERR_HIP; }
  if (m < 1 || nz < 1 || !t || !z || !draws || !rank) { gh_set_error("bad argument to kernel_sample"); return GH_ERR_BAD_ARG; }
  GH_CHECK(k->upload());
  hipStream_t st = 0;
  const long mp = gh_round_up(m, T);
  GhBuf tb, cov, work;
  const double* td = t;
  if (!gh_is_device_ptr(t)) {
    GH_CHECK(tb.ensure((size_t)m * k->ndim * sizeof(double)));
    GH_CHECK(gh_to_device(tb.d(), t, (size_t)m * k->ndim, st));
    td = tb.d();
  }
  GH_CHECK(cov.ensure((size_t)mp * mp * sizeof(double)));
  GH_CHECK(gh_launch_kmat(k, td, m, td, m, nullptr, cov.d(), mp, mp, mp, 0, 0, true, false, st));
  if (jitter != 0.0) {
    hipLaunchKernelGGL(add_diag_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, cov.d(), mp, (long)m, jitter);
    GH_HIP(hipGetLastError());
  }
  const size_t wb = gh_sample_work_bytes(m, nz, 1);
  GH_CHECK(work.ensure(wb));
  GhSample q{};
  q.cov = cov.d(); q.lda = mp; q.stride = mp * mp; q.m = m; q.nbatch = 1; q.tol = tol; q.tol_dev = nullptr; q.mu = nullptr;
  q.z = z; q.nz = nz; q.draws = draws; q.fac = fac; q.rank = rank; q.work = work.p; q.work_bytes = work.bytes;
  const int rc = gh_sample_enqueue(q, st);
  (void)hipStreamSynchronize(st);                  // (the buffers above are freed on return)
  if (rc != GH_OK) return rc;
  GH_HIP(hipGetLastError());
  return GH_OK;
}
