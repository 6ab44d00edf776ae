// gh_predict.hip -- what the solvers' predict calls share: the test points on the device, the pitched copy to or from the caller,
// the column reduction behind the mean and the variance, and the strip driver of the solvers that keep no buffers of their own
// (gh_hodlr_predict, gh_vecchia_predict).  Launchers and driver are declared in gh_common.h.
#include <algorithm>
#include "gh_common.h"

int gh_stage_points(const double* xs, int64_t m, int ndim, GhBuf& own, hipStream_t st, const double** xs_dev) {
  *xs_dev = xs;
  if (!gh_is_device_ptr(xs)) {
    GH_CHECK(own.ensure((size_t)m * ndim * sizeof(double)));
    GH_CHECK(gh_to_device(own.d(), xs, (size_t)m * ndim, st));
    *xs_dev = own.d();
  }
  return GH_OK;
}
int gh_copy_rows(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t cols, int64_t rows, bool from_caller, hipStream_t st) {
  const bool dev = gh_is_device_ptr(from_caller ? (const void*)src : (const void*)dst);
  GH_HIP(hipMemcpy2DAsync(dst, ldd * sizeof(double), src, lds * sizeof(double), cols * sizeof(double), rows,
                          dev ? hipMemcpyDeviceToDevice : from_caller ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
  return GH_OK;
}

// ===================================================================== column reduction
// For the `cols` columns of row-major operands (row pitch ld) and the rows of chunk blockIdx.y
//   pmu[chunk][j] = sum_i A[i][j] z[i],   pvar[chunk][j] = sum_i P[i][j] Q[i][j]
// A thread per column: a wavefront reads 64 consecutive doubles of a row of each operand, z[i] is a uniform load.  Rows ascending,
// one multiply-add per row and sum.  SECOND says where P and Q lie, so that no operand is loaded twice:
enum { RED_MEAN = 0,    // no second moment
       RED_AA,          // P == Q == A     (dense: V = L^-1 K(x, xs))
       RED_AQ,          // P == A          (HODLR: K(x, xs) and K^-1 K(x, xs))
       RED_QQ };        // P == Q != A     (Vecchia: V = F^-1/2 (I - B) K(x, xs))
template <int SECOND>
__global__ __launch_bounds__(256) void gh_colred_kernel(const double* __restrict__ A, const double* __restrict__ z, const double* __restrict__ Q,
                                                        long ld, long n, long rows_per, long cols, double* __restrict__ pmu,
                                                        double* __restrict__ pvar, long ldp) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  const long r0 = (long)blockIdx.y * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double smu = 0.0, sv = 0.0;
  if (SECOND == RED_QQ) {
    // a pass per operand: with both streams in one loop the Vecchia predict at n = 262 144 (strips of 512 MiB) took 0.5 - 2 %
    // longer (profiles/predict_refactor_ab.md)
    for (long i = r0; i < r1; ++i) smu += A[i * ld + j] * z[i];
    for (long i = r0; i < r1; ++i) { const double q = Q[i * ld + j]; sv += q * q; }
  } else {
#pragma unroll 4
    for (long i = r0; i < r1; ++i) {
      const double a = A[i * ld + j];
      smu += a * z[i];
      if (SECOND == RED_AA) sv += a * a;
      if (SECOND == RED_AQ) sv += a * Q[i * ld + j];
    }
  }
  pmu[(long)blockIdx.y * ldp + j] = smu;
  if (SECOND != RED_MEAN) pvar[(long)blockIdx.y * ldp + j] = sv;
}
// the chunk partials added in chunk order: mu[j] = sum, var[j] = var[j] (holding k(xs_j, xs_j)) - sum
__global__ __launch_bounds__(256) void gh_colfinal_kernel(const double* __restrict__ pmu, const double* __restrict__ pvar, long nchunks, long ldp,
                                                          long cols, double* __restrict__ mu, double* __restrict__ var) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double smu = 0.0, sv = 0.0;
  for (long c = 0; c < nchunks; ++c) smu += pmu[c * ldp + j];
  mu[j] = smu;
  if (var) {
    for (long c = 0; c < nchunks; ++c) sv += pvar[c * ldp + j];
    var[j] = var[j] - sv;
  }
}
int gh_launch_colreduce(const double* A, const double* z, const double* P, const double* Q, int64_t ld, int64_t nrows, int64_t rows_per,
                        int64_t nchunks, int64_t cols, double* pmu, double* pvar, int64_t ldp, double* mu, double* var, int threads,
                        hipStream_t st) {
  if (threads < 64 || threads > 256 || (var && !P) || (P && P != A && P != Q)) { gh_set_error("bad argument to the column reduction"); return GH_ERR_BAD_ARG; }
  const dim3 grid((unsigned)((cols + threads - 1) / threads), (unsigned)nchunks), wg(threads);
#define GH_COLRED(SECOND) \
  hipLaunchKernelGGL(gh_colred_kernel<SECOND>, grid, wg, 0, st, A, z, Q, (long)ld, (long)nrows, (long)rows_per, (long)cols, pmu, pvar, (long)ldp)
  if (!P) GH_COLRED(RED_MEAN);
  else if (P != A) GH_COLRED(RED_QQ);
  else if (Q == A) GH_COLRED(RED_AA);
  else GH_COLRED(RED_AQ);
#undef GH_COLRED
  hipLaunchKernelGGL(gh_colfinal_kernel, dim3(grid.x), wg, 0, st, (const double*)pmu, (const double*)pvar, (long)nchunks, (long)ldp, (long)cols,
                     mu, var);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// ===================================================================== strip driver
// Strips of K(x, xs_J), n x Ct row-major, are built on the device; make_second() turns a strip into the solver's second operand
// (same shape, a buffer of its own) when the variance or the covariance is asked for, and the column reduction consumes both: only
// m-vectors reach the host.  With cov both operands stay whole for one product: a single strip of mp columns over np rows
// (GhGemm: M, N multiples of 128, K of 16; the padding is zero).
int gh_predict_strips(gh_kernel* k, const double* x, int64_t n, int ndim, const double* alpha, const double* xs_dev, int64_t m,
                      int64_t strip_cols, int64_t red_rows, int64_t red_chunks, double* mu, double* var, double* cov, hipStream_t st,
                      bool first_second, const GhMakeSecond& make_second) {
  const int64_t mp = gh_round_up(m, GH_TILE), np = cov ? gh_round_up(n, 16) : n;
  const int64_t Ct = cov ? mp : strip_cols;
  const size_t strip_bytes = (size_t)np * Ct * sizeof(double);
  const bool want_second = var || cov;
  GhPooledBuf sK, sS, kss, part, res;
  GH_CHECK(sK.ensure(strip_bytes));
  if (want_second) GH_CHECK(sS.ensure(strip_bytes));
  if (cov) GH_CHECK(kss.ensure((size_t)mp * mp * sizeof(double)));
  const int64_t nchunks = std::min<int64_t>(red_chunks, (n + red_rows - 1) / red_rows);
  const int64_t rows_per = (n + nchunks - 1) / nchunks;
  GH_CHECK(part.ensure((size_t)2 * nchunks * Ct * sizeof(double)));
  GH_CHECK(res.ensure((size_t)2 * m * sizeof(double)));
  double* pmu = part.d();
  double* pvar = pmu + nchunks * Ct;
  double* dmu = res.d();
  double* dvar = dmu + m;
  if (var) GH_CHECK(gh_launch_kdiag(k, xs_dev, xs_dev, m, dvar, st));           // gp.py:539
  if (np > n) GH_HIP(hipMemsetAsync(sS.d() + n * Ct, 0, (size_t)(np - n) * Ct * sizeof(double), st));     // (the rows the product reads past n)
  for (int64_t j0 = 0; j0 < m; j0 += Ct) {
    const int cw = (int)std::min<int64_t>(Ct, m - j0);
    // Kx = K(x, xs_J), np x Ct row-major (columns past cw, rows past n: zero)
    GH_CHECK(gh_launch_kmat(k, x, n, xs_dev + j0 * ndim, cw, nullptr, sK.d(), Ct, np, Ct, 0, 0, false, false, st));
    if (want_second) GH_CHECK(make_second(sK.d(), sS.d(), Ct, np, cw, strip_bytes));
    const double* P = !var ? nullptr : first_second ? sK.d() : sS.d();
    GH_CHECK(gh_launch_colreduce(sK.d(), alpha, P, var ? sS.d() : nullptr, Ct, n, rows_per, nchunks, cw, pmu, pvar, Ct, dmu + j0,
                                 var ? dvar + j0 : nullptr, 64, st));
  }
  GH_CHECK(gh_from_device(mu, dmu, (size_t)m, st));
  if (var) GH_CHECK(gh_from_device(var, dvar, (size_t)m, st));
  if (cov) {
    // cov = K(xs, xs) - first^T second, or - second^T second      (gp.py:543-545)
    GH_CHECK(gh_launch_kmat(k, xs_dev, m, xs_dev, m, nullptr, kss.d(), mp, mp, mp, 0, 0, true, false, st));
    GhGemm g{};
    g.C = kss.d(); g.ldc = mp; g.A = first_second ? sK.d() : sS.d(); g.lda = mp; g.B = sS.d(); g.ldb = mp;
    g.M = mp; g.N = mp; g.K = np; g.alpha = -1.0; g.beta = 1.0; g.a_km = false; g.b_km = false;
    GH_CHECK(gh_launch_gemm(g, st));
    GH_CHECK(gh_copy_rows(cov, m, kss.d(), mp, m, m, false, st));
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}
