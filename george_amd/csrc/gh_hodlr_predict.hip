// gh_hodlr_predict.hip -- predict and the likelihood gradient on a computed HODLR factor (gh_hodlr_impl.h has the map of the units)
#include <atomic>
#include "gh_hodlr_impl.h"

// ===================================================================== predict / likelihood gradient on the factor
// gh_hodlr_predict / gh_hodlr_grad (include/george_amd.h): the GP glue around apply_inverse (gp.py:482-545, :429-466) without
// the M x N and N x N host arrays of the generic branch.  Both walk over COLUMN STRIPS: an n x Ct row-major block is built on the
// device (cross-covariances, or columns of the identity), hodlr_solve_all() turns it into K^-1 times itself in place, and one
// reduction kernel consumes it; only M- or P-vectors reach the host.
//
// HODLR_STRIP_BYTES is what ONE strip of n x Ct doubles may take: 512 MiB.  predict holds two strips (K(x, xs_J) and K^-1 of
// it), grad one, so the calls need at most 1 GiB beyond the factor whatever M or n is.  At n = 262 144 it gives Ct = 256 = CPASS
// -- one column pass of the wide solve per strip, its natural width; at n <= 32 768 the cap of 2048 columns applies (wider
// strips gain nothing: the solve goes in passes of CPASS columns anyway).
#define HODLR_STRIP_BYTES (512L << 20)
#define HODLR_STRIP_MAX 2048
#define HODLR_RED_ROWS 128         // rows per chunk of the column reduction (at most HODLR_RED_CHUNKS chunks)
#define HODLR_RED_CHUNKS 2048
#define HGT 64                     // tile edge of the strip gradient reduction (kgrad_reduce_kernel's)
static std::atomic<int> g_hodlr_strip_cols{0};
extern "C" int gh_debug_set_hodlr_strip_cols(int cols) {
  return g_hodlr_strip_cols.exchange(cols > 0 ? cols : 0);
}
// strip width for an n-row problem that has `need` columns to get through
static long strip_cols(long n, long need) {
  const int forced = g_hodlr_strip_cols;
  long ct = forced > 0 ? gh_round_up(forced, 64) : HODLR_STRIP_BYTES / (8 * n) / 64 * 64;
  if (forced <= 0) ct = std::min<long>(ct, HODLR_STRIP_MAX);
  ct = std::min<long>(ct, gh_round_up(need, 64));
  return std::max<long>(ct, 64);
}

// Two-operand column reduction: for the cw columns of a strip (row pitch ld) and the rows of chunk blockIdx.y,
//   pmu[chunk][j] = sum_i Kx[i][j] alpha[i],   pvar[chunk][j] = sum_i Kx[i][j] W[i][j]   (W == nullptr: the mean only)
// A thread per column: a wavefront reads 64 consecutive doubles of a row of each operand, alpha[i] is a uniform load.
__global__ __launch_bounds__(64) void hodlr_colred2_kernel(const double* __restrict__ Kx, const double* __restrict__ W, long ld, long n,
                                                           long rows_per, const double* __restrict__ alpha, int cw,
                                                           double* __restrict__ pmu, double* __restrict__ pvar, long ldp) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= cw) return;
  const long r0 = (long)blockIdx.y * rows_per, r1 = r0 + rows_per < n ? r0 + rows_per : n;
  double smu = 0.0, sv = 0.0;
  if (W) {
#pragma unroll 4
    for (long i = r0; i < r1; ++i) {
      const double a = Kx[i * ld + j];
      smu += a * alpha[i];
      sv += a * W[i * ld + j];
    }
    pvar[(long)blockIdx.y * ldp + j] = sv;
  } else {
#pragma unroll 4
    for (long i = r0; i < r1; ++i) smu += Kx[i * ld + j] * alpha[i];
  }
  pmu[(long)blockIdx.y * ldp + j] = smu;
}
// the chunk partials added in chunk order: mu[j] = sum, var[j] = var[j] (holding k(xs_j, xs_j)) - sum
__global__ __launch_bounds__(64) void hodlr_colfinal2_kernel(const double* __restrict__ pmu, const double* __restrict__ pvar, long nchunks, long ldp,
                                                             int cw, double* __restrict__ mu, double* __restrict__ var) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= cw) return;
  double smu = 0.0, sv = 0.0;
  for (long c = 0; c < nchunks; ++c) smu += pmu[c * ldp + j];
  mu[j] = smu;
  if (var) {
    for (long c = 0; c < nchunks; ++c) sv += pvar[c * ldp + j];
    var[j] = var[j] - sv;
  }
}
// The rectangular strip form of kgrad_reduce_kernel (gh_kmat.hip): W = K^-1 E_J for the columns J = [col0, col0 + cw) (row pitch
// ld); workgroup (blockIdx.x, blockIdx.y) takes the 64 x 64 tile of rows 64 blockIdx.x .. and strip columns 64 blockIdx.y .. and
// writes ONE partial row  1/2 sum_{i, j in tile} (alpha_i alpha_j - W[i][j - col0]) dK(x_i, x_j)/dtheta_p.  Every (i, j) of the
// square counts (the solver's inverse is not exactly symmetric: 0.5 * einsum("ijk,ij", dK, A) of the generic branch); dK is evaluated
// with the smaller index first (kernel_interface.cpp:117-121).  The element on the diagonal also gives diagA.
template <int PMAX>
__global__ __launch_bounds__(256, PMAX <= 16 ? 2 : 1) void hodlr_kgrad_strip_kernel(const GhNode* __restrict__ prog, int n_nodes, int nd, int P,
                                                           const uint32_t* which, const double* x, long n, const double* alpha,
                                                           const double* W, long ld, long col0, int cw,
                                                           double* partial, double* diagA) {
  extern __shared__ __attribute__((aligned(16))) double hgx[];      // the tile's x rows and x columns, 2 * HGT * nd doubles (launch argument)
  double* const xr = hgx;
  double* const xc = hgx + HGT * nd;
  __shared__ double red[4][PMAX];
  // the evaluator's runtime-indexed arrays -- g[] and its work space -- per thread: in LDS for PMAX <= 16 (an odd pitch in doubles:
  // the 64-bit accesses of 32 consecutive threads fall on different banks), so that those forms use no scratch memory.  33 doubles
  // per thread at PMAX = 16 are 66 KiB a workgroup: with the x rows sized by nd, two workgroups share a CU's 160 KiB up to nd = 13.
  constexpr int GP = PMAX <= 16 ? PMAX + GH_EVAL_WS + 1 : 1;
  __shared__ double gl[PMAX <= 16 ? 256 * GP : 1];
  double gp_[PMAX <= 16 ? 1 : PMAX];
  double* const g = PMAX <= 16 ? &gl[threadIdx.x * GP] : gp_;
  double* const ws = PMAX <= 16 ? g + PMAX : nullptr;
  const long r0 = (long)blockIdx.x * HGT;
  const int cl0 = blockIdx.y * HGT;
  const long c0 = col0 + cl0;
  for (int t = threadIdx.x; t < HGT * nd; t += 256) {
    const long r = r0 + t / nd;
    xr[t] = (r < n) ? x[r * nd + (t % nd)] : 0.0;
    const long c = c0 + t / nd;
    xc[t] = (c < n) ? x[c * nd + (t % nd)] : 0.0;
  }
  __syncthreads();
  double acc[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) acc[p] = 0.0;
  const int lc = threadIdx.x & 63;
  const int lr = threadIdx.x >> 6;
  const int cl = cl0 + lc;
  const long c = col0 + cl;
#pragma unroll 1
  for (int pass = 0; pass < HGT / 4; ++pass) {
    const int rr = lr + pass * 4;
    const long r = r0 + rr;
    if (r < n && cl < cw) {                 // (cl < cw implies c < n)
      const bool lower = c <= r;
      gh_eval_grad(prog, n_nodes, lower ? &xc[lc * nd] : &xr[rr * nd], lower ? &xr[rr * nd] : &xc[lc * nd], g, ws);
      const double aij = alpha[r] * alpha[c] - W[r * ld + cl];
      if (r == c && diagA) diagA[r] = aij;
      const double w = 0.5 * aij;
#pragma unroll
      for (int p = 0; p < PMAX; ++p) if (p < P) acc[p] += w * g[p];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < PMAX; ++p) {
    double v = acc[p];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][p] = v;
  }
  __syncthreads();
  if (threadIdx.x < PMAX && threadIdx.x < P) {
    const int p = threadIdx.x;
    partial[((long)blockIdx.y * gridDim.x + blockIdx.x) * P + p] = which[p] ? (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]) : 0.0;
  }
}
// what predict and grad check alike (the order of gh_chol_predict / gh_chol_grad: handle, arguments, dimension)
static int need_whole(gh_hodlr* h, const char* what) {
  GH_CHECK(hodlr_need(h));
  if (h->sub.depth != 0) { gh_set_error("%s: not offered on a sub-tree handle of the multi-device split", what); return GH_ERR_BAD_ARG; }
  return GH_OK;
}
// alpha = K^-1 r into a device vector of its own (the one-column solve of gh_hodlr_dot_solve)
static int solve_alpha(gh_hodlr* h, const double* r, GhBuf& al) {
  GH_CHECK(al.ensure((size_t)h->n * sizeof(double)));
  GH_CHECK(gh_to_device(al.d(), r, (size_t)h->n, h->st));
  return hodlr_solve_all(h, hodlr_passes(), al.d(), 1, 1);
}

extern "C" int gh_hodlr_predict(gh_hodlr* h, gh_kernel* k, const double* r, const double* xs, int64_t m,
                                double* mu, double* var, double* cov) {
  GH_CHECK(need_whole(h, "predict"));
  if (!k || !r || !xs || !mu || m <= 0 || (var && cov) || m > 0x3fffffffL) { gh_set_error("bad argument to predict"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_CHECK(k->upload());
  const long n = h->n;
  const int passes = hodlr_passes();
  hipStream_t st = h->st;
  GhPooledBuf al, xsd, sK, sW, part, res, kss;
  GH_CHECK(solve_alpha(h, r, al));
  const double* xs_dev = xs;
  if (!gh_is_device_ptr(xs)) {
    GH_CHECK(xsd.ensure((size_t)m * h->ndim * sizeof(double)));
    GH_CHECK(gh_to_device(xsd.d(), xs, (size_t)m * h->ndim, st));
    xs_dev = xsd.d();
  }
  // with cov, all of Kx and W stay resident for the product: one strip of mp columns over np rows (GhGemm: M, N multiples of
  // 128, K of 16; the padding is zero).  Without, strips of Ct columns.
  const long mp = gh_round_up(m, 128), np = cov ? gh_round_up(n, 16) : n;
  const long Ct = cov ? mp : strip_cols(n, m);
  const size_t strip_bytes = (size_t)np * Ct * sizeof(double);
  const bool want_w = var || cov;
  if (sK.ensure(strip_bytes) != GH_OK || (want_w && sW.ensure(strip_bytes) != GH_OK) || (cov && kss.ensure((size_t)mp * mp * sizeof(double)) != GH_OK)) {
    if (cov) gh_set_error("predict: the covariance keeps K(x, xs) and K^-1 K(x, xs) on the device, 2 x %zu bytes for n = %ld, m = %ld, and they do not "
                          "fit; ask for the variance or for fewer test points at a time", strip_bytes, n, (long)m);
    return GH_ERR_NOMEM;
  }
  const long nchunks = std::min<long>(HODLR_RED_CHUNKS, (n + HODLR_RED_ROWS - 1) / HODLR_RED_ROWS);
  const long rows_per = (n + nchunks - 1) / nchunks;
  GH_CHECK(part.ensure((size_t)2 * nchunks * Ct * sizeof(double)));
  GH_CHECK(res.ensure((size_t)2 * m * sizeof(double)));
  double* pmu = part.d();
  double* pvar = pmu + nchunks * Ct;
  double* dmu = res.d();
  double* dvar = dmu + m;
  if (var) GH_CHECK(gh_launch_kdiag(k, xs_dev, xs_dev, m, dvar, st));           // gp.py:539
  for (long j0 = 0; j0 < m; j0 += Ct) {
    const int cw = (int)std::min<long>(Ct, m - j0);
    // Kx = K(x, xs_J), n x Ct row-major (columns past cw, rows past n: zero)
    GH_CHECK(gh_launch_kmat(k, h->x.d(), n, xs_dev + j0 * h->ndim, cw, nullptr, sK.d(), Ct, np, Ct, 0, 0, false, false, st));
    if (want_w) {
      // W = K^-1 Kx on a second copy   (gp.py:541, 544: apply_inverse(Kxs.T))
      GH_HIP(hipMemcpyAsync(sW.p, sK.p, strip_bytes, hipMemcpyDeviceToDevice, st));
      GH_CHECK(hodlr_solve_all(h, passes, sW.d(), Ct, cw));
    }
    hipLaunchKernelGGL(hodlr_colred2_kernel, dim3((unsigned)((cw + 63) / 64), (unsigned)nchunks), dim3(64), 0, st,
                       (const double*)sK.d(), var ? (const double*)sW.d() : (const double*)nullptr, Ct, n, rows_per,
                       (const double*)al.d(), cw, pmu, pvar, Ct);
    hipLaunchKernelGGL(hodlr_colfinal2_kernel, dim3((unsigned)((cw + 63) / 64)), dim3(64), 0, st, (const double*)pmu, (const double*)pvar,
                       nchunks, Ct, cw, dmu + j0, var ? dvar + j0 : (double*)nullptr);
    GH_HIP(hipGetLastError());
  }
  GH_CHECK(gh_from_device(mu, dmu, (size_t)m, st));
  if (var) GH_CHECK(gh_from_device(var, dvar, (size_t)m, st));
  if (cov) {
    // cov = K(xs, xs) - Kx^T W      (gp.py:543-545; not a V^T V form: the HODLR inverse is not exactly symmetric)
    GH_CHECK(gh_launch_kmat(k, xs_dev, m, xs_dev, m, nullptr, kss.d(), mp, mp, mp, 0, 0, true, false, st));
    GhGemm g{};
    g.C = kss.d(); g.ldc = mp; g.A = sK.d(); g.lda = mp; g.B = sW.d(); g.ldb = mp;
    g.M = mp; g.N = mp; g.K = np; g.alpha = -1.0; g.beta = 1.0; g.a_km = false; g.b_km = false;
    GH_CHECK(gh_launch_gemm(g, st));
    GH_HIP(hipMemcpy2DAsync(cov, m * sizeof(double), kss.d(), mp * sizeof(double), m * sizeof(double), m,
                            gh_is_device_ptr(cov) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_hodlr_grad(gh_hodlr* h, gh_kernel* k, const uint32_t* which, const double* r,
                             double* grad, double* alpha, double* diagA) {
  GH_CHECK(need_whole(h, "grad"));
  if (!k || !which || !r || !grad) { gh_set_error("bad argument to grad"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_CHECK(k->upload());
  const long n = h->n;
  const int P = k->size, nn = (int)k->nodes.size();
  const int passes = hodlr_passes();
  hipStream_t st = h->st;
  GhPooledBuf al, sW, part, sums, dg;
  GH_CHECK(solve_alpha(h, r, al));                   // gp.py:429
  if (alpha) GH_CHECK(gh_from_device(alpha, al.d(), (size_t)n, st));
  if (P <= 0 && !diagA) { GH_HIP(hipStreamSynchronize(st)); return GH_OK; }
  const long Ct = strip_cols(n, n);
  const long nstrips = (n + Ct - 1) / Ct, tm = (n + HGT - 1) / HGT, tc = Ct / HGT;
  const int Pw = P > 0 ? P : 1;
  const size_t which_bytes = ((sizeof(uint32_t) * Pw + 15) / 16) * 16;
  GH_CHECK(sW.ensure((size_t)n * Ct * sizeof(double)));
  GH_CHECK(part.ensure(which_bytes + (size_t)tm * tc * Pw * sizeof(double)));
  GH_CHECK(sums.ensure((size_t)(nstrips + 1) * Pw * sizeof(double)));
  GH_CHECK(dg.ensure((size_t)n * sizeof(double)));
  uint32_t* d_which = (uint32_t*)part.p;
  double* partial = (double*)((char*)part.p + which_bytes);
  double* dgrad = sums.d() + nstrips * Pw;
  if (P > 0) GH_HIP(hipMemcpyAsync(d_which, which, sizeof(uint32_t) * P, hipMemcpyHostToDevice, st));
  for (long s = 0; s < nstrips; ++s) {
    const long col0 = s * Ct;
    const int cw = (int)std::min<long>(Ct, n - col0);
    // W = K^-1 E_J    (gp.py:436 get_inverse, a strip of its columns at a time)
    GH_HIP(hipMemsetAsync(sW.p, 0, (size_t)n * Ct * sizeof(double), st));
    GH_CHECK(hodlr_launch_eye_strip(sW.d(), Ct, col0, cw, st));
    GH_CHECK(hodlr_solve_all(h, passes, sW.d(), Ct, cw));
    const dim3 grid((unsigned)tm, (unsigned)((cw + HGT - 1) / HGT));
#define GH_LAUNCH_STRIP(PM)                                                                                          \
  hipLaunchKernelGGL(hodlr_kgrad_strip_kernel<PM>, grid, dim3(256), (size_t)2 * HGT * k->ndim * sizeof(double), st, (const GhNode*)k->d_nodes, nn, k->ndim, P, \
                     (const uint32_t*)d_which, (const double*)h->x.d(), n, (const double*)al.d(), (const double*)sW.d(), Ct, col0, cw, partial, dg.d())
    if (P <= 4) GH_LAUNCH_STRIP(4);
    else if (P <= 16) GH_LAUNCH_STRIP(16);
    else GH_LAUNCH_STRIP(GH_MAX_GRAD);
#undef GH_LAUNCH_STRIP
    GH_HIP(hipGetLastError());
    // the strip's tiles in a fixed order, then (below) the strips in order: two calls give the same bits
    GH_CHECK(gh_launch_kgrad_final(partial, (long)grid.x * grid.y, P, sums.d() + s * P, st));
  }
  if (P > 0) {
    GH_CHECK(gh_launch_kgrad_final(sums.d(), nstrips, P, dgrad, st));
    GH_CHECK(gh_from_device(grad, dgrad, (size_t)P, st));
  }
  if (diagA) GH_CHECK(gh_from_device(diagA, dg.d(), (size_t)n, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}
