// gh_hodlr_predict.hip -- predict and the likelihood gradient on a computed HODLR factor (gh_hodlr_impl.h has the map of the units)
#include <atomic>
#include "gh_hodlr_impl.h"

// ===================================================================== predict / likelihood gradient on the factor
// gh_hodlr_predict / gh_hodlr_grad (include/george_amd.h): the GP glue around apply_inverse (gp.py:482-545, :429-466) without
// the M x N and N x N host arrays of the generic branch.  Both walk over COLUMN STRIPS: an n x Ct row-major block is built on the
// device (cross-covariances, or columns of the identity), hodlr_solve_all() turns it into K^-1 times itself in place, and one
// reduction kernel consumes it; only M- or P-vectors reach the host.  predict's walk is the driver every solver shares
// (gh_predict_strips, gh_predict.hip): what is its own is alpha, the strip width and how a strip becomes K^-1 times itself.
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
  GhPooledBuf al, xsd;
  GH_CHECK(solve_alpha(h, r, al));
  const double* xs_dev = nullptr;
  GH_CHECK(gh_stage_points(xs, m, h->ndim, xsd, st, &xs_dev));
  // W = K^-1 Kx on a second copy   (gp.py:541, 544: apply_inverse(Kxs.T)); the moments are Kx . W, not a V^T V form: the HODLR
  // inverse is not exactly symmetric
  const int rc = gh_predict_strips(k, h->x.d(), n, h->ndim, al.d(), xs_dev, m, strip_cols(n, m), HODLR_RED_ROWS, HODLR_RED_CHUNKS, mu, var, cov,
                                   st, true, [&](const double* sK, double* sW, int64_t ld, int64_t, int cw, size_t strip_bytes) -> int {
    GH_HIP(hipMemcpyAsync(sW, sK, strip_bytes, hipMemcpyDeviceToDevice, st));
    return hodlr_solve_all(h, passes, sW, ld, cw);
  });
  if (rc == GH_ERR_NOMEM && cov)
    gh_set_error("predict: the covariance keeps K(x, xs) and K^-1 K(x, xs) on the device, 2 x %zu bytes for n = %ld, m = %ld, and they do not "
                 "fit; ask for the variance or for fewer test points at a time",
                 (size_t)gh_round_up(n, 16) * gh_round_up(m, 128) * sizeof(double), n, (long)m);
  return rc;
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
