// gh_inducing.hip -- the inducing-point (DTC / FITC / variational bound) solver behind gh_inducing_* (include/george_amd.h has
// the definition)
//
// Everything heavy is a launch of the fp64 GEMM (gh_launch_gemm) on strips of K_fu = K(x_J, u): `se` data points (rows) by mp
// columns, row-major with pitch mp (m padded to a multiple of 128; the padding is zero, and the identity in the m x m matrices).
// Triangular factors act through explicit inverses (gh_chol_linv), so there is no substitution kernel and no spin-wait; a
// product of two of them (K_uu^-1 = Lui^T Lui, M1^T M1) is never formed -- it would square the conditioning of K_uu -- but applied
// as two GEMMs.  Kept between calls, all mp x mp:  Lui = L_u^-1,  M1 = L_A^-1 L_u^-1 and two work matrices; plus lambda (n), x,
// yerr, u and a copy of the kernel program of compute() -- solve and dot_solve take no kernel.
//   compute:  V_J^T = F_J Lui^T;  lambda from its row sums;  G += (Lambda^-1/2 V_J^T)^T (Lambda^-1/2 V_J^T), a lower SYRK with beta = 1
//   solve:    c = sum_J F_J^T Lambda_J^-1 b_J;  t = M1 c;  w = M1^T t;  out_J = Lambda_J^-1 (b_J - F_J w)
//   grad:     H_J^T = F_J M1^T gives |H[:, i]|^2, and Z_J^T = alpha_J w^T - Lambda_J^-1 (H_J^T M1) - phi diag(diagA_J) (V_J^T Lui)
//             (P alpha = w and P C^-1 = M1^T M1 K_uf Lambda^-1 by the Woodbury identity; P^T = V^T Lui);  ZF = sum_J Z_J F_J;
//             W = -1/2 (ZF Lui^T) Lui.  The variational bound takes the FITC path with omega = -1 / lambda in place of diagA.
//   grad_u:   the same pass after one for G2 = H Lambda^-1 P^T and w = P alpha; per strip Z_J^T once more, from P_J^T itself
//             (ind_grad_body has the reason), ugrad += sum_i Z_J^T[i][j] d1 k(u_j, x_i) (gh_launch_wxgrad on the strip) and
//             Z P^T += Z_J P_J^T; after the strips ugrad -= sum_b (-(W + W^T))[b][j] d1 k(u_j, u_b)
//   loo:      c_i = (C^-1)_ii from the rows of H_J^T, and the values; with a mask two passes for B = 1/2 (v alpha^T + alpha v^T) -
//             C^-1 diag(w) C^-1 in low-rank form, and grad's reduction with 2 B in the place of alpha alpha^T - C^-1 (gh_inducing_loo)
//   predict:  V*^T = F* Lui^T,  H*^T = F* M1^T,  mu = F* w
// Strips go in ascending order on the handle's one stream and every sum has a fixed order (GEMM tiles, wave trees, per-workgroup
// partials added by gh_launch_kgrad_final): two calls give the same bits.  No kernel here uses scratch memory or atomics (the
// interpreter form of gh_launch_wxgrad, gh_predgrad.hip, keeps its operand stacks in scratch memory).
#include <string.h>
#include <algorithm>
#include "gh_common.h"
#include "gh_device_util.h"
#include "gh_chol_impl.h"

#define IND_M_MAX 8192                  // the cap on m: five padded m x m matrices (four kept, one of grad's; grad_u: one more) are 2.7 GB there
#define IND_STRIP_BYTES (3L << 29)      // what the three strips of a pass (F, Y and the FITC operand) may take together (grad_u: two more strips)
#define IND_COV_BYTES (8L << 30)        // what predict's covariance may keep on the device: three M x m strips and the M x M result
#define IND_GT 64                       // tile edge of the gradient reduction = lanes of its one-wavefront workgroup
#define IND_GRAD_LDS (128 * 1024)

struct gh_inducing {
  gh_inducing_opts opts;
  hipStream_t st = nullptr;
  bool shared_stream = false;
  int64_t n = 0, m = 0, mp = 0;
  int ndim = 0;
  bool computed = false;
  int64_t info = 0;
  double logdet = 0.0;
  double tau = 0.0;                     // the trace term of the variational bound, sum_i resid_i / yerr_i^2; 0 without the bound
  gh_kernel kc;                         // the kernel program as of compute(): what solve, dot_solve and t(r) build K_fu from
  GhPooledBuf x, yerr, u, lam, resid, vals, Lui, M1, wk1, wk2, dinv, scal;   // resid_i = max(k_ii - q_i, 0): with the bound only
};

// ================================================================================ kernels
// A[j][j] += v for j < n
__global__ __launch_bounds__(256) void ind_diag_add_kernel(double* __restrict__ A, long ld, long n, double v) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) A[j * ld + j] += v;
}
// out[j] = 2 log A[j][j] for j < n
__global__ __launch_bounds__(256) void ind_logdiag_kernel(const double* __restrict__ A, long ld, long n, double* __restrict__ out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = 2.0 * log(A[j * ld + j]);
}
// A wavefront per row of V^T (rows x ld, the padding columns zero): q = |row|^2, lambda = yerr^2 + phi max(kd - q, 0), the row
// scaled by lambda^-1/2 in place; lam and loglam per row.  The sum: lane-strided, then the wave tree.  With resid (the
// variational bound) max(kd - q, 0) stays out of lambda: resid and the term of tau, resid / lambda, per row.
__global__ __launch_bounds__(256) void ind_lambda_kernel(double* __restrict__ Vt, long ld, long rows, const double* __restrict__ yerr,
                                                         const double* __restrict__ kd, double* __restrict__ lam,
                                                         double* __restrict__ loglam, double* __restrict__ resid,
                                                         double* __restrict__ tauterm) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  double* v = Vt + row * ld;
  double q = 0.0;
  for (long j = lane; j < ld; j += 64) q += v[j] * v[j];
  q = __shfl(wave_sum(q), 0, 64);
  const double ye = yerr[row];
  double l = ye * ye;
  if (kd && !resid) l += fmax(kd[row] - q, 0.0);
  const double w = 1.0 / sqrt(l);
  for (long j = lane; j < ld; j += 64) v[j] *= w;
  if (lane == 0) { lam[row] = l; loglam[row] = log(l); }
  if (resid && lane == 0) { const double rv = fmax(kd[row] - q, 0.0); resid[row] = rv; tauterm[row] = rv / l; }
}
// R (se x rp) = Lambda^-1 b over the strip's rows (b: rows x nrhs), zero in the padding
__global__ __launch_bounds__(256) void ind_rhs_kernel(const double* __restrict__ b, long nrhs, const double* __restrict__ lam, long rows,
                                                      long se, long rp, double* __restrict__ R) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= se * rp) return;
  const long i = idx / rp, c = idx - i * rp;
  R[idx] = (i < rows && c < nrhs) ? b[i * nrhs + c] / lam[i] : 0.0;
}
// out (rows x nrhs) = R - Lambda^-1 D
__global__ __launch_bounds__(256) void ind_out_kernel(const double* __restrict__ R, const double* __restrict__ D, const double* __restrict__ lam,
                                                      long rows, long nrhs, long rp, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * nrhs) return;
  const long i = idx / nrhs, c = idx - i * nrhs;
  out[idx] = R[i * rp + c] - D[i * rp + c] / lam[i];
}
// the terms of b^T C^-1 b: vals[i] = b_i^2 / lambda_i (i < n), vals[n + j] = -t_j^2 (j < mp; t has the stride ts)
__global__ __launch_bounds__(256) void ind_quad_kernel(const double* __restrict__ b, const double* __restrict__ lam, long n,
                                                       const double* __restrict__ t, long ts, long mp, double* __restrict__ vals) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) vals[i] = b[i] * b[i] / lam[i];
  else if (i < n + mp) { const double tj = t[(i - n) * ts]; vals[i] = -tj * tj; }
}
// A wavefront per data point of the strip: diagA_i = alpha_i^2 - (1 / lambda_i - |H[:, i]|^2 / lambda_i^2) from row i of H^T.
// With resid (the variational bound): diagA_i += resid_i / lambda_i^2, the part of tau, and omega_i = -1 / lambda_i.
__global__ __launch_bounds__(256) void ind_diaga_kernel(const double* __restrict__ Ht, long ld, long rows, const double* __restrict__ lam,
                                                        const double* __restrict__ alpha, double* __restrict__ diagA,
                                                        const double* __restrict__ resid, double* __restrict__ omega) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  double hh = 0.0;
  for (long j = lane; j < ld; j += 64) { const double v = Ht[row * ld + j]; hh += v * v; }
  hh = wave_sum(hh);
  const double l = lam[row], a = alpha[row];
  if (lane == 0) {
    const double dA = a * a - (1.0 / l - hh / (l * l));
    diagA[row] = resid ? dA + resid[row] / (l * l) : dA;
    if (resid) omega[row] = -1.0 / l;
  }
}
// Y (se x ld; `rows` of them data points) holding H^T M1  <-  alpha_i w_j - Y_ij / lambda_i, the DTC part of Z^T; the rows past
// the data points stay zero
__global__ __launch_bounds__(256) void ind_zt_kernel(double* __restrict__ Y, long ld, long rows, const double* __restrict__ lam,
                                                     const double* __restrict__ alpha, const double* __restrict__ w, long ws) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * ld) return;
  const long i = idx / ld, j = idx - i * ld;
  Y[idx] = alpha[i] * w[j * ws] - Y[idx] / lam[i];
}
// The same Z^T for the gradient of the inducing inputs, from P itself: Zt (rows x ld) holding H^T G2, G2 = H Lambda^-1 P^T  <-
// alpha_i w_j - (Pt_ij - Zt_ij) / lambda_i - omega_i Pt_ij (omega == nullptr: DTC); w = P alpha with the stride ws
__global__ __launch_bounds__(256) void ind_zt_p_kernel(double* __restrict__ Zt, const double* __restrict__ Pt, long ld, long rows,
                                                       const double* __restrict__ lam, const double* __restrict__ alpha,
                                                       const double* __restrict__ omega, const double* __restrict__ w, long ws) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * ld) return;
  const long i = idx / ld, j = idx - i * ld;
  const double p = Pt[idx];
  double z = alpha[i] * w[j * ws] - (p - Zt[idx]) / lam[i];
  if (omega) z -= omega[i] * p;
  Zt[idx] = z;
}
// Leave-one-out, a wavefront per data point of the strip: c_i = (C^-1)_ii = 1 / lambda_i - |H[:, i]|^2 / lambda_i^2 from row i of
// H^T; resid = alpha / c, var = 1 / c, lpd = 1/2 log c - 1/2 alpha resid - 1/2 log 2 pi and, with w (the gradient path),
// w = 1/2 (1 + alpha resid) / c
__global__ __launch_bounds__(256) void ind_loo_point_kernel(const double* __restrict__ Ht, long ld, long rows, const double* __restrict__ lam,
                                                            const double* __restrict__ alpha, double* __restrict__ resid,
                                                            double* __restrict__ var, double* __restrict__ lpd, double* __restrict__ w) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  double hh = 0.0;
  for (long j = lane; j < ld; j += 64) { const double v = Ht[row * ld + j]; hh += v * v; }
  hh = wave_sum(hh);
  if (lane == 0) {
    const double l = lam[row], a = alpha[row];
    const double c = 1.0 / l - hh / (l * l), rs = a / c;
    resid[row] = rs;
    var[row] = 1.0 / c;
    lpd[row] = 0.5 * log(c) - 0.5 * a * rs - 0.918938533204672741780329736406;     // 1/2 log 2 pi
    if (w) w[row] = 0.5 * (1.0 + a * rs) / c;
  }
}
// A wavefront per data point of the strip: d2_i = (C^-1 diag(w) C^-1)_ii = w_i / lambda_i^2 - 2 w_i / lambda_i |R[:, i]|^2 +
// R[:, i] . (S R)[:, i] from rows i of R^T and R^T S (R = H Lambda^-1, S = R diag(w) R^T); diagB_i = alpha_i v_i - d2_i
__global__ __launch_bounds__(256) void ind_loo_diagb_kernel(const double* __restrict__ Rt, const double* __restrict__ RS, long ld, long rows,
                                                            const double* __restrict__ lam, const double* __restrict__ w,
                                                            const double* __restrict__ alpha, const double* __restrict__ v,
                                                            double* __restrict__ diagB) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  double rr = 0.0, rs = 0.0;
  for (long j = lane; j < ld; j += 64) { const double t = Rt[row * ld + j]; rr += t * t; rs += t * RS[row * ld + j]; }
  rr = wave_sum(rr);
  rs = wave_sum(rs);
  if (lane == 0) {
    const double wl = w[row] / lam[row];
    diagB[row] = alpha[row] * v[row] - ((wl / lam[row] - 2.0 * wl * rr) + rs);
  }
}
// Y (se x ld; `rows` of them data points) holding R^T (S G1 - G3), with RG = R^T G1 and Pt = P_J^T  <-  the leave-one-out Z^T:
// alpha_i pv_j + v_i pa_j - 2 (w_i / lambda_i^2 Pt_ij - w_i / lambda_i RG_ij + Y_ij) - 2 diagB_i Pt_ij (diagB == nullptr: DTC);
// pa = P alpha and pv = P v with the stride ws; the rows past the data points stay zero
__global__ __launch_bounds__(256) void ind_loo_zt_kernel(double* __restrict__ Y, const double* __restrict__ RG, const double* __restrict__ Pt, long ld,
                                                         long rows, const double* __restrict__ lam, const double* __restrict__ w,
                                                         const double* __restrict__ alpha, const double* __restrict__ v,
                                                         const double* __restrict__ diagB, const double* __restrict__ pa,
                                                         const double* __restrict__ pv, long ws) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * ld) return;
  const long i = idx / ld, j = idx - i * ld;
  const double wl = w[i] / lam[i], p = Pt[idx];
  double z = (alpha[i] * pv[j * ws] + v[i] * pa[j * ws]) - 2.0 * ((wl / lam[i] * p - wl * RG[idx]) + Y[idx]);
  if (diagB) z -= 2.0 * diagB[i] * p;
  Y[idx] = z;
}
// R (se x rp) = the vector a (rows entries) in column 0, zero elsewhere
__global__ __launch_bounds__(256) void ind_col_kernel(const double* __restrict__ a, long rows, long se, long rp, double* __restrict__ R) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= se * rp) return;
  const long i = idx / rp, c = idx - i * rp;
  R[idx] = (i < rows && c == 0) ? a[i] : 0.0;
}
// row i of V (rows x ld) divided by d[i]
__global__ __launch_bounds__(256) void ind_row_div_kernel(double* __restrict__ V, long ld, long rows, const double* __restrict__ d) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * ld) return;
  V[idx] /= d[idx / ld];
}
// row i of V (rows x ld) scaled by d[i]
__global__ __launch_bounds__(256) void ind_row_scale_kernel(double* __restrict__ V, long ld, long rows, const double* __restrict__ d) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * ld) return;
  V[idx] *= d[idx / ld];
}
// Ks = 1/2 (X + X^T), np x np
__global__ __launch_bounds__(256) void ind_sym_kernel(const double* __restrict__ X, long np, double* __restrict__ Ks) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= np * np) return;
  const long i = idx / np, j = idx - i * np;
  Ks[idx] = 0.5 * (X[idx] + X[j * np + i]);
}
// A wavefront per test point: mu = F_i . w and, with Vt, var = var (holding k**) - |Vt_i|^2 + |Ht_i|^2
__global__ __launch_bounds__(256) void ind_predict_rows_kernel(const double* __restrict__ F, const double* __restrict__ Vt,
                                                               const double* __restrict__ Ht, long ld, long rows, const double* __restrict__ w,
                                                               long ws, double* __restrict__ mu, double* __restrict__ var) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  double sm = 0.0, sv = 0.0, sh = 0.0;
  for (long j = lane; j < ld; j += 64) sm += F[row * ld + j] * w[j * ws];
  sm = wave_sum(sm);
  if (var) {
    for (long j = lane; j < ld; j += 64) { const double v = Vt[row * ld + j]; sv += v * v; }
    for (long j = lane; j < ld; j += 64) { const double v = Ht[row * ld + j]; sh += v * v; }
    sv = wave_sum(sv);
    sh = wave_sum(sh);
  }
  if (lane == 0) {
    mu[row] = sm;
    if (var) var[row] = (var[row] - sv) + sh;
  }
}

// The rectangular gradient reduction: partial[workgroup][p] = sum over the tile of Wt[i][j] dk(x1_i, x2_j)/dtheta_p -- 64 rows
// i (points of x1) by 64 columns j (points of x2), the weights read from the dense strip Wt (pitch ld).  DIAG: the pairs are
// (x1_i, x1_i) for the 64 x 64 points of the workgroup and the weight is wt_scale * Wt[i] (the FITC term 1/2 diagA_i dk_ii).
// One wavefront per workgroup, lane = column.  The gradient row of a pair, the lane's running sums and the evaluator's
// runtime-indexed temporaries sit in the lane's LDS area of gp doubles (gp odd: no bank conflicts) -- no scratch memory; lane p
// then adds the 64 lanes' sums of parameter p in lane order.  The evaluator's gradient is taken per pair, for every kernel (a
// program in fast form has its nodes too).
template <bool DIAG>
__global__ __launch_bounds__(IND_GT) void ind_grad_tile_kernel(const GhNode* __restrict__ prog, int n_nodes, int nd, int P, int gp,
                                                               const uint32_t* __restrict__ which, const double* __restrict__ x1, long n1,
                                                               const double* __restrict__ x2, long n2, const double* __restrict__ Wt, long ld,
                                                               double wt_scale, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double ism[];
  const int lane = threadIdx.x;
  double* const xr = ism;                                   // the tile's 64 rows of x1
  double* const xc = xr + IND_GT * nd;                      // lane's column point of x2
  double* const area = xc + IND_GT * nd;
  double* const g = area + lane * gp;
  double* const acc = g + P;
  double* const ws = acc + P;
  __builtin_assume(ws != nullptr);
  const long r0 = DIAG ? (long)blockIdx.x * IND_GT * IND_GT : (long)blockIdx.y * IND_GT;
  const long c = (long)blockIdx.x * IND_GT + lane;
  if (!DIAG) {
    for (int t = lane; t < IND_GT * nd; t += IND_GT) {
      const long r = r0 + t / nd;
      xr[t] = r < n1 ? x1[r * nd + (t % nd)] : 0.0;
    }
    for (int d = 0; d < nd; ++d) xc[lane * nd + d] = c < n2 ? x2[c * nd + d] : 0.0;
  }
  for (int p = 0; p < P; ++p) acc[p] = 0.0;
  __syncthreads();
  for (int rr = 0; rr < IND_GT; ++rr) {
    const long r = DIAG ? r0 + (long)rr * IND_GT + lane : r0 + rr;
    if (DIAG) {
      if (r < n1) {
        for (int d = 0; d < nd; ++d) xc[lane * nd + d] = x1[r * nd + d];
        gh_eval_grad(prog, n_nodes, &xc[lane * nd], &xc[lane * nd], g, ws);
        const double w = wt_scale * Wt[r];
        for (int p = 0; p < P; ++p) acc[p] += w * g[p];
      }
    } else if (r < n1 && c < n2) {
      gh_eval_grad(prog, n_nodes, &xr[rr * nd], &xc[lane * nd], g, ws);
      const double w = Wt[r * ld + c];
      for (int p = 0; p < P; ++p) acc[p] += w * g[p];
    }
  }
  __syncthreads();
  if (lane < P) {
    double s = 0.0;
    for (int q = 0; q < IND_GT; ++q) s += area[q * gp + P + lane];
    const long wg = DIAG ? (long)blockIdx.x : (long)blockIdx.y * gridDim.x + blockIdx.x;
    partial[wg * P + lane] = which[lane] ? s : 0.0;
  }
}

// ================================================================================ host side
static inline unsigned ind_blocks(size_t work) { return (unsigned)((work + 255) / 256); }
static inline unsigned ind_row_blocks(int64_t rows) { return (unsigned)((rows + 3) / 4); }
static inline size_t ind_sq(const gh_inducing* h) { return (size_t)h->mp * h->mp * sizeof(double); }

extern "C" int gh_inducing_create(const gh_inducing_opts* opts, gh_inducing** out) {
  if (!out || !opts) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (opts->method != 0 && opts->method != 1) { gh_set_error("the inducing-point solver takes method 0 (DTC) or 1 (FITC), not %d", (int)opts->method); return GH_ERR_BAD_ARG; }
  if (opts->strip_points < 0) { gh_set_error("strip_points must not be negative"); return GH_ERR_BAD_ARG; }
  if (opts->variational != 0 && opts->variational != 1) { gh_set_error("variational is 0 or 1, not %d", (int)opts->variational); return GH_ERR_BAD_ARG; }
  if (opts->variational && opts->method != 0) { gh_set_error("the variational bound goes with method 0 (DTC)"); return GH_ERR_BAD_ARG; }
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd inducing-point solver needs an MI355X"); return GH_ERR_HIP; }
  gh_inducing* h = new gh_inducing();
  h->opts = *opts;
  if (hipSetDevice(h->opts.device) != hipSuccess) { delete h; gh_set_error("cannot initialise HIP device %d", (int)opts->device); return GH_ERR_HIP; }
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  if (gh_shared_streams(h->opts.device, shq) && shq[0]) {
    h->shared_stream = true;
    h->st = shq[0];
  } else if ((gh_prime_device(h->opts.device), hipStreamCreate(&h->st)) != hipSuccess) {
    delete h; gh_set_error("cannot initialise HIP device %d", (int)opts->device); return GH_ERR_HIP;
  }
  *out = h;
  return GH_OK;
}
extern "C" void gh_inducing_destroy(gh_inducing* h) {
  if (!h) return;
  (void)hipSetDevice(h->opts.device);
  if (h->st) (void)hipStreamSynchronize(h->st);             // (pooled blocks may be re-acquired by another handle)
  if (h->st && !h->shared_stream) (void)hipStreamDestroy(h->st);
  delete h;
}
extern "C" int64_t gh_inducing_info(const gh_inducing* h) { return h ? h->info : 0; }
extern "C" int gh_inducing_trace_term(const gh_inducing* h, double* out) {
  if (!h || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (!h->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  *out = h->opts.variational ? h->tau : 0.0;
  return GH_OK;
}

static int ind_need(gh_inducing* h) {
  if (!h) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!h->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  GH_HIP(hipSetDevice(h->opts.device));
  return GH_OK;
}
// points per strip: the caller's, or what the byte budget holds; a multiple of 128, no more than `count` rounded up
static int64_t ind_strip_points(const gh_inducing* h, int64_t count) {
  int64_t s = h->opts.strip_points > 0 ? gh_round_up(h->opts.strip_points, GH_TILE)
                                       : std::max<int64_t>(GH_TILE, IND_STRIP_BYTES / (3 * 8 * h->mp) / GH_TILE * GH_TILE);
  return std::min<int64_t>(s, gh_round_up(count, GH_TILE));
}
// C (M x N, pitch ldc) = alpha op(A) op(B) + beta C; a_km: A(m, k) at A[m * lda + k], else at A[k * lda + m]; b_km: B(n, k) at
// B[n * ldb + k], else at B[k * ldb + n]
static int ind_mm(hipStream_t st, double* Cm, int64_t ldc, const double* A, int64_t lda, bool a_km, const double* B, int64_t ldb, bool b_km,
                  int64_t M, int64_t N, int64_t K, double alpha, double beta, bool khi_col = false, bool lower = false) {
  GhGemm g = gemm_desc(Cm, ldc, A, lda, a_km, B, ldb, b_km, M, N, K, alpha, beta);
  g.khi_col = khi_col;
  g.lower = lower;
  return gh_launch_gemm(g, st);
}
// F = K(p_J, u): cw points p (rows; the first argument) against the m inducing points, se x mp with zero padding
static int ind_build(const gh_inducing* h, const gh_kernel* k, const double* p, int64_t cw, int64_t se, double* F) {
  return gh_launch_kmat(k, p, cw, h->u.d(), h->m, nullptr, F, h->mp, se, h->mp, 0, 0, false, false, h->st);
}
// Linv <- the inverse of the factor of the symmetric A (mp x mp, destroyed); *word (device) receives the failing pivot
static int ind_factor(gh_inducing* h, double* A, long long* word) {
  return gh_chol_potrf_block(h->st, A, h->mp, h->mp, h->dinv.d(), word, 0);
}
static int ind_keep_kernel(gh_inducing* h, const gh_kernel* k) {
  if (h->kc.d_nodes) { (void)hipFree(h->kc.d_nodes); h->kc.d_nodes = nullptr; }
  h->kc.nodes = k->nodes;
  h->kc.ndim = k->ndim;
  h->kc.size = k->size;
  h->kc.fast = k->fast;
  h->kc.device = -1;
  return h->kc.upload();
}

extern "C" int gh_inducing_compute(gh_inducing* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                                   const double* u, int64_t m, double jitter, double* logdet_out) {
  if (!h || !k || !x || !yerr || !u || n <= 0 || n > 0x7ffffff0L || !(jitter >= 0.0)) { gh_set_error("bad argument to compute"); return GH_ERR_BAD_ARG; }
  h->computed = false;
  h->info = 0;
  if (m < 1 || m > IND_M_MAX) { gh_set_error("the inducing-point solver takes 1 <= m <= %d inducing points, not %lld", IND_M_MAX, (long long)m); return GH_ERR_BAD_ARG; }
  if (ndim != k->ndim || ndim < 1 || ndim > GH_MAX_NDIM) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_HIP(hipSetDevice(h->opts.device));
  GH_CHECK(k->upload());
  GH_CHECK(ind_keep_kernel(h, k));
  hipStream_t st = h->st;
  const int64_t mp = gh_round_up(m, GH_TILE);
  h->n = n; h->m = m; h->mp = mp; h->ndim = ndim;
  GH_CHECK(h->x.ensure((size_t)n * ndim * sizeof(double)));
  GH_CHECK(h->yerr.ensure((size_t)n * sizeof(double)));
  GH_CHECK(h->u.ensure((size_t)m * ndim * sizeof(double)));
  GH_CHECK(h->lam.ensure((size_t)n * sizeof(double)));
  const bool vfe = h->opts.variational != 0, diag = vfe || h->opts.method != 0;    // diag: the kernel diagonal is needed
  if (vfe) GH_CHECK(h->resid.ensure((size_t)n * sizeof(double)));
  GH_CHECK(h->vals.ensure((size_t)(n + mp) * sizeof(double)));
  for (GhBuf* b : {(GhBuf*)&h->Lui, (GhBuf*)&h->M1, (GhBuf*)&h->wk1, (GhBuf*)&h->wk2}) GH_CHECK(b->ensure(ind_sq(h)));
  GH_CHECK(h->dinv.ensure((size_t)mp * GH_TILE * sizeof(double)));
  GH_CHECK(h->scal.ensure(4 * sizeof(double)));
  GH_CHECK(gh_to_device(h->x.d(), x, (size_t)n * ndim, st));
  GH_CHECK(gh_to_device(h->yerr.d(), yerr, (size_t)n, st));
  GH_CHECK(gh_to_device(h->u.d(), u, (size_t)m * ndim, st));
  GH_HIP(hipMemsetAsync(h->scal.p, 0, 4 * sizeof(double), st));
  long long* const word_u = (long long*)(h->scal.d() + 1);  // the failure words of the two factorisations
  long long* const word_a = (long long*)(h->scal.d() + 2);
  double res[4] = {0.0, 0.0, 0.0, 0.0};

  // K_uu + jitter I = L_u L_u^T (the padding: the identity), Lui = L_u^-1
  GH_CHECK(gh_launch_kmat(k, h->u.d(), m, h->u.d(), m, nullptr, h->wk1.d(), mp, mp, mp, 0, 0, true, false, st));
  if (jitter > 0.0) hipLaunchKernelGGL(ind_diag_add_kernel, dim3(ind_blocks((size_t)m)), dim3(256), 0, st, h->wk1.d(), (long)mp, (long)m, jitter);
  GH_HIP(hipGetLastError());
  GH_CHECK(ind_factor(h, h->wk1.d(), word_u));
  GH_HIP(hipMemcpyAsync(res, h->scal.d(), 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  if (info_from_bits(res[1]) != 0) {
    h->info = info_from_bits(res[1]);
    gh_set_error("K_uu + jitter I is not positive definite at inducing point %lld", (long long)(h->info - 1));
    return GH_ERR_NOT_PD;
  }
  GH_CHECK(gh_chol_linv(st, h->wk1.d(), h->dinv.d(), mp, h->Lui.d()));

  // G = sum_J (Lambda_J^-1/2 V_J^T)^T (Lambda_J^-1/2 V_J^T) into wk2, strips ascending
  const int64_t s = ind_strip_points(h, n);
  GhPooledBuf sF, sV, kd, tauv;
  GH_CHECK(sF.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(sV.ensure((size_t)s * mp * sizeof(double)));
  if (diag) GH_CHECK(kd.ensure((size_t)s * sizeof(double)));
  if (vfe) GH_CHECK(tauv.ensure((size_t)n * sizeof(double)));
  GH_HIP(hipMemsetAsync(h->wk2.p, 0, ind_sq(h), st));
  for (int64_t j0 = 0; j0 < n; j0 += s) {
    const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
    const double* xj = h->x.d() + j0 * ndim;
    GH_CHECK(ind_build(h, k, xj, cw, se, sF.d()));
    GH_CHECK(ind_mm(st, sV.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, se, mp, mp, 1.0, 0.0, /* Lui is lower */ true));
    if (diag) GH_CHECK(gh_launch_kdiag(k, xj, xj, cw, kd.d(), st));
    hipLaunchKernelGGL(ind_lambda_kernel, dim3(ind_row_blocks(cw)), dim3(256), 0, st, sV.d(), (long)mp, (long)cw, (const double*)h->yerr.d() + j0,
                       (const double*)(diag ? kd.d() : nullptr), h->lam.d() + j0, h->vals.d() + j0,
                       vfe ? h->resid.d() + j0 : (double*)nullptr, vfe ? tauv.d() + j0 : (double*)nullptr);
    GH_HIP(hipGetLastError());
    GH_CHECK(ind_mm(st, h->wk2.d(), mp, sV.d(), mp, false, sV.d(), mp, false, mp, mp, se, 1.0, 1.0, false, /* lower */ true));
  }
  // A = I + G = L_A L_A^T;  log|C| = sum_i log lambda_i + 2 sum_j log (L_A)_jj
  hipLaunchKernelGGL(ind_diag_add_kernel, dim3(ind_blocks((size_t)mp)), dim3(256), 0, st, h->wk2.d(), (long)mp, (long)mp, 1.0);
  GH_HIP(hipGetLastError());
  GH_CHECK(ind_factor(h, h->wk2.d(), word_a));
  hipLaunchKernelGGL(ind_logdiag_kernel, dim3(ind_blocks((size_t)mp)), dim3(256), 0, st, (const double*)h->wk2.d(), (long)mp, (long)mp, h->vals.d() + n);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(h->vals.d(), n + mp, 1, h->scal.d(), st));
  if (vfe) GH_CHECK(gh_launch_kgrad_final(tauv.d(), n, 1, h->scal.d() + 3, st));       // tau = sum_i resid_i / lambda_i, fixed order
  // M1 = L_A^-1 L_u^-1
  GH_CHECK(gh_chol_linv(st, h->wk2.d(), h->dinv.d(), mp, h->wk1.d()));
  GH_CHECK(ind_mm(st, h->M1.d(), mp, h->wk1.d(), mp, true, h->Lui.d(), mp, false, mp, mp, mp, 1.0, 0.0));
  GH_HIP(hipMemcpyAsync(res, h->scal.d(), 4 * sizeof(double), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  if (info_from_bits(res[2]) != 0) {
    h->info = -info_from_bits(res[2]);
    gh_set_error("A = I + V Lambda^-1 V^T is not positive definite at pivot %lld", (long long)(-h->info - 1));
    return GH_ERR_NOT_PD;
  }
  h->logdet = res[0];
  h->tau = vfe ? res[3] : 0.0;
  if (logdet_out) *logdet_out = res[0];
  h->computed = true;
  return GH_OK;
}

// The solve on device memory: b (n, nrhs) row-major -> out (n, nrhs), or out == nullptr for c, t and w alone.  ctw receives
// c = K_uf Lambda^-1 b, t = M1 c = t(b) and w = M1^T t, each mp x rp with rp = nrhs rounded up to 128.
static int ind_apply(gh_inducing* h, const double* b, int64_t nrhs, double* out, GhBuf& ctw) {
  hipStream_t st = h->st;
  const int64_t n = h->n, mp = h->mp, nd = h->ndim, rp = gh_round_up(nrhs, GH_TILE), s = ind_strip_points(h, n);
  const size_t vec = (size_t)mp * rp;
  GhPooledBuf sF, sR, sD;
  GH_CHECK(sF.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(sR.ensure((size_t)s * rp * sizeof(double)));
  GH_CHECK(ctw.ensure(3 * vec * sizeof(double)));
  double* const c = ctw.d();
  double* const t = c + vec;
  double* const w = t + vec;
  GH_HIP(hipMemsetAsync(c, 0, vec * sizeof(double), st));
  for (int64_t j0 = 0; j0 < n; j0 += s) {
    const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
    GH_CHECK(ind_build(h, &h->kc, h->x.d() + j0 * nd, cw, se, sF.d()));
    hipLaunchKernelGGL(ind_rhs_kernel, dim3(ind_blocks((size_t)se * rp)), dim3(256), 0, st, b + j0 * nrhs, (long)nrhs, (const double*)h->lam.d() + j0,
                       (long)cw, (long)se, (long)rp, sR.d());
    GH_HIP(hipGetLastError());
    GH_CHECK(ind_mm(st, c, rp, sF.d(), mp, false, sR.d(), rp, false, mp, rp, se, 1.0, 1.0));
  }
  GH_CHECK(ind_mm(st, t, rp, h->M1.d(), mp, true, c, rp, false, mp, rp, mp, 1.0, 0.0));
  GH_CHECK(ind_mm(st, w, rp, h->M1.d(), mp, false, t, rp, false, mp, rp, mp, 1.0, 0.0));
  if (!out) return GH_OK;
  GH_CHECK(sD.ensure((size_t)s * rp * sizeof(double)));
  for (int64_t j0 = 0; j0 < n; j0 += s) {
    const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
    if (s < n) {                                            // (one strip: F and R are still the first pass's)
      GH_CHECK(ind_build(h, &h->kc, h->x.d() + j0 * nd, cw, se, sF.d()));
      hipLaunchKernelGGL(ind_rhs_kernel, dim3(ind_blocks((size_t)se * rp)), dim3(256), 0, st, b + j0 * nrhs, (long)nrhs,
                         (const double*)h->lam.d() + j0, (long)cw, (long)se, (long)rp, sR.d());
      GH_HIP(hipGetLastError());
    }
    GH_CHECK(ind_mm(st, sD.d(), rp, sF.d(), mp, true, w, rp, false, se, rp, mp, 1.0, 0.0));
    hipLaunchKernelGGL(ind_out_kernel, dim3(ind_blocks((size_t)cw * nrhs)), dim3(256), 0, st, (const double*)sR.d(), (const double*)sD.d(),
                       (const double*)h->lam.d() + j0, (long)cw, (long)nrhs, (long)rp, out + j0 * nrhs);
    GH_HIP(hipGetLastError());
  }
  return GH_OK;
}

extern "C" int gh_inducing_solve(gh_inducing* h, const double* b, int64_t nrhs, double* out) {
  GH_CHECK(ind_need(h));
  if (!b || !out || nrhs <= 0) { gh_set_error("bad argument to solve"); return GH_ERR_BAD_ARG; }
  const size_t tot = (size_t)h->n * nrhs;
  GhPooledBuf rhs, res, ctw;
  GH_CHECK(rhs.ensure(tot * sizeof(double)));
  GH_CHECK(res.ensure(tot * sizeof(double)));
  GH_CHECK(gh_to_device(rhs.d(), b, tot, h->st));
  GH_CHECK(ind_apply(h, rhs.d(), nrhs, res.d(), ctw));
  GH_CHECK(gh_from_device(out, res.d(), tot, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  return GH_OK;
}
extern "C" int gh_inducing_dot_solve(gh_inducing* h, const double* y, double* out) {
  GH_CHECK(ind_need(h));
  if (!y || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  const int64_t n = h->n, mp = h->mp;
  GhPooledBuf yd, ctw;
  GH_CHECK(yd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(yd.d(), y, (size_t)n, h->st));
  GH_CHECK(ind_apply(h, yd.d(), 1, nullptr, ctw));
  const double* t = ctw.d() + (size_t)mp * GH_TILE;
  hipLaunchKernelGGL(ind_quad_kernel, dim3(ind_blocks((size_t)(n + mp))), dim3(256), 0, h->st, (const double*)yd.d(), (const double*)h->lam.d(), (long)n,
                     t, (long)GH_TILE, (long)mp, h->vals.d());
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(h->vals.d(), n + mp, 1, h->scal.d(), h->st));     // sum_i b_i^2 / lambda_i - |t|^2, fixed order
  double v = 0.0;
  GH_HIP(hipMemcpyAsync(&v, h->scal.d(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  *out = v;
  return GH_OK;
}

// The reduction of the kernel gradient, for ind_grad_body and gh_inducing_loo: grad[p] = sum_J (sum_ij Z_J^T[i][j] dk(x_i, u_j) +
// scale sum_i wd_i dk(x_i, x_i)) + sum_jj' W_jj' dk(u_j, u_j') with W = -1/2 (ZF Lui^T) Lui, ZF = sum_J Z_J F_J in wk2.  The
// partial sums: one row per workgroup of a launch (part, reused launch after launch in stream order), then one row per launch
// (rows): the strips' rectangles and diagonals, and the K_uu term last.
struct IndRed {
  GhPooledBuf part, rows, zero, scratch;
  uint32_t* d_which = nullptr;
  double* partial = nullptr;
  int P = 0, gp = 0;
  size_t lds = 0;
  int64_t tiles_c = 0, nrows = 0;
};
// P = 0: no kernel gradient, the buffers at their smallest
static int ind_red_begin(gh_inducing* h, const uint32_t* which, int P, int64_t s, int64_t nstrips, IndRed& q) {
  const int64_t nd = h->ndim;
  const int Pw = P > 0 ? P : 1;
  q.P = P;
  GH_CHECK(q.zero.ensure((size_t)h->mp * sizeof(double)));
  q.tiles_c = (h->m + IND_GT - 1) / IND_GT;
  const int64_t tiles_r = (s + IND_GT - 1) / IND_GT;
  const size_t which_bytes = ((sizeof(uint32_t) * Pw + 15) / 16) * 16;
  GH_CHECK(q.part.ensure(which_bytes + (size_t)q.tiles_c * tiles_r * Pw * sizeof(double)));
  GH_CHECK(q.rows.ensure((size_t)(2 * nstrips + 2) * Pw * sizeof(double)));
  q.d_which = (uint32_t*)q.part.p;
  q.partial = (double*)((char*)q.part.p + which_bytes);
  if (P > 0) GH_HIP(hipMemcpyAsync(q.d_which, which, sizeof(uint32_t) * P, hipMemcpyHostToDevice, h->st));
  q.gp = (2 * P + GH_EVAL_WS) | 1;                          // doubles per lane: the gradient row, the sums, the evaluator's work space; odd
  q.lds = ((size_t)2 * IND_GT * nd + (size_t)IND_GT * q.gp) * sizeof(double);      // (at most 91 KB: 64 parameters, 16 dimensions)
  if (q.lds > 64 * 1024) {
    GH_HIP(hipFuncSetAttribute((const void*)ind_grad_tile_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, IND_GRAD_LDS));
    GH_HIP(hipFuncSetAttribute((const void*)ind_grad_tile_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, IND_GRAD_LDS));
  }
  GH_HIP(hipMemsetAsync(q.zero.p, 0, (size_t)h->mp * sizeof(double), h->st));
  return GH_OK;
}
// the strip's rectangle with the weights Zt (cw x mp) and, with wd, its diagonal term with the weights wd_scale * wd
static int ind_red_strip(gh_inducing* h, const gh_kernel* k, IndRed& q, const double* xj, int64_t cw, const double* Zt, const double* wd,
                         double wd_scale) {
  hipStream_t st = h->st;
  const int P = q.P;
  const dim3 grid((unsigned)q.tiles_c, (unsigned)((cw + IND_GT - 1) / IND_GT));
  hipLaunchKernelGGL(ind_grad_tile_kernel<false>, grid, dim3(IND_GT), q.lds, st, (const GhNode*)k->d_nodes, (int)k->nodes.size(), (int)h->ndim, P, q.gp,
                     (const uint32_t*)q.d_which, xj, (long)cw, (const double*)h->u.d(), (long)h->m, Zt, (long)h->mp, 1.0, q.partial);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(q.partial, (int64_t)grid.x * grid.y, P, q.rows.d() + q.nrows++ * P, st));
  if (wd) {
    const unsigned nwg = (unsigned)((cw + IND_GT * IND_GT - 1) / (IND_GT * IND_GT));
    hipLaunchKernelGGL(ind_grad_tile_kernel<true>, dim3(nwg), dim3(IND_GT), q.lds, st, (const GhNode*)k->d_nodes, (int)k->nodes.size(), (int)h->ndim, P,
                       q.gp, (const uint32_t*)q.d_which, xj, (long)cw, (const double*)nullptr, 0L, wd, 0L, wd_scale, q.partial);
    GH_HIP(hipGetLastError());
    GH_CHECK(gh_launch_kgrad_final(q.partial, nwg, P, q.rows.d() + q.nrows++ * P, st));
  }
  return GH_OK;
}
// the K_uu term from ZF in wk2 (Xb: an mp x mp work matrix), the sum over the launches, grad (host or device memory)
static int ind_red_end(gh_inducing* h, gh_kernel* k, const uint32_t* which, IndRed& q, double* Xb, double* grad) {
  hipStream_t st = h->st;
  const int64_t m = h->m, mp = h->mp;
  const int P = q.P;
  // W = -1/2 Z P^T = -1/2 (ZF Lui^T) Lui: the symmetric reduction with alpha = 0 and "K^-1" = -2 sym(W) = sym(ZF K_uu^-1)
  GH_CHECK(ind_mm(st, Xb, mp, h->wk2.d(), mp, true, h->Lui.d(), mp, true, mp, mp, mp, 1.0, 0.0, true));
  GH_CHECK(ind_mm(st, h->wk1.d(), mp, Xb, mp, true, h->Lui.d(), mp, false, mp, mp, mp, 1.0, 0.0));
  hipLaunchKernelGGL(ind_sym_kernel, dim3(ind_blocks((size_t)mp * mp)), dim3(256), 0, st, (const double*)h->wk1.d(), (long)mp, h->wk2.d());
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_reduce(k, which, h->u.d(), m, q.zero.d(), h->wk2.d(), mp, q.rows.d() + q.nrows++ * P, nullptr, q.scratch, st));
  GH_CHECK(gh_launch_kgrad_final(q.rows.d(), q.nrows, P, q.rows.d() + q.nrows * P, st));
  GH_CHECK(gh_from_device(grad, q.rows.d() + q.nrows * P, (size_t)P, st));
  return GH_OK;
}

// The body of gh_inducing_grad and gh_inducing_grad_u.  which == nullptr: no kernel gradient; ugrad == nullptr: no gradient of
// the inducing inputs (and then not one launch more than before).
// ugrad does not take the kernel gradient's Z_J^T and W: those are products with the explicit inverses M1 and Lui, whose single
// elements carry a relative error of eps cond(K_uu) -- harmless in sums over j against derivatives that are smooth in u_j, but
// ugrad is one row of Z and W per inducing input.  It takes them from P itself: a pass over the strips for
// G2 = H Lambda^-1 P^T = sum_J (Lambda_J^-1 H_J^T)^T P_J^T and w = P alpha = sum_J P_J alpha_J, then per strip
// Z_J^T = alpha_J w^T - Lambda_J^-1 (P_J^T - H_J^T G2) - diag(omega_J) P_J^T  (C^-1 = Lambda^-1 - Lambda^-1 H^T H Lambda^-1)
// and Z P^T = sum_J Z_J P_J^T = -2 W.
static int ind_grad_body(gh_inducing* h, gh_kernel* k, const uint32_t* which, const double* r, double* grad, double* alpha, double* diagA,
                         double* ugrad) {
  hipStream_t st = h->st;
  const int64_t n = h->n, m = h->m, mp = h->mp, nd = h->ndim, s = ind_strip_points(h, n), nstrips = (n + s - 1) / s;
  const int P = which ? k->size : 0;
  const bool vfe = h->opts.variational != 0, fitc = h->opts.method != 0 || vfe;    // fitc: Z has a diagonal part, of weight `wd`
  GhPooledBuf rd, al, dg, om, ug, upart, sP, sZ, aR, wp, Wa, ctw, sF, sY, sB, Xb;
  GH_CHECK(rd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(al.ensure((size_t)n * sizeof(double)));
  GH_CHECK(dg.ensure((size_t)n * sizeof(double)));
  if (vfe) GH_CHECK(om.ensure((size_t)n * sizeof(double)));
  const double* const wd = vfe ? om.d() : dg.d();           // omega: diagA (FITC) or -1 / lambda (the bound)
  if (ugrad) {
    GH_CHECK(ug.ensure((size_t)m * nd * sizeof(double)));
    // (the chunk count is not monotone in the row count: the full strip, the last strip and the K_uu term each have their own)
    const size_t need = std::max({gh_wxgrad_work_doubles(std::min<int64_t>(s, n), m, (int)nd), gh_wxgrad_work_doubles(n - (nstrips - 1) * s, m, (int)nd),
                                  gh_wxgrad_work_doubles(m, m, (int)nd)});
    GH_CHECK(upart.ensure(need * sizeof(double)));
    GH_CHECK(sP.ensure((size_t)s * mp * sizeof(double)));
    GH_CHECK(sZ.ensure((size_t)s * mp * sizeof(double)));
    GH_CHECK(aR.ensure((size_t)s * GH_TILE * sizeof(double)));
    GH_CHECK(wp.ensure((size_t)mp * GH_TILE * sizeof(double)));
    GH_CHECK(Wa.ensure(ind_sq(h)));
  }
  GH_CHECK(gh_to_device(rd.d(), r, (size_t)n, st));
  GH_CHECK(ind_apply(h, rd.d(), 1, al.d(), ctw));           // alpha = C^-1 r, and w = M1^T t(r) = P alpha
  const double* w = ctw.d() + 2 * (size_t)mp * GH_TILE;
  GH_CHECK(sF.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(sY.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(sB.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(Xb.ensure(ind_sq(h)));
  IndRed q;
  GH_CHECK(ind_red_begin(h, which, P, s, nstrips, q));
  double* const G2 = Xb.d();                                // (Xb is the kernel gradient's only after the strips)
  if (ugrad) {                                              // the pass for G2 and w = P alpha
    GH_HIP(hipMemsetAsync(Xb.p, 0, ind_sq(h), st));
    GH_HIP(hipMemsetAsync(Wa.p, 0, ind_sq(h), st));
    GH_HIP(hipMemsetAsync(wp.p, 0, (size_t)mp * GH_TILE * sizeof(double), st));
    for (int64_t j0 = 0; j0 < n; j0 += s) {
      const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
      GH_CHECK(ind_build(h, &h->kc, h->x.d() + j0 * nd, cw, se, sF.d()));
      GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, se, mp, mp, 1.0, 0.0, true));
      GH_CHECK(ind_mm(st, sP.d(), mp, sB.d(), mp, true, h->Lui.d(), mp, false, se, mp, mp, 1.0, 0.0));                          // P_J^T
      hipLaunchKernelGGL(ind_col_kernel, dim3(ind_blocks((size_t)se * GH_TILE)), dim3(256), 0, st, (const double*)al.d() + j0, (long)cw, (long)se,
                         (long)GH_TILE, aR.d());
      GH_HIP(hipGetLastError());
      GH_CHECK(ind_mm(st, wp.d(), GH_TILE, sP.d(), mp, false, aR.d(), GH_TILE, false, mp, GH_TILE, se, 1.0, 1.0));
      GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, se, mp, mp, 1.0, 0.0, true));                      // H_J^T
      hipLaunchKernelGGL(ind_row_div_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sB.d(), (long)mp, (long)cw, (const double*)h->lam.d() + j0);
      GH_HIP(hipGetLastError());
      GH_CHECK(ind_mm(st, G2, mp, sB.d(), mp, false, sP.d(), mp, false, mp, mp, se, 1.0, 1.0));
    }
  }
  // ZF = sum_J Z_J F_J into wk2
  GH_HIP(hipMemsetAsync(h->wk2.p, 0, ind_sq(h), st));
  for (int64_t j0 = 0; j0 < n; j0 += s) {
    const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
    const double* xj = h->x.d() + j0 * nd;
    GH_CHECK(ind_build(h, &h->kc, xj, cw, se, sF.d()));
    GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, se, mp, mp, 1.0, 0.0, /* M1 is lower */ true));      // H_J^T
    hipLaunchKernelGGL(ind_diaga_kernel, dim3(ind_row_blocks(cw)), dim3(256), 0, st, (const double*)sB.d(), (long)mp, (long)cw,
                       (const double*)h->lam.d() + j0, (const double*)al.d() + j0, dg.d() + j0,
                       vfe ? (const double*)h->resid.d() + j0 : (const double*)nullptr, vfe ? om.d() + j0 : (double*)nullptr);
    GH_HIP(hipGetLastError());
    GH_CHECK(ind_mm(st, sY.d(), mp, sB.d(), mp, true, h->M1.d(), mp, false, se, mp, mp, 1.0, 0.0));
    hipLaunchKernelGGL(ind_zt_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sY.d(), (long)mp, (long)cw, (const double*)h->lam.d() + j0,
                       (const double*)al.d() + j0, w, (long)GH_TILE);
    GH_HIP(hipGetLastError());
    if (fitc) {                                             // - diag(omega_J) P_J^T,  P_J^T = (F_J Lui^T) Lui
      GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, se, mp, mp, 1.0, 0.0, true));
      hipLaunchKernelGGL(ind_row_scale_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sB.d(), (long)mp, (long)cw, wd + j0);
      GH_HIP(hipGetLastError());
      GH_CHECK(ind_mm(st, sY.d(), mp, sB.d(), mp, true, h->Lui.d(), mp, false, se, mp, mp, -1.0, 1.0));
    }
    GH_CHECK(ind_mm(st, h->wk2.d(), mp, sY.d(), mp, false, sF.d(), mp, false, mp, mp, se, 1.0, 1.0));
    if (ugrad) {
      GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, se, mp, mp, 1.0, 0.0, true));
      GH_CHECK(ind_mm(st, sP.d(), mp, sB.d(), mp, true, h->Lui.d(), mp, false, se, mp, mp, 1.0, 0.0));                          // P_J^T
      GH_CHECK(ind_mm(st, sB.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, se, mp, mp, 1.0, 0.0, true));                      // H_J^T
      GH_CHECK(ind_mm(st, sZ.d(), mp, sB.d(), mp, true, G2, mp, false, se, mp, mp, 1.0, 0.0));                                  // H_J^T G2
      hipLaunchKernelGGL(ind_zt_p_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sZ.d(), (const double*)sP.d(), (long)mp, (long)cw,
                         (const double*)h->lam.d() + j0, (const double*)al.d() + j0, fitc ? wd + j0 : (const double*)nullptr, (const double*)wp.d(),
                         (long)GH_TILE);
      GH_HIP(hipGetLastError());
      GH_CHECK(gh_launch_wxgrad(k, h->u.d(), m, xj, cw, sZ.d(), mp, 1.0, j0 > 0, ug.d(), upart.d(), st));
      GH_CHECK(ind_mm(st, Wa.d(), mp, sZ.d(), mp, false, sP.d(), mp, false, mp, mp, se, 1.0, 1.0));                             // Z P^T += Z_J P_J^T
    }
    if (P > 0) GH_CHECK(ind_red_strip(h, k, q, xj, cw, sY.d(), fitc ? wd + j0 : nullptr, 0.5));
  }
  if (P > 0) GH_CHECK(ind_red_end(h, k, which, q, Xb.d(), grad));
  if (ugrad) {                                              // sG = 1/2 (Z P^T + its transpose) = -(W + W^T): ugrad_j += sum_b (W + W^T)_jb d1 k(u_j, u_b)
    double* const sG = Xb.d();
    hipLaunchKernelGGL(ind_sym_kernel, dim3(ind_blocks((size_t)mp * mp)), dim3(256), 0, st, (const double*)Wa.d(), (long)mp, sG);
    GH_HIP(hipGetLastError());
    GH_CHECK(gh_launch_wxgrad(k, h->u.d(), m, h->u.d(), m, sG, mp, -1.0, true, ug.d(), upart.d(), st));
    GH_CHECK(gh_from_device(ugrad, ug.d(), (size_t)m * nd, st));
  }
  if (alpha) GH_CHECK(gh_from_device(alpha, al.d(), (size_t)n, st));
  if (diagA) GH_CHECK(gh_from_device(diagA, dg.d(), (size_t)n, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_inducing_grad(gh_inducing* h, gh_kernel* k, const uint32_t* which, const double* r, double* grad, double* alpha,
                                double* diagA) {
  GH_CHECK(ind_need(h));
  if (!k || !which || !r || !grad) { gh_set_error("bad argument to grad"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (k->size > GH_MAX_GRAD) { gh_set_error("grad: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  GH_CHECK(k->upload());
  return ind_grad_body(h, k, which, r, grad, alpha, diagA, nullptr);
}
extern "C" int gh_inducing_grad_u(gh_inducing* h, gh_kernel* k, const uint32_t* which, const double* r, double* grad, double* alpha,
                                  double* diagA, double* ugrad) {
  if (!h) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!k || !r || !ugrad || (which && !grad)) { gh_set_error("bad argument to grad_u"); return GH_ERR_BAD_ARG; }
  if (!h->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (which && k->size > GH_MAX_GRAD) { gh_set_error("grad_u: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  GH_HIP(hipSetDevice(h->opts.device));
  GH_CHECK(k->upload());
  return ind_grad_body(h, k, which, r, grad, alpha, diagA, ugrad);
}

// Leave-one-out of the DTC / FITC density (include/george_amd.h has the formulas).  Per strip J: H_J^T = F_J M1^T, R_J^T =
// Lambda_J^-1 H_J^T and P_J^T = (F_J Lui^T) Lui.  The first pass gives c and the values from the rows of H_J^T and, with `which`,
// S = sum_J (diag(w_J) R_J^T)^T R_J^T, G1 = sum_J R_J P_J^T and G3 = sum_J (diag(w_J D_J) R_J^T)^T P_J^T; then v = C^-1 resid and
// P v by a second apply and Mx = S G1 - G3; the second pass gives diagB from R_J^T and R_J^T S, Z_J^T from P_J^T, R_J^T G1 and
// R_J^T Mx, and feeds the reduction of ind_grad_body.  With one strip the second pass keeps the first one's F, R^T and P^T.
extern "C" int gh_inducing_loo(gh_inducing* h, gh_kernel* k, const uint32_t* which, const double* r, double* lpd_sum, double* resid,
                               double* var, double* lpd, double* grad, double* v, double* diagB) {
  GH_CHECK(ind_need(h));
  if (!k || !r || !lpd_sum || !resid || !var || (which ? !grad : (grad || v || diagB))) { gh_set_error("bad argument to loo"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (which && k->size > GH_MAX_GRAD) { gh_set_error("loo: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  hipStream_t st = h->st;
  const int64_t n = h->n, mp = h->mp, nd = h->ndim, s = ind_strip_points(h, n), nstrips = (n + s - 1) / s;
  const bool fitc = h->opts.method != 0;                    // (the bound's solves and predictions are DTC's)
  // vals: r, alpha, resid, var, lpd and their sum; with the gradient also w, v and diagB
  GhPooledBuf vals, ctw, ctv, sF, sH, sP, sT, sY, mats;
  GH_CHECK(vals.ensure(((size_t)(which ? 8 : 5) * n + 1) * sizeof(double)));
  double* const rd = vals.d();
  double* const al = rd + n;
  double* const rs = al + n;
  double* const vr = rs + n;
  double* const lp = vr + n;
  double* const total = lp + n;
  double* const wv = which ? total + 1 : nullptr;
  double* const vv = which ? wv + n : nullptr;
  double* const db = which ? vv + n : nullptr;
  GH_CHECK(gh_to_device(rd, r, (size_t)n, st));
  GH_CHECK(ind_apply(h, rd, 1, al, ctw));                   // alpha = C^-1 r, and P alpha
  GH_CHECK(sF.ensure((size_t)s * mp * sizeof(double)));
  GH_CHECK(sH.ensure((size_t)s * mp * sizeof(double)));
  double *S = nullptr, *G1 = nullptr, *G3 = nullptr;
  if (which) {
    GH_CHECK(sP.ensure((size_t)s * mp * sizeof(double)));
    GH_CHECK(sT.ensure((size_t)s * mp * sizeof(double)));
    GH_CHECK(sY.ensure((size_t)s * mp * sizeof(double)));
    GH_CHECK(mats.ensure(3 * ind_sq(h)));
    S = mats.d();
    G1 = S + (size_t)mp * mp;
    G3 = G1 + (size_t)mp * mp;
    GH_HIP(hipMemsetAsync(mats.p, 0, 3 * ind_sq(h), st));
  }
  // F_J, R_J^T and P_J^T of the strip at j0 into sF, sH and sP (sT: work space)
  auto strip_factors = [&](int64_t j0, int64_t cw, int64_t se) -> int {
    GH_CHECK(ind_mm(st, sT.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, se, mp, mp, 1.0, 0.0, true));
    GH_CHECK(ind_mm(st, sP.d(), mp, sT.d(), mp, true, h->Lui.d(), mp, false, se, mp, mp, 1.0, 0.0));
    hipLaunchKernelGGL(ind_row_div_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sH.d(), (long)mp, (long)cw, (const double*)h->lam.d() + j0);
    GH_HIP(hipGetLastError());
    return GH_OK;
  };
  for (int64_t j0 = 0; j0 < n; j0 += s) {
    const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
    GH_CHECK(ind_build(h, &h->kc, h->x.d() + j0 * nd, cw, se, sF.d()));
    GH_CHECK(ind_mm(st, sH.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, se, mp, mp, 1.0, 0.0, /* M1 is lower */ true));      // H_J^T
    hipLaunchKernelGGL(ind_loo_point_kernel, dim3(ind_row_blocks(cw)), dim3(256), 0, st, (const double*)sH.d(), (long)mp, (long)cw,
                       (const double*)h->lam.d() + j0, (const double*)al + j0, rs + j0, vr + j0, lp + j0, which ? wv + j0 : (double*)nullptr);
    GH_HIP(hipGetLastError());
    if (!which) continue;
    GH_CHECK(strip_factors(j0, cw, se));
    GH_CHECK(ind_mm(st, G1, mp, sH.d(), mp, false, sP.d(), mp, false, mp, mp, se, 1.0, 1.0));
    GH_HIP(hipMemcpyAsync(sT.p, sH.p, (size_t)se * mp * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ind_row_scale_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sT.d(), (long)mp, (long)cw, (const double*)wv + j0);
    GH_HIP(hipGetLastError());
    GH_CHECK(ind_mm(st, S, mp, sT.d(), mp, false, sH.d(), mp, false, mp, mp, se, 1.0, 1.0));
    hipLaunchKernelGGL(ind_row_div_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sT.d(), (long)mp, (long)cw, (const double*)h->lam.d() + j0);
    GH_HIP(hipGetLastError());
    GH_CHECK(ind_mm(st, G3, mp, sT.d(), mp, false, sP.d(), mp, false, mp, mp, se, 1.0, 1.0));
  }
  GH_CHECK(gh_launch_kgrad_final(lp, n, 1, total, st));     // L = sum_i lpd_i, fixed order
  GH_HIP(hipMemcpyAsync(lpd_sum, total, sizeof(double), hipMemcpyDeviceToHost, st));
  GH_CHECK(gh_from_device(resid, rs, (size_t)n, st));
  GH_CHECK(gh_from_device(var, vr, (size_t)n, st));
  if (lpd) GH_CHECK(gh_from_device(lpd, lp, (size_t)n, st));
  if (which) {
    GH_CHECK(k->upload());
    const int P = k->size;
    GH_CHECK(ind_apply(h, rs, 1, vv, ctv));                 // v = C^-1 resid, and P v
    const double* pa = ctw.d() + 2 * (size_t)mp * GH_TILE;
    const double* pv = ctv.d() + 2 * (size_t)mp * GH_TILE;
    GH_CHECK(ind_mm(st, G3, mp, S, mp, true, G1, mp, false, mp, mp, mp, 1.0, -1.0));                                             // Mx = S G1 - G3
    IndRed q;
    GH_CHECK(ind_red_begin(h, which, P, s, nstrips, q));
    GH_HIP(hipMemsetAsync(h->wk2.p, 0, ind_sq(h), st));     // ZF = sum_J Z_J F_J into wk2
    for (int64_t j0 = 0; j0 < n; j0 += s) {
      const int64_t cw = std::min<int64_t>(s, n - j0), se = gh_round_up(cw, GH_TILE);
      const double* xj = h->x.d() + j0 * nd;
      if (s < n) {                                          // (one strip: F, R^T and P^T are still the first pass's)
        GH_CHECK(ind_build(h, &h->kc, xj, cw, se, sF.d()));
        GH_CHECK(ind_mm(st, sH.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, se, mp, mp, 1.0, 0.0, true));
        GH_CHECK(strip_factors(j0, cw, se));
      }
      GH_CHECK(ind_mm(st, sT.d(), mp, sH.d(), mp, true, S, mp, false, se, mp, mp, 1.0, 0.0));                                   // R_J^T S
      hipLaunchKernelGGL(ind_loo_diagb_kernel, dim3(ind_row_blocks(cw)), dim3(256), 0, st, (const double*)sH.d(), (const double*)sT.d(), (long)mp, (long)cw,
                         (const double*)h->lam.d() + j0, (const double*)wv + j0, (const double*)al + j0, (const double*)vv + j0, db + j0);
      GH_HIP(hipGetLastError());
      GH_CHECK(ind_mm(st, sY.d(), mp, sH.d(), mp, true, G3, mp, false, se, mp, mp, 1.0, 0.0));                                  // R_J^T Mx
      GH_CHECK(ind_mm(st, sT.d(), mp, sH.d(), mp, true, G1, mp, false, se, mp, mp, 1.0, 0.0));                                  // R_J^T G1
      hipLaunchKernelGGL(ind_loo_zt_kernel, dim3(ind_blocks((size_t)cw * mp)), dim3(256), 0, st, sY.d(), (const double*)sT.d(), (const double*)sP.d(),
                         (long)mp, (long)cw, (const double*)h->lam.d() + j0, (const double*)wv + j0, (const double*)al + j0, (const double*)vv + j0,
                         fitc ? (const double*)db + j0 : (const double*)nullptr, pa, pv, (long)GH_TILE);
      GH_HIP(hipGetLastError());
      GH_CHECK(ind_mm(st, h->wk2.d(), mp, sY.d(), mp, false, sF.d(), mp, false, mp, mp, se, 1.0, 1.0));
      if (P > 0) GH_CHECK(ind_red_strip(h, k, q, xj, cw, sY.d(), fitc ? db + j0 : nullptr, 1.0));
    }
    if (P > 0) GH_CHECK(ind_red_end(h, k, which, q, S, grad));                  // (S is free by now)
    if (v) GH_CHECK(gh_from_device(v, vv, (size_t)n, st));
    if (diagB) GH_CHECK(gh_from_device(diagB, db, (size_t)n, st));
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_inducing_predict(gh_inducing* h, gh_kernel* k, const double* r, const double* xs, int64_t M, double* mu, double* var,
                                   double* cov) {
  GH_CHECK(ind_need(h));
  if (!k || !r || !xs || !mu || M <= 0 || (var && cov) || M > 0x3fffffffL) { gh_set_error("bad argument to predict"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_CHECK(k->upload());
  hipStream_t st = h->st;
  const int64_t n = h->n, mp = h->mp, nd = h->ndim, Mp = gh_round_up(M, GH_TILE);
  if (cov) {
    const double need = 3.0 * 8.0 * (double)Mp * (double)mp + 8.0 * (double)Mp * (double)Mp;
    if (need > (double)IND_COV_BYTES) {
      gh_set_error("predict: the covariance keeps three M x m strips and the M x M result on the device, %.3g bytes for M = %lld, m = %lld, "
                   "over the budget of %ld; ask for the variance or for fewer test points at a time", need, (long long)M, (long long)h->m,
                   (long)IND_COV_BYTES);
      return GH_ERR_NOMEM;
    }
  }
  GhPooledBuf rd, ctw, xsd, sF, sV, sH, res, kss;
  GH_CHECK(rd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(rd.d(), r, (size_t)n, st));
  GH_CHECK(ind_apply(h, rd.d(), 1, nullptr, ctw));          // w = M1^T t(r):  mu = H*^T t(r) = F* w
  const double* w = ctw.d() + 2 * (size_t)mp * GH_TILE;
  const double* xs_dev = nullptr;
  GH_CHECK(gh_stage_points(xs, M, (int)nd, xsd, st, &xs_dev));
  const int64_t Ct = cov ? Mp : ind_strip_points(h, M);
  const bool second = var || cov;
  GH_CHECK(sF.ensure((size_t)Ct * mp * sizeof(double)));
  if (second) {
    GH_CHECK(sV.ensure((size_t)Ct * mp * sizeof(double)));
    GH_CHECK(sH.ensure((size_t)Ct * mp * sizeof(double)));
  }
  GH_CHECK(res.ensure((size_t)2 * M * sizeof(double)));
  double* dmu = res.d();
  double* dvar = dmu + M;
  if (var) GH_CHECK(gh_launch_kdiag(k, xs_dev, xs_dev, M, dvar, st));
  for (int64_t j0 = 0; j0 < M; j0 += Ct) {
    const int64_t cw = std::min<int64_t>(Ct, M - j0), ce = gh_round_up(cw, GH_TILE);
    GH_CHECK(ind_build(h, k, xs_dev + j0 * nd, cw, ce, sF.d()));
    if (second) {
      GH_CHECK(ind_mm(st, sV.d(), mp, sF.d(), mp, true, h->Lui.d(), mp, true, ce, mp, mp, 1.0, 0.0, true));
      GH_CHECK(ind_mm(st, sH.d(), mp, sF.d(), mp, true, h->M1.d(), mp, true, ce, mp, mp, 1.0, 0.0, true));
    }
    hipLaunchKernelGGL(ind_predict_rows_kernel, dim3(ind_row_blocks(cw)), dim3(256), 0, st, (const double*)sF.d(), (const double*)sV.d(),
                       (const double*)sH.d(), (long)mp, (long)cw, w, (long)GH_TILE, dmu + j0, var ? dvar + j0 : (double*)nullptr);
    GH_HIP(hipGetLastError());
  }
  GH_CHECK(gh_from_device(mu, dmu, (size_t)M, st));
  if (var) GH_CHECK(gh_from_device(var, dvar, (size_t)M, st));
  if (cov) {
    // cov = K(xs, xs) - V*^T V* + H*^T H* on the one strip of Mp rows
    GH_CHECK(kss.ensure((size_t)Mp * Mp * sizeof(double)));
    GH_CHECK(gh_launch_kmat(k, xs_dev, M, xs_dev, M, nullptr, kss.d(), Mp, Mp, Mp, 0, 0, true, false, st));
    GH_CHECK(ind_mm(st, kss.d(), Mp, sV.d(), mp, true, sV.d(), mp, true, Mp, Mp, mp, -1.0, 1.0));
    GH_CHECK(ind_mm(st, kss.d(), Mp, sH.d(), mp, true, sH.d(), mp, true, Mp, Mp, mp, 1.0, 1.0));
    GH_CHECK(gh_copy_rows(cov, M, kss.d(), Mp, M, M, false, st));
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}
