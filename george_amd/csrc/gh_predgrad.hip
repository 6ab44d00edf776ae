// gh_predgrad.hip -- input derivatives of the posterior mean and variance (gh_chol_predict_grad), the reduction.
//
// With G_cid = d k(t_c, x_i) / d t_cd (the evaluator's x1-gradient), alpha = K^-1 r and W = K^-1 K(x, t):
//     dmu_cd  = sum_i G_cid alpha_i
//     dvar_cd = D_cd - 2 sum_i G_cid W_ic,      D_cd = [x1-gradient + x2-gradient]_d of k at (t_c, t_c).
// The (M, N, ndim) tensor G is never stored: predgrad_kernel evaluates an element and adds it into the sums of its
// test point at once, predgrad_final_kernel adds the row chunks in index order.  No atomics: two calls give the same
// bits.  (No reference counterpart: src/george/gp.py stops at predict.)
//
// Tile: a workgroup of four wavefronts takes PG_COLS = 64 test points (one per lane) and one row chunk, PG_ROWS = 128
// training rows at a time.  The rows' coordinates and their alpha are staged in LDS once per workgroup; wavefront w
// takes rows w, w + 4, ... of the tile, so every W load of a wavefront is one row segment of 64 consecutive doubles.
// A lane keeps ndim (x 2 with the variance) running sums for its test point over all tiles of the chunk; the four
// wavefronts' sums meet in LDS in wavefront order and one partial row per (chunk, test point, d) is written.
// Rows >= n and test points >= m of the padded buffers are neither evaluated nor read.
//
// gh_launch_wxgrad is the same tile without the alpha operand: out_cd (+)= scale sum_i Wt[i][c] G_cid for a dense weight
// strip Wt, the chunks added in index order by wxgrad_final_kernel (the inducing-point solver's gradient with respect to
// its inducing inputs, gh_inducing_grad_u).
#include <algorithm>
#include "gh_common.h"

#define PG_COLS 64
#define PG_ROWS 128
#define PG_MAX_CHUNKS 64

struct PredGradArgs {
  const double* x; long n;            // training points (n, nd)
  const double* xs; long m;           // test points (m, nd)
  const double* alpha;                // (>= n)
  const double* W; long ldw;          // (>= n rows, pitch ldw >= m), or unused without VAR
  long rows_per;                      // rows of a chunk, a multiple of PG_ROWS
  double* pmu; double* pvar;          // partial rows (chunks, m, nd)
  int nd, n_nodes;
  GhFast fast;
};

// ND > 0: the fast form a + b F(r2) in ND input dimensions, registers only (gh_fast_xgrad); ND == 0: any kernel, through
// the interpreter (gh_eval_xgrad; its operand stacks and the sums live in scratch memory).  VAR = false: no W operand.
// MU = false (with VAR): no alpha operand and no pmu -- the weighted reduction of gh_launch_wxgrad, the same tile.
template <bool MU, bool VAR, int ND>
__global__ __launch_bounds__(256) void predgrad_kernel(PredGradArgs a, const GhNode* __restrict__ prog) {
  static_assert(MU || VAR, "a reduction without operands");
  constexpr int NA = ND > 0 ? ND : GH_MAX_NDIM;
  __shared__ double xr[PG_ROWS * NA];
  __shared__ double al[MU ? PG_ROWS : 1];
  __shared__ double xc[ND > 0 ? 1 : PG_COLS * GH_MAX_NDIM];
  __shared__ double red[VAR ? 2 : 1][3][PG_COLS];
  const int nd = ND > 0 ? ND : a.nd;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long c = (long)blockIdx.x * PG_COLS + lane;
  const bool live = c < a.m;
  const long r_begin = (long)blockIdx.y * a.rows_per;
  const long r_end = r_begin + a.rows_per < a.n ? r_begin + a.rows_per : a.n;

  double t[NA], am[NA], av[NA];
#pragma unroll
  for (int d = 0; d < NA; ++d) { t[d] = 0.0; am[d] = 0.0; av[d] = 0.0; }
  if (ND > 0) {
    if (live) {
#pragma unroll
      for (int d = 0; d < NA; ++d) t[d] = a.xs[c * ND + d];
    }
  } else {
    const long c0 = (long)blockIdx.x * PG_COLS;
    for (int e = threadIdx.x; e < PG_COLS * nd; e += 256) {
      const long cc = c0 + e / nd;
      xc[e] = cc < a.m ? a.xs[cc * nd + e % nd] : 0.0;
    }
  }

  for (long r0 = r_begin; r0 < r_end; r0 += PG_ROWS) {
    const int rows = (int)(r_end - r0 < PG_ROWS ? r_end - r0 : PG_ROWS);
    __syncthreads();                                    // the previous tile has been read (and xc is staged)
    for (int e = threadIdx.x; e < rows * nd; e += 256) xr[e] = a.x[r0 * nd + e];
    if (MU && (int)threadIdx.x < rows) al[threadIdx.x] = a.alpha[r0 + threadIdx.x];
    __syncthreads();
    if (!live) continue;
    for (int rr = wave; rr < rows; rr += 4) {
      const double ai = MU ? al[rr] : 0.0;
      double wi = 0.0;
      if (VAR) wi = a.W[(r0 + rr) * a.ldw + c];
      if (ND > 0) {
        double g[NA];
        gh_fast_xgrad<NA>(a.fast, t, &xr[rr * ND], g);
#pragma unroll
        for (int d = 0; d < NA; ++d) {
          if (MU) am[d] += g[d] * ai;
          if (VAR) av[d] += g[d] * wi;
        }
      } else {
        double g1[GH_MAX_NDIM], g2[GH_MAX_NDIM];
        gh_eval_xgrad(prog, a.n_nodes, nd, &xc[lane * nd], &xr[rr * nd], g1, g2);
        for (int d = 0; d < nd; ++d) {
          if (MU) am[d] += g1[d] * ai;
          if (VAR) av[d] += g1[d] * wi;
        }
      }
    }
  }

  // wavefronts 1 .. 3 hand their sums to wavefront 0, one component at a time; added in wavefront order
  for (int d = 0; d < nd; ++d) {
    double vm = 0.0, vv = 0.0;
#pragma unroll
    for (int e = 0; e < NA; ++e) { vm = (e == d) ? am[e] : vm; vv = (e == d) ? av[e] : vv; }
    __syncthreads();
    if (wave > 0) {
      if (MU) red[0][wave - 1][lane] = vm;
      if (VAR) red[VAR ? 1 : 0][wave - 1][lane] = vv;
    }
    __syncthreads();
    if (wave == 0 && live) {
      const long o = ((long)blockIdx.y * a.m + c) * nd + d;
      if (MU) a.pmu[o] = ((vm + red[0][0][lane]) + red[0][1][lane]) + red[0][2][lane];
      if (VAR) a.pvar[o] = ((vv + red[VAR ? 1 : 0][0][lane]) + red[VAR ? 1 : 0][1][lane]) + red[VAR ? 1 : 0][2][lane];
    }
  }
}

// dmu[c][d] = sum over the chunks, in index order; dvar[c][d] = D_cd - 2 (the same sum of pvar), D from the evaluator.
// One thread per test point.
__global__ __launch_bounds__(256) void predgrad_final_kernel(const GhNode* __restrict__ prog, int n_nodes, int nd, const double* xs, long m,
                                                             const double* pmu, const double* pvar, long nchunks,
                                                             double* dmu, double* dvar /* or NULL */) {
  const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  double g1[GH_MAX_NDIM], g2[GH_MAX_NDIM];
  if (dvar) gh_eval_xgrad(prog, n_nodes, nd, xs + c * nd, xs + c * nd, g1, g2);
  for (int d = 0; d < nd; ++d) {
    double sm = 0.0, sv = 0.0;
    for (long s = 0; s < nchunks; ++s) {
      sm += pmu[(s * m + c) * nd + d];
      if (dvar) sv += pvar[(s * m + c) * nd + d];
    }
    dmu[c * nd + d] = sm;
    if (dvar) dvar[c * nd + d] = (g1[d] + g2[d]) - 2.0 * sv;
  }
}

// out[c][d] = (add ? out[c][d] : 0) + scale * (the sum over the chunks, in index order).  One thread per entry.
__global__ __launch_bounds__(256) void wxgrad_final_kernel(const double* __restrict__ part, long entries, long nchunks, double scale,
                                                           int add, double* __restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  double s = 0.0;
  for (long q = 0; q < nchunks; ++q) s += part[q * entries + e];
  s *= scale;
  out[e] = add ? out[e] + s : s;
}

static void predgrad_chunks(int64_t n, int64_t* nchunks, int64_t* rows_per) {
  const int64_t tiles = (n + PG_ROWS - 1) / PG_ROWS;
  const int64_t per = (tiles + PG_MAX_CHUNKS - 1) / PG_MAX_CHUNKS;       // tiles of a chunk
  *nchunks = (tiles + per - 1) / per;
  *rows_per = per * PG_ROWS;
}
size_t gh_predgrad_work_doubles(int64_t n, int64_t m, int ndim, bool want_var) {
  int64_t nchunks, rows_per;
  predgrad_chunks(n, &nchunks, &rows_per);
  return (size_t)nchunks * m * ndim * (want_var ? 2 : 1);
}

// the tile kernel for k: the fast form's axes index the ND coordinates the kernel holds in registers (validated < ndim at creation)
template <bool MU, bool VAR>
static void predgrad_launch_tile(const gh_kernel* k, const PredGradArgs& a, dim3 grid, hipStream_t st) {
  const dim3 block(256);
  const GhNode* prog = k->d_nodes;
  const int fnd = (k->fast.ok && k->ndim <= 3) ? k->ndim : 0;
  if (fnd == 1)      hipLaunchKernelGGL((predgrad_kernel<MU, VAR, 1>), grid, block, 0, st, a, prog);
  else if (fnd == 2) hipLaunchKernelGGL((predgrad_kernel<MU, VAR, 2>), grid, block, 0, st, a, prog);
  else if (fnd == 3) hipLaunchKernelGGL((predgrad_kernel<MU, VAR, 3>), grid, block, 0, st, a, prog);
  else               hipLaunchKernelGGL((predgrad_kernel<MU, VAR, 0>), grid, block, 0, st, a, prog);
}

int gh_launch_predgrad(const gh_kernel* k, const double* x, int64_t n, const double* xs, int64_t m, const double* alpha,
                       const double* W, int64_t ldw, double* dmu, double* dvar, double* partial, hipStream_t st) {
  if (n <= 0 || m <= 0) return GH_OK;
  const bool var = dvar != nullptr;
  if (var && (!W || ldw < m)) { gh_set_error("predict_grad: the variance part needs W"); return GH_ERR_BAD_ARG; }
  int64_t nchunks, rows_per;
  predgrad_chunks(n, &nchunks, &rows_per);
  PredGradArgs a;
  a.x = x; a.n = (long)n; a.xs = xs; a.m = (long)m; a.alpha = alpha; a.W = var ? W : nullptr; a.ldw = (long)ldw;
  a.rows_per = (long)rows_per;
  a.pmu = partial; a.pvar = var ? partial + nchunks * m * k->ndim : nullptr;
  a.nd = k->ndim; a.n_nodes = (int)k->nodes.size(); a.fast = k->fast;
  const int64_t gx = (m + PG_COLS - 1) / PG_COLS;
  if (gx > 0x7fffffffL) { gh_set_error("predict_grad: too many test points"); return GH_ERR_BAD_ARG; }
  const dim3 grid((unsigned)gx, (unsigned)nchunks);
  if (var) predgrad_launch_tile<true, true>(k, a, grid, st); else predgrad_launch_tile<true, false>(k, a, grid, st);
  GH_HIP(hipGetLastError());
  hipLaunchKernelGGL(predgrad_final_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const GhNode*)k->d_nodes, a.n_nodes, k->ndim,
                     xs, (long)m, a.pmu, a.pvar, (long)nchunks, dmu, dvar);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

size_t gh_wxgrad_work_doubles(int64_t nx, int64_t nt, int ndim) { return gh_predgrad_work_doubles(nx, nt, ndim, false); }

int gh_launch_wxgrad(const gh_kernel* k, const double* t, int64_t nt, const double* x, int64_t nx, const double* Wt, int64_t ld,
                     double scale, bool add, double* out, double* partial, hipStream_t st) {
  if (nx <= 0 || nt <= 0) return GH_OK;
  if (!Wt || ld < nt) { gh_set_error("wxgrad: the weight strip has fewer columns than there are points t"); return GH_ERR_BAD_ARG; }
  int64_t nchunks, rows_per;
  predgrad_chunks(nx, &nchunks, &rows_per);
  PredGradArgs a;
  a.x = x; a.n = (long)nx; a.xs = t; a.m = (long)nt; a.alpha = nullptr; a.W = Wt; a.ldw = (long)ld;
  a.rows_per = (long)rows_per;
  a.pmu = nullptr; a.pvar = partial;
  a.nd = k->ndim; a.n_nodes = (int)k->nodes.size(); a.fast = k->fast;
  const int64_t gx = (nt + PG_COLS - 1) / PG_COLS;
  if (gx > 0x7fffffffL) { gh_set_error("wxgrad: too many points t"); return GH_ERR_BAD_ARG; }
  predgrad_launch_tile<false, true>(k, a, dim3((unsigned)gx, (unsigned)nchunks), st);
  GH_HIP(hipGetLastError());
  const long entries = (long)(nt * k->ndim);
  hipLaunchKernelGGL(wxgrad_final_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, (const double*)partial, entries, (long)nchunks,
                     scale, add ? 1 : 0, out);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
