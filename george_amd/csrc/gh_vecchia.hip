// gh_vecchia.hip -- the Vecchia (nearest-neighbour) solver behind gh_vecchia_* (include/george_amd.h has the definition)
//
// p(y) ~ prod_i p(y_i | y_c(i)), c(i) at most m <= 64 predecessors of i.  For every point the block A = K[c + {i}, c + {i}] (i last)
// is built from the kernel evaluator and factored; with v = L_cc^-1 k_ci:  f_i = k_ii - v^T v (the square of the block factor's last
// pivot) and b_i = L_cc^-T v.  Q = (I - B)^T F^-1 (I - B).  Local prediction (gh_vecchia_predict_local) puts a test point in the
// place of point i and its nearest data points in the place of c(i): the same block, mu = v^T L_cc^-1 r_c, var = k** - v^T v.
// The expected information of the hyper-parameters (gh_vecchia_fisher) is a sum over the same blocks: vecchia_fisher_kernel.
// So is the gradient of the leave-one-out score of this density (gh_vecchia_loo: c = diag Q, alpha = Q r): vecchia_loo_grad_kernel.
//
// Kernels: one point per 64-thread workgroup (one wavefront), lane s owns conditioning point s.  The point's coordinates, the lower
// triangle of A (packed by rows) and the evaluator's runtime-indexed temporaries sit in LDS: no kernel here uses scratch memory.
// Phases are separated by __syncthreads(); values cross lanes only through LDS or wave operations (readlane, shuffles).
// Every sum has a fixed order (wave trees, per-workgroup partials added by gh_launch_kgrad_final, gathers through the transposed
// index instead of floating-point atomics): two calls give the same bits.
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"
#include "gh_device_util.h"
#include "gh_vecchia_impl.h"

#define VWS (GH_EVAL_WS + 1)            // the evaluator's work space per lane, an odd pitch in doubles
#define V_GRAD_WGS 4096                 // workgroups of the gradient kernel (each walks points blockIdx.x, + gridDim.x, ..)
#define V_GRAD_LDS (96 * 1024)
#define V_FISHER_PLANES 64              // derivative planes of one call of the information kernel: one lane each
#define V_FISHER_LDS (128 * 1024)       // the raised limit of its dynamic LDS (119 KB at most)
#define V_STRIP_COLS 256                // test points per strip of predict (mean / variance) ..
#define V_STRIP_BYTES (1L << 30)        // .. within this many bytes for K(x, xs_J) and V together
#define V_COV_BYTES (8L << 30)          // what predict's covariance may keep on the device: K(x, xs), V and the m x m result
#define V_RED_ROWS 128                  // rows per chunk of the column reduction (at most V_RED_CHUNKS chunks)
#define V_RED_CHUNKS 2048

// the workgroup's LDS, in doubles from a 16-byte aligned base; gp = doubles per lane of the evaluator's area (0: none)
struct VLds {
  double *xs, *ye, *A, *dinv, *uv, *zv, *wl, *gl; int* gi;
};
__host__ __device__ static inline int v_tri(int j) { return j * (j + 1) / 2; }
__host__ __device__ static inline size_t v_lds_doubles(int m, int nd, int gp) {
  return (size_t)(m + 1) * nd + (m + 1) + v_tri(m + 1) + VM_MAX + 2 * (m + 1) + VM_MAX + (size_t)VM_MAX * gp + (m + 3) / 2;
}
__device__ __forceinline__ VLds v_carve(double* base, int m, int nd, int gp) {
  VLds l;
  l.xs = base;
  l.ye = l.xs + (m + 1) * nd;
  l.A = l.ye + (m + 1);
  l.dinv = l.A + v_tri(m + 1);
  l.uv = l.dinv + VM_MAX;
  l.zv = l.uv + (m + 1);
  l.wl = l.zv + (m + 1);
  l.gl = l.wl + VM_MAX;
  l.gi = (int*)(l.gl + VM_MAX * gp);
  return l;
}
__device__ __forceinline__ double v_bcast(double v, int src_lane) {           // src_lane: wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
// lane j < c holds t_j: L_cc^-1 t and L_cc^-T t with the factor of K_cc in A (dinv = 1 / its diagonal); lanes >= c keep t
__device__ __forceinline__ double v_fwd(const double* A, const double* dinv, int c, int lane, double t) {
  for (int k = 0; k < c; ++k) {
    const double vk = v_bcast(t, k) * dinv[k];
    if (lane == k) t = vk;
    else if (lane > k && lane < c) t -= A[v_tri(lane) + k] * vk;
  }
  return t;
}
__device__ __forceinline__ double v_bwd(const double* A, const double* dinv, int c, int lane, double t) {
  for (int k = c - 1; k >= 0; --k) {
    const double bk = v_bcast(t, k) * dinv[k];
    if (lane == k) t = bk;
    else if (lane < k) t -= A[v_tri(k) + lane] * bk;
  }
  return t;
}
// the kernel at block slots (j, k): the point with the lower index is the first argument (as gh_kmat.hip's symmetric build)
template <bool FAST>
__device__ __forceinline__ double v_value(const GhFast& fast, const GhNode* prog, int n_nodes, const double* x1, const double* x2,
                                          double* ws) {
  if (FAST) return gh_fast_value(fast, x1, x2);
  __builtin_assume(ws != nullptr);                          // (the evaluator then drops its private arrays: no scratch memory)
  return gh_eval_value(prog, n_nodes, x1, x2, ws);
}

// The three steps of a block, shared by the likelihood kernels (v_block) and by local prediction (vecchia_local_kernel).
// Stage: slots s < c take the data points row[s]; slot c -- the block's last row -- takes the point x_last with the error bar
// ye_last and the index g_last, which only orders the kernel's arguments (the point with the lower index comes first).
__device__ __forceinline__ void v_stage(const VArgs& a, const int* __restrict__ row, int c, int g_last, const double* __restrict__ x_last,
                                        double ye_last, const VLds& l, int lane) {
  const int nd = a.nd;
  for (int s = lane; s <= c; s += VM_MAX) {
    const int g = s < c ? row[s] : g_last;
    l.gi[s] = g;
    l.ye[s] = s < c ? a.yerr[g] : ye_last;
  }
  for (int t = lane; t < (c + 1) * nd; t += VM_MAX) {
    const int s = t / nd;
    l.xs[t] = s < c ? a.x[(long)row[s] * nd + (t - s * nd)] : x_last[t - s * nd];
  }
}
// Build: the entries t0 <= t < t1 of the packed lower triangle from one kernel, ye^2 added on the diagonal
template <bool FAST>
__device__ __forceinline__ void v_build(const GhFast& fast, const GhNode* prog, int n_nodes, const VLds& l, int nd, int t0, int t1,
                                        double* ws, int lane) {
  for (int t = t0 + lane; t < t1; t += VM_MAX) {
    int j, k;
    tri_index(t, j, k);
    const bool jlow = l.gi[j] <= l.gi[k];
    double v = v_value<FAST>(fast, prog, n_nodes, &l.xs[(jlow ? j : k) * nd], &l.xs[(jlow ? k : j) * nd], ws);
    if (j == k) v += l.ye[j] * l.ye[j];
    l.A[t] = v;
  }
}
// Factor: rows < c of A in place, left-looking, lane j owns row j; dinv = 1 / the factor's diagonal.  Returns false -- in every
// lane -- at a pivot that is not positive and finite.
__device__ __forceinline__ bool v_factor(const VLds& l, int c, int lane) {
  for (int k = 0; k < c; ++k) {
    double s = 0.0;
    if (lane >= k && lane < c) {
      const double* rj = l.A + v_tri(lane);
      const double* rk = l.A + v_tri(k);
      s = rj[k];
      for (int q = 0; q < k; ++q) s -= rj[q] * rk[q];
    }
    const double d = v_bcast(s, k);                         // the pivot, in every lane
    if (!(d > 0.0) || !isfinite(d)) return false;
    const double sd = sqrt(d), inv = 1.0 / sd;
    if (lane == k) { l.A[v_tri(k) + k] = sd; l.dinv[k] = inv; }
    else if (lane > k && lane < c) l.A[v_tri(lane) + k] = s * inv;
    __syncthreads();
  }
  return true;
}

// Point i: stage its block, build A, factor K_cc, then v, f and b.  Returns false -- in every lane -- when a pivot of K_cc or f
// is not positive and finite.  On return: c, this lane's b (lanes < c), f; in LDS the factor of K_cc (rows < c of A), dinv,
// k_ci and k_ii (row c of A), gi, xs, ye.
template <bool FAST>
__device__ __forceinline__ bool v_block(const VArgs& a, const GhFast& fast, const GhNode* prog, long i, const VLds& l, double* ws,
                                        int lane, int& c_out, double& b_out, double& f_out) {
  const int c = a.cnt[i];
  c_out = c;
  __syncthreads();                                          // (the previous point of this workgroup is done with the LDS)
  v_stage(a, a.nbr + i * a.m, c, (int)i, a.x + i * a.nd, a.yerr[i], l, lane);
  __syncthreads();
  v_build<FAST>(fast, prog, a.n_nodes, l, a.nd, 0, v_tri(c + 1), ws, lane);
  __syncthreads();
  if (!v_factor(l, c, lane)) return false;
  const double kci = lane < c ? l.A[v_tri(c) + lane] : 0.0;
  const double v = v_fwd(l.A, l.dinv, c, lane, kci);
  const double f = l.A[v_tri(c) + c] - v_bcast(wave_sum(lane < c ? v * v : 0.0), 0);
  f_out = f;
  if (!(f > 0.0) || !isfinite(f)) return false;
  b_out = v_bwd(l.A, l.dinv, c, lane, v);
  return true;
}

template <bool FAST>
__global__ __launch_bounds__(VM_MAX) void vecchia_factor_kernel(VArgs a, GhFast fast, const GhNode* __restrict__ prog,
                                                                double* __restrict__ B, double* __restrict__ f,
                                                                double* __restrict__ logf, int* fail) {
  extern __shared__ __attribute__((aligned(16))) double vsm[];
  const int lane = threadIdx.x;
  const VLds l = v_carve(vsm, a.m, a.nd, FAST ? 0 : VWS);
  const long i = blockIdx.x;
  int c = 0;
  double b = 0.0, fi = 1.0;
  const bool ok = v_block<FAST>(a, fast, prog, i, l, FAST ? nullptr : l.gl + lane * VWS, lane, c, b, fi);
  if (lane < a.m) B[i * a.m + lane] = (ok && lane < c) ? b : 0.0;
  if (lane == 0) {
    f[i] = ok ? fi : 1.0;
    logf[i] = ok ? log(fi) : 0.0;
    if (!ok) atomicMin(fail, (int)i);                       // the lowest failing point
  }
}

// Local prediction: test point t conditioned on the c data points of its row of the query table (valid entries first), one
// test point per workgroup.  The test point is the block's last row: rows < c are K_cc + yerr^2 from the data kernel, row c is
// k_c = k(x_j, t) and k** = k(t, t) from the cross kernel (its index INT_MAX puts the data point first).  With v = L^-1 k_c and
// w = L^-1 r_c:  mu = v^T w,  var = k** - v^T v.  c == 0: mu = 0, var = k**.  A pivot that is not positive and finite, or a
// variance that is not finite, records the test point in *fail (the lowest one) and writes zeros.
template <bool FAST>
__global__ __launch_bounds__(VM_MAX) void vecchia_local_kernel(VArgs a, GhFast fast_d, const GhNode* __restrict__ prog_d, GhFast fast_c,
                                                               const GhNode* __restrict__ prog_c, int n_nodes_c,
                                                               const double* __restrict__ r, const double* __restrict__ xs,
                                                               const int* __restrict__ qtab, const int* __restrict__ qcnt, int mq,
                                                               double* __restrict__ mu, double* __restrict__ var, int* fail) {
  extern __shared__ __attribute__((aligned(16))) double vsm[];
  const int lane = threadIdx.x, nd = a.nd;
  const VLds l = v_carve(vsm, mq, nd, FAST ? 0 : VWS);
  double* const ws = FAST ? nullptr : l.gl + lane * VWS;
  const long t = blockIdx.x;
  const int c = qcnt[t];
  v_stage(a, qtab + t * mq, c, INT_MAX, xs + t * nd, 0.0, l, lane);
  __syncthreads();
  v_build<FAST>(fast_d, prog_d, a.n_nodes, l, nd, 0, v_tri(c), ws, lane);
  v_build<FAST>(fast_c, prog_c, n_nodes_c, l, nd, v_tri(c), v_tri(c + 1), ws, lane);
  __syncthreads();
  bool ok = v_factor(l, c, lane);
  double m_t = 0.0, v_t = 0.0;
  if (ok) {
    const double v = v_fwd(l.A, l.dinv, c, lane, lane < c ? l.A[v_tri(c) + lane] : 0.0);
    const double w = v_fwd(l.A, l.dinv, c, lane, lane < c ? r[l.gi[lane]] : 0.0);
    m_t = wave_sum(lane < c ? v * w : 0.0);                 // (lane 0 has the sums)
    v_t = l.A[v_tri(c) + c] - wave_sum(lane < c ? v * v : 0.0);
  }
  if (lane == 0) {
    ok = ok && isfinite(v_t);
    mu[t] = ok ? m_t : 0.0;
    if (var) var[t] = ok ? v_t : 0.0;
    if (!ok) atomicMin(fail, (int)t);
  }
}

// The weighted triangle walk both gradient kernels end a block with:  acc_p += sum_jk W_jk dA_jk/dtheta_p  for the block that
// v_block left in LDS and  W = ca u u^T + cb (z u^T + u z^T),  u and z in l.uv and l.zv (c + 1 entries each, written before
// the barrier that precedes the call).  The lower triangle of the block goes through the evaluator 64 entries at a time (lane
// t: gradient row into its LDS area g, weight into wl); then lane p adds the 64 rows' entry p in order: the sum of a parameter
// lives in ONE lane, in one register.
__device__ __forceinline__ double v_walk(const VArgs& a, const GhNode* __restrict__ prog, const VLds& l, int P, int gp, int c, double ca,
                                         double cb, double* g, double* ws, int lane, double acc) {
  const int nd = a.nd, T = v_tri(c + 1);
  for (int t0 = 0; t0 < T && P > 0; t0 += VM_MAX) {
    const int t = t0 + lane, nact = T - t0 < VM_MAX ? T - t0 : VM_MAX;
    if (t < T) {
      int j, k;
      tri_index(t, j, k);
      const double uj = l.uv[j], uk = l.uv[k];
      const double w = ca * uj * uk + cb * (l.zv[j] * uk + uj * l.zv[k]);
      const bool jlow = l.gi[j] <= l.gi[k];
      gh_eval_grad(prog, a.n_nodes, &l.xs[(jlow ? j : k) * nd], &l.xs[(jlow ? k : j) * nd], g, ws);
      l.wl[lane] = j == k ? w : 2.0 * w;
    }
    __syncthreads();
    if (lane < P)
      for (int q = 0; q < nact; ++q) acc += l.wl[q] * l.gl[q * gp + lane];
    __syncthreads();
  }
  return acc;
}

// The likelihood gradient, block by block.  With e = r_i - b^T r_c, z = K_cc^-1 r_c, u = [-b; 1], ze = [z; 0]:
//   W = 1/2 (e^2/f^2 - 1/f) u u^T + 1/2 (e/f) (ze u^T + u ze^T),    d log p(y_i | y_c) / dtheta = sum_jk W_jk dA_jk/dtheta
// (v_walk).  partial[workgroup][p]; wd[i][s] = 2 W_ss for slot s (slot m: the point itself).
template <bool FAST>
__global__ __launch_bounds__(VM_MAX) void vecchia_grad_kernel(VArgs a, GhFast fast, const GhNode* __restrict__ prog, int P, int gp,
                                                              const uint32_t* __restrict__ which, const double* __restrict__ r,
                                                              double* __restrict__ partial, double* __restrict__ wd) {
  extern __shared__ __attribute__((aligned(16))) double vsm[];
  const int lane = threadIdx.x, nd = a.nd;
  const VLds l = v_carve(vsm, a.m, nd, gp);
  double* const g = l.gl + lane * gp;
  double* const ws = g + P;
  __builtin_assume(ws != nullptr);
  double acc = 0.0;
  for (long i = blockIdx.x; i < a.n; i += gridDim.x) {
    int c = 0;
    double b = 0.0, f = 1.0;
    const bool ok = v_block<FAST>(a, fast, prog, i, l, ws, lane, c, b, f);
    if (!ok) {                                              // (compute() has refused such a point: only with another kernel)
      for (int s = lane; s <= a.m; s += VM_MAX) wd[i * (a.m + 1) + s] = 0.0;
      continue;
    }
    const double rc = lane < c ? r[l.gi[lane]] : 0.0;
    const double e = r[i] - v_bcast(wave_sum(lane < c ? b * rc : 0.0), 0);
    const double z = v_bwd(l.A, l.dinv, c, lane, v_fwd(l.A, l.dinv, c, lane, rc));
    const double ca = 0.5 * (e * e / (f * f) - 1.0 / f), cb = 0.5 * e / f;
    if (lane < c) { l.uv[lane] = -b; l.zv[lane] = z; }
    if (lane == 0) { l.uv[c] = 1.0; l.zv[c] = 0.0; }
    if (lane < a.m) wd[i * (a.m + 1) + lane] = lane < c ? 2.0 * (ca * b * b - 2.0 * cb * z * b) : 0.0;
    if (lane == 0) wd[i * (a.m + 1) + a.m] = 2.0 * ca;
    __syncthreads();
    acc = v_walk(a, prog, l, P, gp, c, ca, cb, g, ws, lane, acc);
  }
  if (lane < P) partial[(long)blockIdx.x * P + lane] = which[lane] ? acc : 0.0;
}

// The gradient of the leave-one-out score L = sum_j lpd_j of the Vecchia density, block by block.  With Q = sum_i u u^T / f,
// c = diag Q, alpha = Q r, wv = 1/2 (1 + alpha^2 / c) / c and av = alpha / c:  dL = sum_i d[u^T M u / f] with
// M = diag(wv) - 1/2 (av r^T + r av^T) restricted to the block.  g = M u takes this lane's wv, av, r, u and the two wave sums
// u.r and u.av; h = A^-1 g by the partitioned inverse (h_last = u.g / f, h_c = K_cc^-1 g_c - b h_last: only the factor of K_cc
// that v_block leaves), and
//   W = (u.g / f^2) u u^T - (1/f) (h u^T + u h^T),    dL/dtheta = sum_i sum_jk W_jk dA_jk/dtheta    (v_walk; z = h, z[c] = h_last).
// partial[workgroup][p]; wd[i][s] = W_ss for slot s (slot m: the point itself).
template <bool FAST>
__global__ __launch_bounds__(VM_MAX) void vecchia_loo_grad_kernel(VArgs a, GhFast fast, const GhNode* __restrict__ prog, int P, int gp,
                                                                  const uint32_t* __restrict__ which, const double* __restrict__ r,
                                                                  const double* __restrict__ wv, const double* __restrict__ av,
                                                                  double* __restrict__ partial, double* __restrict__ wd) {
  extern __shared__ __attribute__((aligned(16))) double vsm[];
  const int lane = threadIdx.x;
  const VLds l = v_carve(vsm, a.m, a.nd, gp);
  double* const g = l.gl + lane * gp;
  double* const ws = g + P;
  __builtin_assume(ws != nullptr);
  double acc = 0.0;
  for (long i = blockIdx.x; i < a.n; i += gridDim.x) {
    int c = 0;
    double b = 0.0, f = 1.0;
    const bool ok = v_block<FAST>(a, fast, prog, i, l, ws, lane, c, b, f);
    if (!ok) {                                              // (as the likelihood gradient: only with another kernel)
      for (int s = lane; s <= a.m; s += VM_MAX) wd[i * (a.m + 1) + s] = 0.0;
      continue;
    }
    const long gj = lane < c ? (long)l.gi[lane] : i;        // (lanes >= c read the point itself and use none of it)
    const double rj = r[gj], aj = av[gj], wj = wv[gj];
    const double ri = r[i], ai = av[i];
    const double ur = ri - v_bcast(wave_sum(lane < c ? b * rj : 0.0), 0);
    const double ua = ai - v_bcast(wave_sum(lane < c ? b * aj : 0.0), 0);
    const double gc = lane < c ? -wj * b - 0.5 * (aj * ur + rj * ua) : 0.0;
    const double ug = (wv[i] - 0.5 * (ai * ur + ri * ua)) - v_bcast(wave_sum(lane < c ? b * gc : 0.0), 0);
    const double hl = ug / f;
    const double h = v_bwd(l.A, l.dinv, c, lane, v_fwd(l.A, l.dinv, c, lane, gc)) - b * hl;
    const double ca = hl / f, cb = -1.0 / f;
    if (lane < c) { l.uv[lane] = -b; l.zv[lane] = h; }
    if (lane == 0) { l.uv[c] = 1.0; l.zv[c] = hl; }
    if (lane < a.m) wd[i * (a.m + 1) + lane] = lane < c ? ca * b * b - 2.0 * cb * h * b : 0.0;
    if (lane == 0) wd[i * (a.m + 1) + a.m] = ca + 2.0 * cb * hl;
    __syncthreads();
    acc = v_walk(a, prog, l, P, gp, c, ca, cb, g, ws, lane, acc);
  }
  if (lane < P) partial[(long)blockIdx.x * P + lane] = which[lane] ? acc : 0.0;
}

// The expected (Fisher) information of the Vecchia likelihood, block by block (Guinness 2021).  A derivative plane D_a restricted
// to the block -- diag(s_a) of a diagonal parameter, or dA/dtheta_a of a kernel parameter -- gives, with u = [-b; 1]:
//   v_a = D_a u,   df_a = u^T v_a,   w_a = L_cc^-1 (v_a)[:c],   F_ab += 1/2 df_a df_b / f^2 + (w_a . w_b) / f.
// The workgroup's LDS continues behind v_lds_doubles(m, nd, gp) with the plane area V (Q rows of pitch pw, row a = v_a and then
// w_a), the Q values df_a and the packed pairs a <= b (gh_fisher_pair), which stay there for the whole kernel.
__host__ __device__ static inline int v_fisher_pitch(int m) { return (m + 1) | 1; }     // odd: lane a walks row a
__host__ __device__ static inline size_t v_fisher_lds_doubles(int m, int nd, int gp, int Q) {
  return v_lds_doubles(m, nd, gp) + (size_t)Q * v_fisher_pitch(m) + VM_MAX + (size_t)Q * (Q + 1) / 2;
}
// lanes j < c hold t[e]_j for NP planes at once: v_fwd on each, the steps interleaved
template <int NP>
__device__ __forceinline__ void v_fwd_n(const double* A, const double* dinv, int c, int lane, double (&t)[NP]) {
  for (int k = 0; k < c; ++k) {
    const double dk = dinv[k];
    const double ajk = (lane > k && lane < c) ? A[v_tri(lane) + k] : 0.0;
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      const double vk = v_bcast(t[e], k) * dk;
      if (lane == k) t[e] = vk;
      else if (lane > k && lane < c) t[e] -= ajk * vk;
    }
  }
}
// One lane, one kernel plane: the nact entries of the packed triangle from (j, k) on, whose gradient rows lie gp apart in g (this
// lane's parameter first), added into the lane's row of V in their order.  row[j] of the running row j stays in a register.
__device__ __forceinline__ void v_fisher_sweep(double* __restrict__ row, const double* __restrict__ g, const double* __restrict__ u,
                                               int gp, int nact, int j, int k) {
  int q = 0;
  while (q < nact) {
    const int run = min(nact - q, j - k + 1), off = min(run, j - k);      // entries left in row j; those below the diagonal
    const double uj = u[j];
    double rj = row[j];
#pragma unroll 4
    for (int e = 0; e < off; ++e) {
      const double ge = g[(q + e) * gp];
      rj += ge * u[k + e];
      row[k + e] += ge * uj;
    }
    if (off < run) rj += g[(q + off) * gp] * uj;                          // (j, j)
    row[j] = rj;
    q += run;
    k += run;
    if (k > j) { ++j; k = 0; }
  }
}
// Plane a < n_diag is diag(diag_rows[a]) (row a of an (n_diag, n) array), plane a >= n_diag is the kernel parameter
// kpar[a - n_diag]; Q planes in all, at most 64.  Lane a owns row a of V while the planes are built, lane j owns slot j during
// the substitution, and lane b owns the pairs (a, b), a <= b, for the whole kernel.  partial[workgroup][pair].
template <bool FAST>
__global__ __launch_bounds__(VM_MAX) void vecchia_fisher_kernel(VArgs a, GhFast fast, const GhNode* __restrict__ prog, int P, int gp,
                                                                int Q, int n_diag, const int* __restrict__ kpar,
                                                                const double* __restrict__ diag_rows, double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double vsm[];
  const int lane = threadIdx.x, nd = a.nd, pw = v_fisher_pitch(a.m), npair = Q * (Q + 1) / 2;
  const VLds l = v_carve(vsm, a.m, nd, gp);
  double* const g = l.gl + lane * gp;
  double* const ws = g + P;
  __builtin_assume(ws != nullptr);
  double* const V = vsm + v_lds_doubles(a.m, nd, gp);
  double* const dfv = V + Q * pw;
  double* const Fp = dfv + VM_MAX;
  double* const row = V + (lane < Q ? lane : 0) * pw;
  const int kp = (lane >= n_diag && lane < Q) ? kpar[lane - n_diag] : -1;
  for (int p = lane; p < npair; p += VM_MAX) Fp[p] = 0.0;
  __syncthreads();
  for (long i = blockIdx.x; i < a.n; i += gridDim.x) {
    int c = 0;
    double b = 0.0, f = 1.0;
    if (!v_block<FAST>(a, fast, prog, i, l, ws, lane, c, b, f)) continue;     // (as the gradient: such a point adds nothing)
    if (lane < c) l.uv[lane] = -b;
    if (lane == 0) l.uv[c] = 1.0;
    __syncthreads();
    if (lane < n_diag)
      for (int j = 0; j <= c; ++j) row[j] = diag_rows[(long)lane * a.n + l.gi[j]] * l.uv[j];
    else if (lane < Q)
      for (int j = 0; j <= c; ++j) row[j] = 0.0;
    const int T = v_tri(c + 1);
    for (int t0 = 0; t0 < T && Q > n_diag; t0 += VM_MAX) {
      const int t = t0 + lane, nact = T - t0 < VM_MAX ? T - t0 : VM_MAX;
      if (t < T) {
        int j, k;
        tri_index(t, j, k);
        const bool jlow = l.gi[j] <= l.gi[k];
        gh_eval_grad(prog, a.n_nodes, &l.xs[(jlow ? j : k) * nd], &l.xs[(jlow ? k : j) * nd], g, ws);
      }
      __syncthreads();
      if (kp >= 0) {
        int j0, k0;
        tri_index(t0, j0, k0);
        v_fisher_sweep(row, l.gl + kp, l.uv, gp, nact, j0, k0);
      }
      __syncthreads();
    }
    __syncthreads();
    // df_a and w_a, four planes at a time: lane j has slot j
    for (int a0 = 0; a0 < Q; a0 += 4) {
      double t[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        t[e] = (a0 + e < Q && lane < c) ? V[(a0 + e) * pw + lane] : 0.0;
        const double s = wave_sum(lane < c ? -b * t[e] : 0.0);
        if (lane == 0 && a0 + e < Q) dfv[a0 + e] = s + V[(a0 + e) * pw + c];
      }
      v_fwd_n<4>(l.A, l.dinv, c, lane, t);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (a0 + e < Q && lane < c) V[(a0 + e) * pw + lane] = t[e];
    }
    __syncthreads();
    if (lane < Q) {
      const double h2 = 0.5 / (f * f), h1 = 1.0 / f, dfb = dfv[lane];
      for (int pa = 0; pa <= lane; ++pa) {
        const double* ra = V + pa * pw;
        double s = 0.0;
        for (int j = 0; j < c; ++j) s += ra[j] * row[j];
        Fp[gh_fisher_pair(pa, lane, Q)] += h2 * dfv[pa] * dfb + h1 * s;
      }
    }
  }
  __syncthreads();
  for (int p = lane; p < npair; p += VM_MAX) partial[(long)blockIdx.x * npair + p] = Fp[p];
}
// out (ptot x ptot, zeroed by the caller): the pair (a, b) of the packed sums F to the rows / columns opos[a], opos[b] and mirrored
__global__ __launch_bounds__(256) void vecchia_fisher_scatter_kernel(const double* __restrict__ F, int Q, const int* __restrict__ opos,
                                                                     int ptot, double* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= Q * Q) return;
  const int pa = idx / Q, pb = idx - pa * Q;
  if (pb < pa) return;
  const double v = F[gh_fisher_pair(pa, pb, Q)];
  out[(long)opos[pa] * ptot + opos[pb]] = v;
  out[(long)opos[pb] * ptot + opos[pa]] = v;
}

// The forward operator as a row gather over the nrhs columns of r (row pitch ldr): with e = r_i - sum_s b_is r_c(i,s)
//   mode 0: e     1: e / f_i     2: e / sqrt(f_i)     3: e^2 / f_i
__global__ __launch_bounds__(256) void vecchia_fwd_kernel(const double* __restrict__ B, const double* __restrict__ f,
                                                          const int* __restrict__ nbr, const int* __restrict__ cnt, long n, int m,
                                                          const double* __restrict__ r, long nrhs, long ldr,
                                                          double* __restrict__ out, long ldo, int mode) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nrhs) return;
  const long i = idx / nrhs, col = idx - i * nrhs;
  const int c = cnt[i];
  double s = 0.0;
  for (int q = 0; q < c; ++q) s += B[i * m + q] * r[(long)nbr[i * m + q] * ldr + col];
  const double e = r[i * ldr + col] - s;
  const double fi = f[i];
  out[i * ldo + col] = mode == 0 ? e : mode == 1 ? e / fi : mode == 2 ? e / sqrt(fi) : e * e / fi;
}
// (I - B)^T as a gather through the transposed index: out_j = w_j - sum over the entries (row, slot) of column j of b_row,slot w_row
__global__ __launch_bounds__(256) void vecchia_bwd_kernel(const double* __restrict__ B, const long long* __restrict__ tptr,
                                                          const int* __restrict__ trow, const int* __restrict__ tslot, long n, int m,
                                                          const double* __restrict__ w, long nrhs, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * nrhs) return;
  const long j = idx / nrhs, col = idx - j * nrhs;
  double s = 0.0;
  for (long long q = tptr[j]; q < tptr[j + 1]; ++q) s += B[(long)trow[q] * m + tslot[q]] * w[(long)trow[q] * nrhs + col];
  out[idx] = w[idx] - s;
}
// diagA_j = the point's own slot plus its slots in the blocks of later points
__global__ __launch_bounds__(256) void vecchia_diag_kernel(const double* __restrict__ wd, const long long* __restrict__ tptr,
                                                           const int* __restrict__ trow, const int* __restrict__ tslot, long n, int m,
                                                           double* __restrict__ diagA) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = wd[j * (m + 1) + m];
  for (long long q = tptr[j]; q < tptr[j + 1]; ++q) s += wd[(long)trow[q] * (m + 1) + tslot[q]];
  diagA[j] = s;
}
// c_j = Q_jj = 1 / f_j + sum over the entries (row, slot) of column j of B[row, slot]^2 / f_row, rows ascending
__global__ __launch_bounds__(256) void vecchia_qdiag_kernel(const double* __restrict__ B, const double* __restrict__ f,
                                                            const long long* __restrict__ tptr, const int* __restrict__ trow,
                                                            const int* __restrict__ tslot, long n, int m, double* __restrict__ cq) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  double s = 1.0 / f[j];
  for (long long q = tptr[j]; q < tptr[j + 1]; ++q) {
    const double bq = B[(long)trow[q] * m + tslot[q]];
    s += bq * bq / f[trow[q]];
  }
  cq[j] = s;
}
// The leave-one-out values of point j from c = Q_jj and alpha = (Q r)_j: resid = alpha / c, var = 1 / c,
// lpd = 1/2 log c - 1/2 alpha^2 / c - 1/2 log 2 pi, and for the gradient wv = 1/2 (1 + alpha^2 / c) / c and av = alpha / c
// (= resid).  part[workgroup] = the sum of its 256 lpd in a fixed order.
__global__ __launch_bounds__(256) void vecchia_loo_point_kernel(const double* __restrict__ cq, const double* __restrict__ alpha, long n,
                                                                double* __restrict__ resid, double* __restrict__ var,
                                                                double* __restrict__ lpd, double* __restrict__ wv,
                                                                double* __restrict__ part) {
  __shared__ double sh[4];
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  double lp = 0.0;
  if (j < n) {
    const double c = cq[j], al = alpha[j], u = al / c;
    lp = 0.5 * log(c) - 0.5 * al * u - 0.9189385332046727418;
    resid[j] = u;
    var[j] = 1.0 / c;
    lpd[j] = lp;
    wv[j] = 0.5 * (1.0 + al * u) / c;
  }
  lp = block_sum_256(lp, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = lp;
}

// ================================================================================ host side
extern "C" int gh_vecchia_create(const gh_vecchia_opts* opts, gh_vecchia** out) {
  if (!out || !opts) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (opts->m < 1 || opts->m > VM_MAX) { gh_set_error("the Vecchia solver takes 1 <= m <= %d neighbours, not %d", VM_MAX, (int)opts->m); return GH_ERR_BAD_ARG; }
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd Vecchia solver needs an MI355X"); return GH_ERR_HIP; }
  gh_vecchia* h = new gh_vecchia();
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
extern "C" void gh_vecchia_destroy(gh_vecchia* h) {
  if (!h) return;
  (void)hipSetDevice(h->opts.device);
  if (h->st) (void)hipStreamSynchronize(h->st);             // (pooled blocks may be re-acquired by another handle)
  if (h->st && !h->shared_stream) (void)hipStreamDestroy(h->st);
  delete h;
}
extern "C" int64_t gh_vecchia_info(const gh_vecchia* h) { return h ? h->info : 0; }

static int v_need(gh_vecchia* h) {
  if (!h) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!h->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  GH_HIP(hipSetDevice(h->opts.device));
  return GH_OK;
}
template <typename Tv>
static int v_upload(GhBuf& buf, const std::vector<Tv>& v, hipStream_t st) {
  GH_CHECK(buf.ensure(std::max<size_t>(v.size(), 1) * sizeof(Tv)));
  if (!v.empty()) GH_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(Tv), hipMemcpyHostToDevice, st));
  return GH_OK;
}
// The neighbour table checked and compacted on the host: every entry of row i is -1 or in [0, i), no entry twice in a row.  A bad
// index would be an out-of-bounds read on the device, so nothing is launched before this has passed.  tab: valid entries first
// (their order kept), then -1; cnt: per row; and the transposed index by a counting sort (rows ascending inside a column).
static int v_index(const int32_t* nbr, int64_t n, int m, std::vector<int>& tab, std::vector<int>& cnt, std::vector<long long>& tptr,
                   std::vector<int>& trow, std::vector<int>& tslot) {
  tab.assign((size_t)n * m, -1);
  cnt.assign((size_t)n, 0);
  tptr.assign((size_t)n + 1, 0);
  std::vector<int64_t> seen((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    int c = 0;
    for (int s = 0; s < m; ++s) {
      const int32_t j = nbr[i * m + s];
      if (j == -1) continue;
      if (j < 0 || j >= i) { gh_set_error("neighbour table: row %lld holds %d, which is not one of its predecessors", (long long)i, (int)j); return GH_ERR_BAD_ARG; }
      if (seen[j] == i) { gh_set_error("neighbour table: row %lld holds %d twice", (long long)i, (int)j); return GH_ERR_BAD_ARG; }
      seen[j] = i;
      tab[(size_t)i * m + c++] = j;
      ++tptr[(size_t)j + 1];
    }
    cnt[(size_t)i] = c;
  }
  for (int64_t j = 0; j < n; ++j) tptr[(size_t)j + 1] += tptr[(size_t)j];
  trow.assign((size_t)tptr[(size_t)n], 0);
  tslot.assign((size_t)tptr[(size_t)n], 0);
  std::vector<long long> at(tptr.begin(), tptr.end() - 1);
  for (int64_t i = 0; i < n; ++i)
    for (int s = 0; s < cnt[(size_t)i]; ++s) {
      const long long q = at[(size_t)tab[(size_t)i * m + s]]++;
      trow[(size_t)q] = (int)i;
      tslot[(size_t)q] = s;
    }
  return GH_OK;
}
static VArgs v_args(const gh_vecchia* h, const gh_kernel* k) {
  VArgs a;
  a.x = h->x.d(); a.yerr = h->yerr.d(); a.nbr = (const int*)h->nbr.p; a.cnt = (const int*)h->cnt.p;
  a.n = (long)h->n; a.m = h->opts.m; a.nd = h->ndim; a.n_nodes = (int)k->nodes.size();
  return a;
}
static inline unsigned v_blocks(size_t work) { return (unsigned)((work + 255) / 256); }
// out (n, nrhs) = (I - B)^T F^-1 (I - B) rhs; tmp: n * nrhs doubles; all device memory
static int v_apply_q(gh_vecchia* h, const double* rhs, long nrhs, double* tmp, double* out) {
  const size_t tot = (size_t)h->n * nrhs;
  hipLaunchKernelGGL(vecchia_fwd_kernel, dim3(v_blocks(tot)), dim3(256), 0, h->st, (const double*)h->B.d(), (const double*)h->f.d(),
                     (const int*)h->nbr.p, (const int*)h->cnt.p, (long)h->n, h->opts.m, rhs, nrhs, nrhs, tmp, nrhs, 1);
  hipLaunchKernelGGL(vecchia_bwd_kernel, dim3(v_blocks(tot)), dim3(256), 0, h->st, (const double*)h->B.d(), (const long long*)h->tptr.p,
                     (const int*)h->trow.p, (const int*)h->tslot.p, (long)h->n, h->opts.m, (const double*)tmp, nrhs, out);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

extern "C" int gh_vecchia_compute(gh_vecchia* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                                  const int32_t* nbr, double* logdet_out) {
  if (!h || !k || !x || !yerr || !nbr || n <= 0 || n > 0x7ffffff0L) { gh_set_error("bad argument to compute"); return GH_ERR_BAD_ARG; }
  h->computed = false;
  h->info = 0;
  if (ndim != k->ndim || ndim < 1 || ndim > GH_MAX_NDIM) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  const int m = h->opts.m;
  if (h->grid.valid && !(h->n == n && h->ndim == ndim && !gh_is_device_ptr(x) &&
                         memcmp(h->grid.x_seen.data(), x, (size_t)n * ndim * sizeof(double)) == 0))
    h->grid.valid = false;                                  // (other points: the next search builds its grid again)
  const bool same_table = h->n == n && h->nbr_seen.size() == (size_t)n * m && memcmp(h->nbr_seen.data(), nbr, (size_t)n * m * sizeof(int32_t)) == 0;
  std::vector<int> tab, cnt, trow, tslot;
  std::vector<long long> tptr;
  if (!same_table) {
    h->nbr_seen.clear();
    GH_CHECK(v_index(nbr, n, m, tab, cnt, tptr, trow, tslot));
  }
  GH_HIP(hipSetDevice(h->opts.device));
  GH_CHECK(k->upload());
  hipStream_t st = h->st;
  h->n = n;
  h->ndim = ndim;
  GH_CHECK(h->x.ensure((size_t)n * ndim * sizeof(double)));
  GH_CHECK(h->yerr.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(h->x.d(), x, (size_t)n * ndim, st));
  GH_CHECK(gh_to_device(h->yerr.d(), yerr, (size_t)n, st));
  if (!same_table) {
    GH_CHECK(v_upload(h->nbr, tab, st));
    GH_CHECK(v_upload(h->cnt, cnt, st));
    GH_CHECK(v_upload(h->tptr, tptr, st));
    GH_CHECK(v_upload(h->trow, trow, st));
    GH_CHECK(v_upload(h->tslot, tslot, st));
    GH_HIP(hipStreamSynchronize(st));                       // (the host vectors end with this call)
    h->nbr_seen.assign(nbr, nbr + (size_t)n * m);
  }
  GH_CHECK(h->B.ensure((size_t)n * m * sizeof(double)));
  GH_CHECK(h->f.ensure((size_t)n * sizeof(double)));
  GH_CHECK(h->w1.ensure((size_t)n * sizeof(double)));
  GH_CHECK(h->scal.ensure(2 * sizeof(double)));
  int* fail = (int*)(h->scal.d() + 1);
  GH_HIP(hipMemsetD32Async((hipDeviceptr_t)fail, INT_MAX, 1, st));
  const VArgs a = v_args(h, k);
  const bool fast = k->fast.ok != 0;
  const size_t lds = v_lds_doubles(m, ndim, fast ? 0 : VWS) * sizeof(double);
  if (fast) hipLaunchKernelGGL(vecchia_factor_kernel<true>, dim3((unsigned)n), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes,
                               h->B.d(), h->f.d(), h->w1.d(), fail);
  else hipLaunchKernelGGL(vecchia_factor_kernel<false>, dim3((unsigned)n), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes,
                          h->B.d(), h->f.d(), h->w1.d(), fail);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(h->w1.d(), n, 1, h->scal.d(), st));          // log|K| ~ sum_i log f_i, fixed order
  double res[2] = {0.0, 0.0};
  GH_HIP(hipMemcpyAsync(res, h->scal.d(), 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  int failed;
  memcpy(&failed, &res[1], sizeof(int));
  if (failed != INT_MAX) {
    h->info = (int64_t)failed + 1;
    gh_set_error("the conditional of point %lld is not positive definite", (long long)failed);
    return GH_ERR_NOT_PD;
  }
  h->logdet = res[0];
  if (logdet_out) *logdet_out = res[0];
  h->computed = true;
  return GH_OK;
}

extern "C" int gh_vecchia_solve(gh_vecchia* h, const double* b, int64_t nrhs, double* out) {
  GH_CHECK(v_need(h));
  if (!b || !out || nrhs <= 0) { gh_set_error("bad argument to solve"); return GH_ERR_BAD_ARG; }
  const size_t tot = (size_t)h->n * nrhs;
  GhPooledBuf rhs, tmp;
  GH_CHECK(rhs.ensure(tot * sizeof(double)));
  GH_CHECK(tmp.ensure(tot * sizeof(double)));
  GH_CHECK(gh_to_device(rhs.d(), b, tot, h->st));
  GH_CHECK(v_apply_q(h, rhs.d(), (long)nrhs, tmp.d(), rhs.d()));
  GH_CHECK(gh_from_device(out, rhs.d(), tot, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  return GH_OK;
}
extern "C" int gh_vecchia_dot_solve(gh_vecchia* h, const double* y, double* out) {
  GH_CHECK(v_need(h));
  if (!y || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  const long n = (long)h->n;
  GhPooledBuf yd;
  GH_CHECK(yd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(yd.d(), y, (size_t)n, h->st));
  hipLaunchKernelGGL(vecchia_fwd_kernel, dim3(v_blocks((size_t)n)), dim3(256), 0, h->st, (const double*)h->B.d(), (const double*)h->f.d(),
                     (const int*)h->nbr.p, (const int*)h->cnt.p, n, h->opts.m, (const double*)yd.d(), 1L, 1L, h->w1.d(), 1L, 3);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(h->w1.d(), n, 1, h->scal.d(), h->st));       // sum_i e_i^2 / f_i, fixed order
  double v = 0.0;
  GH_HIP(hipMemcpyAsync(&v, h->scal.d(), sizeof(double), hipMemcpyDeviceToHost, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  *out = v;
  return GH_OK;
}

// The dynamic LDS of a gradient kernel (vecchia_grad_kernel, vecchia_loo_grad_kernel: v_lds_doubles at gp) above 64 KB -- m = 64
// with eight or more input dimensions and ~60 parameters, 70 KB at most: the limit of both instantiations is raised first.
static int v_grad_lds_limit(const void* k_fast, const void* k_interp, size_t lds) {
  if (lds > 64 * 1024) {
    GH_HIP(hipFuncSetAttribute(k_fast, hipFuncAttributeMaxDynamicSharedMemorySize, V_GRAD_LDS));
    GH_HIP(hipFuncSetAttribute(k_interp, hipFuncAttributeMaxDynamicSharedMemorySize, V_GRAD_LDS));
  }
  return GH_OK;
}

extern "C" int gh_vecchia_grad(gh_vecchia* h, gh_kernel* k, const uint32_t* which, const double* r, double* grad, double* alpha,
                               double* diagA) {
  GH_CHECK(v_need(h));
  if (!k || !which || !r || !grad) { gh_set_error("bad argument to grad"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (k->size > GH_MAX_GRAD) { gh_set_error("grad: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  GH_CHECK(k->upload());
  const long n = (long)h->n;
  const int m = h->opts.m, P = k->size, Pw = P > 0 ? P : 1;
  hipStream_t st = h->st;
  GhPooledBuf rd, tmp, al, part, wd, dg;
  GH_CHECK(rd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(tmp.ensure((size_t)n * sizeof(double)));
  GH_CHECK(al.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(rd.d(), r, (size_t)n, st));
  if (alpha) {
    GH_CHECK(v_apply_q(h, rd.d(), 1L, tmp.d(), al.d()));
    GH_CHECK(gh_from_device(alpha, al.d(), (size_t)n, st));
  }
  const unsigned nwg = (unsigned)std::min<long>(n, V_GRAD_WGS);
  const size_t which_bytes = ((sizeof(uint32_t) * Pw + 15) / 16) * 16;
  GH_CHECK(part.ensure(which_bytes + ((size_t)nwg + 1) * Pw * sizeof(double)));
  GH_CHECK(wd.ensure((size_t)n * (m + 1) * sizeof(double)));
  GH_CHECK(dg.ensure((size_t)n * sizeof(double)));
  uint32_t* d_which = (uint32_t*)part.p;
  double* partial = (double*)((char*)part.p + which_bytes);
  double* dgrad = partial + (size_t)nwg * Pw;
  if (P > 0) GH_HIP(hipMemcpyAsync(d_which, which, sizeof(uint32_t) * P, hipMemcpyHostToDevice, st));
  const VArgs a = v_args(h, k);
  const int gp = (P + GH_EVAL_WS) | 1;                      // doubles per lane: the gradient row, the evaluator's work space; odd
  const size_t lds = v_lds_doubles(m, h->ndim, gp) * sizeof(double);
  GH_CHECK(v_grad_lds_limit((const void*)vecchia_grad_kernel<true>, (const void*)vecchia_grad_kernel<false>, lds));
  if (k->fast.ok) hipLaunchKernelGGL(vecchia_grad_kernel<true>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                                     (const uint32_t*)d_which, (const double*)rd.d(), partial, wd.d());
  else hipLaunchKernelGGL(vecchia_grad_kernel<false>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                          (const uint32_t*)d_which, (const double*)rd.d(), partial, wd.d());
  GH_HIP(hipGetLastError());
  if (P > 0) {
    GH_CHECK(gh_launch_kgrad_final(partial, nwg, P, dgrad, st));
    GH_CHECK(gh_from_device(grad, dgrad, (size_t)P, st));
  }
  if (diagA) {
    hipLaunchKernelGGL(vecchia_diag_kernel, dim3(v_blocks((size_t)n)), dim3(256), 0, st, (const double*)wd.d(), (const long long*)h->tptr.p,
                       (const int*)h->trow.p, (const int*)h->tslot.p, n, m, dg.d());
    GH_HIP(hipGetLastError());
    GH_CHECK(gh_from_device(diagA, dg.d(), (size_t)n, st));
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_vecchia_loo(gh_vecchia* h, gh_kernel* k, const uint32_t* which, const double* r, double* lpd_sum, double* resid,
                              double* var, double* lpd, double* grad, double* v, double* diagB) {
  GH_CHECK(v_need(h));
  if (!k || !r || !lpd_sum || !resid || !var || (which ? !grad : (grad || v || diagB))) { gh_set_error("bad argument to loo"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (k->size > GH_MAX_GRAD) { gh_set_error("loo: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  const long n = (long)h->n;
  const int m = h->opts.m, P = k->size, Pw = P > 0 ? P : 1;
  hipStream_t st = h->st;
  // vals: r, alpha, c, resid (= av), var, lpd, wv, one apply's work space -- n doubles each -- and the partial sums of lpd
  const unsigned nblk = v_blocks((size_t)n);
  GhPooledBuf vals, part, wd;
  GH_CHECK(vals.ensure(((size_t)8 * n + nblk + 1) * sizeof(double)));
  double* const rd = vals.d();
  double* const al = rd + n;
  double* const cq = al + n;
  double* const rs = cq + n;
  double* const vr = rs + n;
  double* const lp = vr + n;
  double* const wv = lp + n;
  double* const tmp = wv + n;
  double* const lpart = tmp + n;
  GH_CHECK(gh_to_device(rd, r, (size_t)n, st));
  hipLaunchKernelGGL(vecchia_qdiag_kernel, dim3(nblk), dim3(256), 0, st, (const double*)h->B.d(), (const double*)h->f.d(),
                     (const long long*)h->tptr.p, (const int*)h->trow.p, (const int*)h->tslot.p, n, m, cq);
  GH_HIP(hipGetLastError());
  GH_CHECK(v_apply_q(h, rd, 1L, tmp, al));
  hipLaunchKernelGGL(vecchia_loo_point_kernel, dim3(nblk), dim3(256), 0, st, (const double*)cq, (const double*)al, n, rs, vr, lp, wv, lpart);
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_launch_kgrad_final(lpart, nblk, 1, lpart + nblk, st));           // per-workgroup partials, fixed order
  GH_HIP(hipMemcpyAsync(lpd_sum, lpart + nblk, sizeof(double), hipMemcpyDeviceToHost, st));
  GH_CHECK(gh_from_device(resid, rs, (size_t)n, st));
  GH_CHECK(gh_from_device(var, vr, (size_t)n, st));
  if (lpd) GH_CHECK(gh_from_device(lpd, lp, (size_t)n, st));
  if (which) {
    GH_CHECK(k->upload());
    const unsigned nwg = (unsigned)std::min<long>(n, V_GRAD_WGS);
    const size_t which_bytes = ((sizeof(uint32_t) * Pw + 15) / 16) * 16;
    GH_CHECK(part.ensure(which_bytes + ((size_t)nwg + 1) * Pw * sizeof(double)));
    GH_CHECK(wd.ensure((size_t)n * (m + 1) * sizeof(double)));
    uint32_t* d_which = (uint32_t*)part.p;
    double* partial = (double*)((char*)part.p + which_bytes);
    double* dgrad = partial + (size_t)nwg * Pw;
    if (P > 0) GH_HIP(hipMemcpyAsync(d_which, which, sizeof(uint32_t) * P, hipMemcpyHostToDevice, st));
    const VArgs a = v_args(h, k);
    const int gp = (P + GH_EVAL_WS) | 1;                    // (as gh_vecchia_grad, and its LDS)
    const size_t lds = v_lds_doubles(m, h->ndim, gp) * sizeof(double);
    GH_CHECK(v_grad_lds_limit((const void*)vecchia_loo_grad_kernel<true>, (const void*)vecchia_loo_grad_kernel<false>, lds));
    if (k->fast.ok) hipLaunchKernelGGL(vecchia_loo_grad_kernel<true>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                                       (const uint32_t*)d_which, (const double*)rd, (const double*)wv, (const double*)rs, partial, wd.d());
    else hipLaunchKernelGGL(vecchia_loo_grad_kernel<false>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                            (const uint32_t*)d_which, (const double*)rd, (const double*)wv, (const double*)rs, partial, wd.d());
    GH_HIP(hipGetLastError());
    if (P > 0) {
      GH_CHECK(gh_launch_kgrad_final(partial, nwg, P, dgrad, st));
      GH_CHECK(gh_from_device(grad, dgrad, (size_t)P, st));
    }
    if (v) {                                                // Q av; al and cq are free by now
      GH_CHECK(v_apply_q(h, rs, 1L, tmp, al));
      GH_CHECK(gh_from_device(v, al, (size_t)n, st));
    }
    if (diagB) {
      hipLaunchKernelGGL(vecchia_diag_kernel, dim3(v_blocks((size_t)n)), dim3(256), 0, st, (const double*)wd.d(), (const long long*)h->tptr.p,
                         (const int*)h->trow.p, (const int*)h->tslot.p, n, m, cq);
      GH_HIP(hipGetLastError());
      GH_CHECK(gh_from_device(diagB, cq, (size_t)n, st));
    }
  }
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_vecchia_fisher(gh_vecchia* h, gh_kernel* k, const uint32_t* which, const double* diag_rows, int32_t n_diag,
                                 double* out) {
  GH_CHECK(v_need(h));
  if (!k || !which || !out || n_diag < 0 || (n_diag > 0 && !diag_rows)) { gh_set_error("bad argument to fisher"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (k->size > GH_MAX_GRAD) { gh_set_error("fisher: %d kernel parameters, at most %d", k->size, GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  const long n = (long)h->n;
  const int m = h->opts.m, P = k->size, ptot = n_diag + P;
  // the planes: the diagonal ones, then the kernel parameters `which` selects; kp_op = kpar (Q - n_diag) and opos (Q) behind it
  std::vector<int> kp_op;
  for (int p = 0; p < P; ++p)
    if (which[p]) kp_op.push_back(p);
  const int nk = (int)kp_op.size(), Q = n_diag + nk;
  if (Q > V_FISHER_PLANES) {
    gh_set_error("fisher: %d diagonal and %d selected kernel parameters, at most %d planes in one call", (int)n_diag, nk, V_FISHER_PLANES);
    return GH_ERR_BAD_ARG;
  }
  if (ptot == 0) return GH_OK;
  for (int a = 0; a < Q; ++a) kp_op.push_back(a < n_diag ? a : n_diag + kp_op[a - n_diag]);
  GH_CHECK(k->upload());
  hipStream_t st = h->st;
  GhPooledBuf od, rows, part;
  GH_CHECK(od.ensure((size_t)ptot * ptot * sizeof(double)));
  GH_HIP(hipMemsetAsync(od.p, 0, (size_t)ptot * ptot * sizeof(double), st));
  if (Q > 0) {
    const int gp = (P + GH_EVAL_WS) | 1, npair = Q * (Q + 1) / 2;               // (gp: as gh_vecchia_grad)
    const size_t lds = v_fisher_lds_doubles(m, h->ndim, gp, Q) * sizeof(double);
    if (lds > V_FISHER_LDS) { gh_set_error("fisher: %zu bytes of LDS, at most %d", lds, V_FISHER_LDS); return GH_ERR_BAD_ARG; }
    const unsigned nwg = (unsigned)std::min<long>(n, V_GRAD_WGS);
    const size_t map_bytes = ((sizeof(int) * kp_op.size() + 15) / 16) * 16;
    GH_CHECK(rows.ensure(std::max<size_t>((size_t)n_diag * n, 1) * sizeof(double)));
    GH_CHECK(part.ensure(map_bytes + ((size_t)nwg + 1) * npair * sizeof(double)));
    if (n_diag > 0) GH_CHECK(gh_to_device(rows.d(), diag_rows, (size_t)n_diag * n, st));
    int* d_kpar = (int*)part.p;
    double* partial = (double*)((char*)part.p + map_bytes);
    double* dF = partial + (size_t)nwg * npair;
    GH_HIP(hipMemcpyAsync(d_kpar, kp_op.data(), sizeof(int) * kp_op.size(), hipMemcpyHostToDevice, st));
    const VArgs a = v_args(h, k);
    if (lds > 64 * 1024) {                                  // (m = 64 in 16 dimensions with 64 planes: 119 KB)
      GH_HIP(hipFuncSetAttribute((const void*)vecchia_fisher_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, V_FISHER_LDS));
      GH_HIP(hipFuncSetAttribute((const void*)vecchia_fisher_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, V_FISHER_LDS));
    }
    if (k->fast.ok) hipLaunchKernelGGL(vecchia_fisher_kernel<true>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                                       Q, (int)n_diag, (const int*)d_kpar, (const double*)rows.d(), partial);
    else hipLaunchKernelGGL(vecchia_fisher_kernel<false>, dim3(nwg), dim3(VM_MAX), lds, st, a, k->fast, (const GhNode*)k->d_nodes, P, gp,
                            Q, (int)n_diag, (const int*)d_kpar, (const double*)rows.d(), partial);
    GH_HIP(hipGetLastError());
    GH_CHECK(gh_launch_kgrad_final(partial, nwg, npair, dF, st));                // per-workgroup partials, fixed order
    hipLaunchKernelGGL(vecchia_fisher_scatter_kernel, dim3(v_blocks((size_t)Q * Q)), dim3(256), 0, st, (const double*)dF, Q,
                       (const int*)(d_kpar + nk), ptot, od.d());
    GH_HIP(hipGetLastError());
  }
  GH_CHECK(gh_from_device(out, od.d(), (size_t)ptot * ptot, st));
  GH_HIP(hipStreamSynchronize(st));                         // (kp_op ends with this call)
  return GH_OK;
}

extern "C" int gh_vecchia_predict(gh_vecchia* h, gh_kernel* k, const double* r, const double* xs, int64_t m, double* mu, double* var,
                                  double* cov) {
  GH_CHECK(v_need(h));
  if (!k || !r || !xs || !mu || m <= 0 || (var && cov) || m > 0x3fffffffL) { gh_set_error("bad argument to predict"); return GH_ERR_BAD_ARG; }
  if (k->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_CHECK(k->upload());
  const long n = (long)h->n;
  hipStream_t st = h->st;
  GhPooledBuf rd, tmp, al, xsd;
  GH_CHECK(rd.ensure((size_t)n * sizeof(double)));
  GH_CHECK(tmp.ensure((size_t)n * sizeof(double)));
  GH_CHECK(al.ensure((size_t)n * sizeof(double)));
  GH_CHECK(gh_to_device(rd.d(), r, (size_t)n, st));
  GH_CHECK(v_apply_q(h, rd.d(), 1L, tmp.d(), al.d()));
  const double* xs_dev = nullptr;
  GH_CHECK(gh_stage_points(xs, m, h->ndim, xsd, st, &xs_dev));
  if (cov) {
    const long mp = gh_round_up(m, 128), np = gh_round_up(n, 16);
    const double need = 2.0 * 8.0 * (double)np * (double)mp + 8.0 * (double)mp * (double)mp;
    if (need > (double)V_COV_BYTES) {
      gh_set_error("predict: the covariance keeps K(x, xs), V and the m x m result on the device, %.3g bytes for n = %ld, m = %ld, over the "
                   "budget of %ld; ask for the variance or for fewer test points at a time", need, n, (long)m, (long)V_COV_BYTES);
      return GH_ERR_NOMEM;
    }
  }
  const long Ct = std::min<long>(std::max<long>(1, std::min<long>(V_STRIP_COLS, V_STRIP_BYTES / (16 * n))), m);
  // V = F^-1/2 (I - B) Kx: the moments are V . V
  return gh_predict_strips(k, h->x.d(), n, h->ndim, al.d(), xs_dev, m, Ct, V_RED_ROWS, V_RED_CHUNKS, mu, var, cov, st, false,
                           [&](const double* sK, double* sV, int64_t ld, int64_t, int, size_t) -> int {
    hipLaunchKernelGGL(vecchia_fwd_kernel, dim3(v_blocks((size_t)n * ld)), dim3(256), 0, st, (const double*)h->B.d(), (const double*)h->f.d(),
                       (const int*)h->nbr.p, (const int*)h->cnt.p, n, h->opts.m, sK, (long)ld, (long)ld, sV, (long)ld, 2);
    GH_HIP(hipGetLastError());
    return GH_OK;
  });
}

// The query table of predict_local checked and compacted on the host, as v_index does with compute's: every entry of a row is -1
// or in [0, n), no entry twice in a row.  tab: valid entries first (their order kept), then -1; cnt: per row.
static int v_query_index(const int32_t* qnbr, int64_t M, int mq, int64_t n, std::vector<int>& tab, std::vector<int>& cnt) {
  tab.assign((size_t)M * mq, -1);
  cnt.assign((size_t)M, 0);
  std::vector<int64_t> seen((size_t)n, -1);
  for (int64_t t = 0; t < M; ++t) {
    int c = 0;
    for (int s = 0; s < mq; ++s) {
      const int32_t j = qnbr[t * mq + s];
      if (j == -1) continue;
      if (j < 0 || j >= n) { gh_set_error("query table: row %lld holds %d, which is not one of the %lld data points", (long long)t, (int)j, (long long)n); return GH_ERR_BAD_ARG; }
      if (seen[j] == t) { gh_set_error("query table: row %lld holds %d twice", (long long)t, (int)j); return GH_ERR_BAD_ARG; }
      seen[j] = t;
      tab[(size_t)t * mq + c++] = j;
    }
    cnt[(size_t)t] = c;
  }
  return GH_OK;
}

// What the two local predictions share.  Head: the argument checks, and r and xs on the device.
static int v_local_begin(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r, const double* xs, int64_t M, int32_t mq,
                         const double* mu, const void* table) {
  GH_CHECK(v_need(h));
  if (!k_data || !k_cross || !r || !xs || !table || !mu || M <= 0 || M > 0x3fffffffL) { gh_set_error("bad argument to predict_local"); return GH_ERR_BAD_ARG; }
  if (mq < 1 || mq > VM_MAX) { gh_set_error("predict_local takes 1 <= mq <= %d neighbours per test point, not %d", VM_MAX, (int)mq); return GH_ERR_BAD_ARG; }
  if (k_data->ndim != h->ndim || k_cross->ndim != h->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  h->info = 0;
  return GH_OK;
}
static int v_local_inputs(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r, const double* xs, int64_t M, GhBuf& rd,
                          GhBuf& xsd, const double** xs_dev) {
  GH_CHECK(k_data->upload());
  if (k_cross != k_data) GH_CHECK(k_cross->upload());
  GH_CHECK(rd.ensure((size_t)h->n * sizeof(double)));
  GH_CHECK(gh_to_device(rd.d(), r, (size_t)h->n, h->st));
  return gh_stage_points(xs, M, h->ndim, xsd, h->st, xs_dev);
}
// Tail: the kernel over the device table qt (valid entries first) with the row counts qc, the failure flag, mu and var back.
static int v_local_run(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* rd, const double* xs_dev, int64_t M,
                       const int* qt, const int* qc, int32_t mq, double* mu, double* var) {
  hipStream_t st = h->st;
  GhPooledBuf res;
  GH_CHECK(res.ensure((size_t)2 * M * sizeof(double)));
  GH_CHECK(h->scal.ensure(2 * sizeof(double)));
  double* dmu = res.d();
  double* dvar = var ? dmu + M : nullptr;
  int* fail = (int*)(h->scal.d() + 1);
  GH_HIP(hipMemsetD32Async((hipDeviceptr_t)fail, INT_MAX, 1, st));
  VArgs a = v_args(h, k_data);
  a.m = mq;
  // the interpreter evaluates every kernel, the fast form only some: one instantiation for "both fast", one for the rest
  const bool fast = k_data->fast.ok != 0 && k_cross->fast.ok != 0;
  const size_t lds = v_lds_doubles(mq, h->ndim, fast ? 0 : VWS) * sizeof(double);        // (at most 37 KB: mq = 64, 16 dimensions)
  if (fast) hipLaunchKernelGGL(vecchia_local_kernel<true>, dim3((unsigned)M), dim3(VM_MAX), lds, st, a, k_data->fast, (const GhNode*)k_data->d_nodes,
                               k_cross->fast, (const GhNode*)k_cross->d_nodes, (int)k_cross->nodes.size(), rd, xs_dev, qt, qc, (int)mq, dmu, dvar,
                               fail);
  else hipLaunchKernelGGL(vecchia_local_kernel<false>, dim3((unsigned)M), dim3(VM_MAX), lds, st, a, k_data->fast, (const GhNode*)k_data->d_nodes,
                          k_cross->fast, (const GhNode*)k_cross->d_nodes, (int)k_cross->nodes.size(), rd, xs_dev, qt, qc, (int)mq, dmu, dvar,
                          fail);
  GH_HIP(hipGetLastError());
  int failed = INT_MAX;
  GH_HIP(hipMemcpyAsync(&failed, fail, sizeof(int), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));                         // (the caller's host tables end with this call)
  if (failed != INT_MAX) {
    h->info = (int64_t)failed + 1;
    gh_set_error("the conditional of test point %lld is not positive definite", (long long)failed);
    return GH_ERR_NOT_PD;
  }
  GH_CHECK(gh_from_device(mu, dmu, (size_t)M, st));
  if (var) GH_CHECK(gh_from_device(var, dvar, (size_t)M, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}

extern "C" int gh_vecchia_predict_local(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r, const double* xs, int64_t M,
                                        const int32_t* qnbr, int32_t mq, double* mu, double* var) {
  GH_CHECK(v_local_begin(h, k_data, k_cross, r, xs, M, mq, mu, qnbr));
  std::vector<int> tab, cnt;
  GH_CHECK(v_query_index(qnbr, M, mq, (long)h->n, tab, cnt));        // (before any launch: a bad index would be an out-of-bounds read)
  GhPooledBuf rd, xsd, qt, qc;
  const double* xs_dev = nullptr;
  GH_CHECK(v_local_inputs(h, k_data, k_cross, r, xs, M, rd, xsd, &xs_dev));
  GH_CHECK(v_upload(qt, tab, h->st));
  GH_CHECK(v_upload(qc, cnt, h->st));
  return v_local_run(h, k_data, k_cross, rd.d(), xs_dev, M, (const int*)qt.p, (const int*)qc.p, mq, mu, var);
}

// The same with the table made on the device: the grid of the handle's x (built at the first search after a compute() on other
// points, or with another occupancy), the search, and its table and row counts straight into the kernel -- the search writes
// valid entries first and nothing but data points, so there is nothing to check, compact or upload.
extern "C" int gh_vecchia_predict_local_search(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r, const double* xs,
                                               int64_t M, int32_t mq, int32_t occupancy, double* mu, double* var, int32_t* table_out) {
  GH_CHECK(v_local_begin(h, k_data, k_cross, r, xs, M, mq, mu, /* the table is made here */ mu));
  if (occupancy < 0) { gh_set_error("bad argument to predict_local"); return GH_ERR_BAD_ARG; }
  hipStream_t st = h->st;
  if (!h->grid.valid || h->grid.occupancy != occupancy) {
    h->grid.valid = false;
    h->grid.x_seen.resize((size_t)h->n * h->ndim);
    GH_HIP(hipMemcpyAsync(h->grid.x_seen.data(), h->x.p, h->grid.x_seen.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    GH_CHECK(gh_vgrid_build(h->grid, h->grid.x_seen.data(), h->n, h->ndim, occupancy, st));
  }
  GhPooledBuf rd, xsd, qt, qc;
  const double* xs_dev = nullptr;
  GH_CHECK(v_local_inputs(h, k_data, k_cross, r, xs, M, rd, xsd, &xs_dev));
  GH_CHECK(qt.ensure((size_t)M * mq * sizeof(int)));
  GH_CHECK(qc.ensure((size_t)M * sizeof(int)));
  GH_CHECK(gh_vgrid_query(h->grid, xs_dev, M, nullptr, mq, (int*)qt.p, (int*)qc.p, st));
  if (table_out) GH_HIP(hipMemcpyAsync(table_out, qt.p, (size_t)M * mq * sizeof(int), hipMemcpyDefault, st));
  return v_local_run(h, k_data, k_cross, rd.d(), xs_dev, M, (const int*)qt.p, (const int*)qc.p, mq, mu, var);
}
