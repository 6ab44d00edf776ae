// gh_batch.hip -- B log-likelihoods of one kernel STRUCTURE at B parameter vectors in one device call
// (gh_chol_objective_batch: GP.log_likelihood_batch, the hook for emcee's `vectorize=True`), with B predictions
// (gh_chol_predict_batch) and B likelihood gradients (gh_chol_objective_grad_batch) built on the same chain.
//
// At the sizes samplers run (N of a few hundred to a few thousand) one factorisation fills a few percent of the chip: it is a
// serial chain of 128-column steps, and a sampler step used to run B such chains one after the other.  Here every launch of
// ONE chain carries all B members: the launch count is that of one problem and each launch does B times the work.
//
// One layout.  Member b owns a row-major panel of rt tile rows (128 rows each) of pitch ld; np = N rounded up to 128,
// nt = np / 128.  The top nt tile rows hold K_b with identity padding (as the one-problem build pads); tile row nt is the
// residual tile, r_b^T (zero-padded) in its first row; the tile rows below it are carried rows: the test rows of a prediction,
// the rows of the identity for a gradient, none for the plain objective.  Besides the panel the member has q 128 x 128 output
// tiles.  The right-looking factorisation over K's nt tile columns leaves z_b = L_b^-1 r_b in row np and the carried rows
// times L_b^-T below it: there is no separate triangular solve.  Per step j, three launches over all members (batch_chain):
//   potf2 : tile (j, j) -> L_jj and L_jj^-1 (gh_potf2::potf2_body; info per member);
//   TRSM  : tiles (i, j), i > j, of K, the residual tile and the carried rows:  P <- P L_jj^-T   (gh_tile128_nt_sp<false>);
//   update: tiles (i, l), j < l < ld / 128, l <= i:  C -= P_i P_l^T, K = 128   (gh_tile128_nt_sp<true>, batch_trap_kernel).
// A member whose info is set returns from every later kernel at once.  The three entry points are three shapes of it:
//   objective: ld = np + 128, rt = nt + 1, nothing carried.  The panel is a bordered square; its one output tile is the corner
//              tile at [np][np], INSIDE the panel, so the update's triangle takes it in and the chain itself leaves
//              -r_b^T K_b^-1 r_b at [np][np].  (The border column tiles above the corner are never written or read.)
//   predict  : ld = np, rt = nt + 1 + mt, the mt test tile rows carried at every step.  One Schur launch after the chain
//              (batch_schur_kernel, K = np) forms the output tiles -z^T z, -V^T z and K** - V^T V.
//   gradient : ld = np, rt = 2 nt + 1, identity rows: at step j only identity row tiles 0 .. j are non-zero and carried; the
//              Schur launch skips each tile's leading zero k-tiles.
//
// Bits.  The one-problem factorisation (gh_chol.hip) applies the same updates to every tile in the same k order, only in
// longer K (panel widths, rows-below TRSM): every k-major x k-major kernel shares one k assignment (gh_gemm_tile.h) and a
// tile's accumulators start from -C and are written back as -acc, both exact, so cutting K at 128 changes no bits.  The
// elements are formed by the same evaluator calls in the same argument order as kmat_generic_tile, and the log-determinant
// is summed in launch_logdet's slice order: L_b and logdet[b] equal gh_chol_compute's bit for bit.  quad[b] is summed tile by
// tile instead of by the chained forward solve and matches to rounding.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"
#include "gh_device_util.h"
#include "gh_gemm_tile.h"
#include "gh_potf2_body.h"

#define T 128

struct GhBatchBufs {
  GhBuf A;                     // B panels
  GhBuf dinv;                  // B x (np / 128) inverses of the 128 x 128 diagonal blocks
  GhBuf in;                    // [member nodes | member fast forms | x | yerr | r] (the last three when they come from the host)
  GhBuf out;                   // [logdet (B) | quad (B) | info (B)]
  GhBuf O;                     // predict: B x (mt + 1 + K** tiles) 128 x 128 output tiles of the Schur complement; grad: -z^T z, -alpha, -K^-1
  GhBuf res;                   // predict: [mu (B, m) | var (B, m) or cov (B, m, m)]; grad: [grad (B, P) | alpha (B, n) | diagA (B, n)]
  GhBuf part;                  // grad: [which (P) | partial rows of the reduction (B, 64-tiles, P)]
  GhBuf samp;                  // sample: [thresholds (B) | the factor / draw work arrays of gh_sample_enqueue]
  std::vector<char> stage;     // host image of `in`: ONE host-to-device copy per call
  std::vector<double> back;    // host image of `out`: ONE device-to-host copy per call
};
GhBatchBufs* gh_batch_new() { return new GhBatchBufs(); }
size_t gh_batch_bytes(const GhBatchBufs* b) {
  if (!b) return 0;
  size_t tot = 0;
  for (const GhBuf* x : {&b->A, &b->dinv, &b->in, &b->out, &b->O, &b->res, &b->part, &b->samp}) tot += x->p ? x->bytes : 0;
  return tot;
}
void gh_batch_free(GhBatchBufs* b) { delete b; }

// wave-uniform: has member b failed at an earlier step?
__device__ __forceinline__ bool member_failed(const long long* info, int b) {
  return __builtin_amdgcn_readfirstlane((int)(info[b] != 0)) != 0;
}

// ---------------------------------------------------------------------------------------------------- build
struct BatchPBuild {
  const GhNode* nodes; int n_nodes; int ndim;    // member b's program: nodes + b * n_nodes
  const GhFast* fast;                            // (B) when every member has the a + b F(r^2) form
  const double* x; long n;                       // (n, ndim), shared
  const double* xs; long m;                      // (m, ndim), shared
  const double* yerr; const double* r;           // (B, n)
  double* A; long ld, np, stride;                // member b's panel: A + b * stride, (np + 128 + mp) rows of pitch ld
  double* O; long ostride;                       // member b's output tile u (not in the panel): O + b * ostride + u * 128 * 128
  int mt, kss;                                   // carried tile rows; K** tiles: 0 none, 1 diagonal, 2 lower
  long long* info;                               // (B): cleared here
  long ktiles, ptiles, tiles;                    // per member: K's lower tiles, + the panel tiles below K, + the output tiles
};
// blockIdx.x = member * 4 * tiles + 4 * tile + quadrant: one 64 x 64 quarter of a 128-tile, as kmat_tile_of builds them.  Tiles,
// in order: K's lower triangle, the (1 + mt) x nt panel tiles below it (residual tile, then carried rows), the mt + 1
// residual-column output tiles (zero), the K** output tiles.
// ROWS, what is carried below the residual tile: 1 the test rows k(x_i, xs_c), with K** output tiles; 2 the rows of the identity
// (gh_chol_objective_grad_batch; the K** tiles zero); 0 nothing, and the one output tile is the panel's corner tile (the
// objective's bordered square): every tile is then a panel tile, the lower triangle of the (nt + 1)^2 tile grid in tri_index order.
template <bool FAST, int ROWS>
__global__ __launch_bounds__(256) void batch_pbuild_kernel(BatchPBuild a) {
  const long q4 = (long)blockIdx.x;
  const int b = (int)(q4 / (4 * a.tiles));
  const long t = (q4 / 4) % a.tiles;
  const int quad = (int)(q4 & 3);
  if (t == 0 && quad == 0 && threadIdx.x == 0) a.info[b] = 0;
  if constexpr (ROWS == 0) {
    // the bordered square on its own: measured 3 % faster with the 17-node walker than the general body below compiled for
    // "nothing carried" (profiles/batch/refactor_ab.md), so the objective keeps the build it always had
    int TI, TJ;
    tri_index(t, TI, TJ);
    const long r0 = (long)TI * T + (quad >> 1) * 64, c0 = (long)TJ * T + (quad & 1) * 64;
    const GhNode* prog = a.nodes + (long)b * a.n_nodes;
    const double* yerr = a.yerr + (long)b * a.n;
    const double* res = a.r + (long)b * a.n;
    double* Ab = a.A + (long)b * a.stride;
    const int nd = a.ndim;
    const int lc = (threadIdx.x & 31) * 2, lr = threadIdx.x >> 5;
    for (int pass = 0; pass < 8; ++pass) {
      const long r = r0 + lr + pass * 8, c = c0 + lc;
      double v[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const long cc = c + e;
        double val;
        if (r < a.n && cc < a.n) {
          const double* p1 = a.x + r * nd;
          const double* p2 = a.x + cc * nd;
          // k(x_min, x_max), the argument order of kmat_generic_tile's symmetric build
          const bool swap = r > cc;
          val = FAST ? gh_fast_value(a.fast[b], swap ? p2 : p1, swap ? p1 : p2)
                     : gh_eval_value(prog, a.n_nodes, swap ? p2 : p1, swap ? p1 : p2);
          if (r == cc) { const double e2 = yerr[r]; val += e2 * e2; }
        } else if (r < a.np) {
          val = (r == cc) ? 1.0 : 0.0;             // identity padding
        } else if (r == a.np) {
          val = cc < a.n ? res[cc] : 0.0;          // the border row: r_b^T
        } else {
          val = 0.0;
        }
        v[e] = val;
      }
      *reinterpret_cast<double2*>(Ab + r * a.ld + c) = make_double2(v[0], v[1]);
    }
    return;
  }
  const long nt = a.np / T;
  const GhNode* prog = a.nodes + (long)b * a.n_nodes;
  const int nd = a.ndim;
  auto kval = [&](const double* p1, const double* p2) -> double {
    return FAST ? gh_fast_value(a.fast[b], p1, p2) : gh_eval_value(prog, a.n_nodes, p1, p2);
  };
  int kind;                                      // 0 K, 1 panel below K, 2 residual-column output, 3 K**
  long TI, TJ, u = 0;
  if (t < a.ktiles) {
    int ti, tj;
    tri_index(t, ti, tj);
    kind = 0; TI = ti; TJ = tj;
  } else if (t < a.ktiles + a.ptiles) {
    const long v = t - a.ktiles;
    kind = 1; TI = nt + v / nt; TJ = v % nt;
  } else if (t < a.ktiles + a.ptiles + a.mt + 1) {
    kind = 2; u = t - a.ktiles - a.ptiles; TI = TJ = 0;
  } else {
    const long v = t - a.ktiles - a.ptiles - a.mt - 1;
    kind = 3; u = a.mt + 1 + v;
    if (a.kss == 1) { TI = TJ = v; } else { int ti, tj; tri_index(v, ti, tj); TI = ti; TJ = tj; }
  }
  const long r0 = TI * T + (quad >> 1) * 64, c0 = TJ * T + (quad & 1) * 64;
  const double* yerr = a.yerr + (long)b * a.n;
  const double* res = a.r + (long)b * a.n;
  double* dst;
  long ld;
  if (kind <= 1) { dst = a.A + (long)b * a.stride + r0 * a.ld + c0; ld = a.ld; }
  else { dst = a.O + (long)b * a.ostride + u * T * T + (quad >> 1) * 64 * T + (quad & 1) * 64; ld = T; }
  const int lc = (threadIdx.x & 31) * 2, lr = threadIdx.x >> 5;
  for (int pass = 0; pass < 8; ++pass) {
    const long r = r0 + lr + pass * 8, c = c0 + lc;
    double v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const long cc = c + e;
      double val = 0.0;
      if (kind == 0) {
        if (r < a.n && cc < a.n) {
          const double* p1 = a.x + r * nd;
          const double* p2 = a.x + cc * nd;
          const bool swap = r > cc;              // k(x_min, x_max), as above
          val = kval(swap ? p2 : p1, swap ? p1 : p2);
          if (r == cc) { const double e2 = yerr[r]; val += e2 * e2; }
        } else {
          val = (r == cc) ? 1.0 : 0.0;           // identity padding
        }
      } else if (kind == 1) {
        const long c_s = r - a.np - T;           // test row index
        if (r == a.np) val = cc < a.n ? res[cc] : 0.0;
        else if (ROWS == 2) val = (c_s == cc) ? 1.0 : 0.0;
        else if (c_s >= 0 && c_s < a.m && cc < a.n) val = kval(a.x + cc * nd, a.xs + c_s * nd);   // k(x_i, xs_c)
      } else if (kind == 3 && ROWS == 1 && r < a.m && cc < a.m) {
        const bool swap = r > cc;                // the one-problem symmetric build: k(xs_min, xs_max), no noise
        val = kval(a.xs + (swap ? cc : r) * nd, a.xs + (swap ? r : cc) * nd);
      }
      v[e] = val;
    }
    *reinterpret_cast<double2*>(dst + (long)(lr + pass * 8) * ld + lc) = make_double2(v[0], v[1]);
  }
}

// ---------------------------------------------------------------------------------------------------- step j
// potf2 of every member's diagonal tile j (the 75-KB LDS body of potf2_inv_mfma_kernel: two workgroups per CU)
__global__ __launch_bounds__(256, 2) void batch_potf2_kernel(double* A, long ld, long stride, double* dinv, long dstride,
                                                             long long* info, int j) {
  const int b = blockIdx.x;
  if (member_failed(info, b)) return;
  __shared__ double s[GH_POTF2_S_DOUBLES];
  __shared__ double dscr[GH_POTF2_D_DOUBLES];
  __shared__ int fail_at;
  const long j0 = (long)j * T;
  (void)gh_potf2::potf2_body(A + (long)b * stride + j0 * ld + j0, ld, dinv + (long)b * dstride + (long)j * T * T, info + b,
                             (long long)j0, s, dscr, &fail_at);
}
// tile (j + 1 + t, j) <- tile L_jj^-T for t < m (K's tiles below the diagonal, the residual tile, carried tiles); blockIdx.x = member * m + t
__global__ __launch_bounds__(256, 2) void batch_trsm_kernel(double* A, long ld, long stride, const double* dinv, long dstride,
                                                            const long long* info, int j, int m) {
  const int b = blockIdx.x / m;
  const long i = j + 1 + (long)(blockIdx.x % m);
  if (member_failed(info, b)) return;
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  double* P = A + (long)b * stride + i * T * ld + (long)j * T;
  gh_tile128_nt_sp<false>(sm, P, ld, P, ld, dinv + (long)b * dstride + (long)j * T * T, T, T);
}
// tile (i, l) -= P_i P_l^T for j < l < tc and l <= i: the trailing triangle over tile columns j + 1 .. tc - 1, then the rectangle
// of the tile rows from tc on (as many as `pairs` covers).  tc = nt: K's triangle, then the residual and carried tiles below K
// (their border columns wait for batch_schur_kernel); tc = nt + 1 (the objective): the residual tile row and the corner tile are
// in the triangle and there is no rectangle.  K = 128; blockIdx.x = member * pairs + pair.
__global__ __launch_bounds__(256, 2) void batch_trap_kernel(double* A, long ld, long stride, const long long* info, int j, int tc,
                                                            long pairs) {
  const int b = (int)(blockIdx.x / pairs);
  if (member_failed(info, b)) return;
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  const long p = (long)(blockIdx.x % pairs), w = tc - j - 1, tri = w * (w + 1) / 2;
  long i, l;
  if (p < tri) {
    int ti, tl;
    tri_index(p, ti, tl);
    i = j + 1 + ti; l = j + 1 + tl;
  } else {
    i = tc + (p - tri) / w; l = j + 1 + (p - tri) % w;
  }
  double* Ab = A + (long)b * stride;
  gh_tile128_nt_sp<true>(sm, Ab + i * T * ld + l * T, ld, Ab + i * T * ld + (long)j * T, ld, Ab + l * T * ld + (long)j * T, ld, T);
}
// After the chain: output tile u of member b, C -= P_a P_b^T with K = np.  u <= mt: panel row tile nt + u against the residual
// tile nt (u = 0: -z^T z at [0][0]; u > 0: -V^T z in column 0); u > mt: carried tiles (c, d) of K** - V^T V (kss 1: the
// diagonal tiles, kss 2: the lower ones).  blockIdx.x = member * q + u.
// KSKIP (the gradient; mt = nt, kss = 2, K** = 0): the carried rows, the identity's, have become W = L^-T, upper triangular:
// W's row tile c is zero left of k-tile c, and each product starts at its first non-zero k-tile (the products skipped are exact
// zeros).  u = 0: K = np as ever; 0 < u <= nt: W's row tile u - 1 against the residual tile: -alpha in column 0; u > nt: lower
// tile (c, d) of -W W^T = -K^-1, from k-tile c on.
// (ldo, the output tiles' pitch, is 128 but a kernel argument: as a constant it lets the compiler fold and keep addresses live
// until the K = np loop spills)
template <bool KSKIP>
__global__ __launch_bounds__(256, 2) void batch_schur_kernel(const double* A, long ld, long stride, double* O, long ostride,
                                                             long ldo, const long long* info, int nt, int mt, int kss, long q) {
  const int b = (int)(blockIdx.x / q);
  if (member_failed(info, b)) return;
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  const long u = (long)(blockIdx.x % q);
  long ia, ib, k0 = 0;
  if (u <= mt) {
    ia = nt + u; ib = nt;
    if (KSKIP && u > 0) k0 = (u - 1) * T;
  } else if (!KSKIP && kss == 1) {
    ia = ib = nt + u - mt;
  } else {
    int ti, tl;
    tri_index(u - mt - 1, ti, tl);
    ia = nt + 1 + ti; ib = nt + 1 + tl;
    if (KSKIP) k0 = (long)ti * T;
  }
  const double* Ab = A + (long)b * stride;
  gh_tile128_nt_sp<true>(sm, O + (long)b * ostride + u * T * T, ldo, Ab + ia * T * ld + k0, ld, Ab + ib * T * ld + k0, ld,
                         ld - k0);
}

// ---------------------------------------------------------------------------------------------------- reductions
// logdet[b] = 2 sum_i log L_b[i][i] over the np diagonal entries in launch_logdet's order (gh_chol.hip: g contiguous slices,
// each summed by 256 lanes and a block reduction, the slices added in index order); quad[b] = -A_b[np][np].  Failed members: NaN.
// (qsrc + b * qstride: where -quad[b] is, A_b[np][np] for the objective, O_b[0][0] for predict)
__global__ __launch_bounds__(256) void batch_reduce_kernel(const double* A, long ld, long stride, long np, const double* qsrc,
                                                           long qstride, const long long* info, double* logdet, double* quad) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const double* Ab = A + (long)b * stride;
  if (member_failed(info, b)) {
    if (threadIdx.x == 0) logdet[b] = quad[b] = __longlong_as_double(0x7FF8000000000000LL);
    return;
  }
  const long g = (np + 2047) / 2048 < 64 ? (np + 2047) / 2048 : 64;
  double tot = 0.0;
  if (g <= 1) {
    double v = 0.0;
    for (long i = threadIdx.x; i < np; i += 256) v += log(Ab[i * ld + i]);
    tot = block_sum_256(v, sh);
  } else {
    const long per = (np + g - 1) / g;
    for (long s = 0; s < g; ++s) {
      const long lo = s * per, hi = lo + per < np ? lo + per : np;
      double v = 0.0;
      for (long i = lo + threadIdx.x; i < hi; i += 256) v += log(Ab[i * ld + i]);
      tot += block_sum_256(v, sh);
    }
  }
  if (threadIdx.x == 0) {
    logdet[b] = 2.0 * tot;
    quad[b] = -qsrc[(long)b * qstride];
  }
}

// predict: the caller's layout.  Element e of member b's [mu (m) | var (m) or cov (m x m)]; blockIdx.x = member * blocks + block.
// cov[c][d] and cov[d][c] read the same lower element: exactly symmetric.  Failed members: NaN.
__global__ __launch_bounds__(256) void batch_pfinal_kernel(const double* O, long ostride, const long long* info, long m, int mt,
                                                           int kss, long per, long blocks, double* mu, double* var, double* cov) {
  const long b = (long)blockIdx.x / blocks;
  const long e = ((long)blockIdx.x % blocks) * 256 + threadIdx.x;
  if (e >= per) return;
  const bool bad = info[b] != 0;
  const double* Ob = O + b * ostride;
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  if (e < m) {
    mu[b * m + e] = bad ? nan : -Ob[(1 + e / T) * T * T + (e % T) * T];
  } else if (kss == 1) {
    const long c = e - m;
    var[b * m + c] = bad ? nan : Ob[(mt + 1 + c / T) * T * T + (c % T) * (T + 1)];
  } else {
    const long c = (e - m) / m, d = (e - m) % m;
    const long lo = c > d ? c : d, hi = c > d ? d : c, ti = lo / T, tj = hi / T;
    cov[b * m * m + c * m + d] = bad ? nan : Ob[(mt + 1 + ti * (ti + 1) / 2 + tj) * T * T + (lo % T) * T + hi % T];
  }
}

// ---------------------------------------------------------------------------------------------------- gradient
// The batched form of gh_kmat.hip's kgrad_reduce_kernel: one 64 x 64 tile of member b's lower triangle per workgroup, member b's
// program, alpha and K^-1 read from its output tiles (negated: exact), the same per-element weights (1/2 on the diagonal) and
// the same wave / cross-wave reduction; one partial row per (member, tile).  The diagonal writes alpha[b] and diagA[b]; a failed
// member gets NaN rows there.  blockIdx.x = member * nblk + tile.
#define GT 64
struct BatchGrad {
  const GhNode* nodes; int n_nodes; int ndim; int P;   // member b's program: nodes + b * n_nodes
  const uint32_t* which;                               // (P), shared by every member
  const double* x; long n;                             // (n, ndim), shared
  const double* O; long ostride; long nt;              // member b's output tiles (batch_schur_kernel<true>): O + b * ostride
  const long long* info;
  double* partial;                                     // (B, nblk, P)
  double* alpha; double* diagA;                        // (B, n)
  long nblk;                                           // 64-tiles of the lower triangle per member
};
template <int PMAX>
__global__ __launch_bounds__(256, PMAX <= 16 ? 4 : 1) void batch_kgrad_kernel(BatchGrad a) {
  __shared__ double xr[GT * GH_MAX_NDIM];
  __shared__ double xc[GT * GH_MAX_NDIM];
  __shared__ double ar[GT], ac[GT];
  __shared__ double red[4][PMAX];
  const int b = (int)(blockIdx.x / a.nblk);
  const long t = (long)(blockIdx.x % a.nblk);
  int ti, tj;
  tri_index(t, ti, tj);
  const long r0 = (long)ti * GT, c0 = (long)tj * GT, n = a.n;
  const int nd = a.ndim, P = a.P;
  if (member_failed(a.info, b)) {
    if (ti == tj && threadIdx.x < GT && r0 + threadIdx.x < n) {
      const double nan = __longlong_as_double(0x7FF8000000000000LL);
      a.alpha[b * n + r0 + threadIdx.x] = nan;
      a.diagA[b * n + r0 + threadIdx.x] = nan;
    }
    return;
  }
  const double* Ob = a.O + (long)b * a.ostride;
  for (int e = threadIdx.x; e < GT * nd; e += 256) {
    const long r = r0 + e / nd;
    xr[e] = (r < n) ? a.x[r * nd + (e % nd)] : 0.0;
    const long c = c0 + e / nd;
    xc[e] = (c < n) ? a.x[c * nd + (e % nd)] : 0.0;
  }
  if (threadIdx.x < GT) {                        // alpha_i = -O[tile 1 + i / 128][i % 128][0]
    const long r = r0 + threadIdx.x, c = c0 + threadIdx.x;
    ar[threadIdx.x] = (r < n) ? -Ob[(1 + r / T) * T * T + (r % T) * T] : 0.0;
    ac[threadIdx.x] = (c < n) ? -Ob[(1 + c / T) * T * T + (c % T) * T] : 0.0;
  }
  __syncthreads();
  const long TI = r0 / T, TJ = c0 / T;           // the 128-tile of -K^-1 that holds this 64-tile
  const double* kt = Ob + (a.nt + 1 + TI * (TI + 1) / 2 + TJ) * T * T + (r0 % T) * T + (c0 % T);
  const GhNode* prog = a.nodes + (long)b * a.n_nodes;
  double acc[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) acc[p] = 0.0;
  const int lc = threadIdx.x & 63;
  const int lr = threadIdx.x >> 6;
#pragma unroll 1
  for (int pass = 0; pass < GT / 4; ++pass) {
    const int rr = lr + pass * 4;
    const long r = r0 + rr, c = c0 + lc;
    if (r < n && c <= r) {
      double g[PMAX];
      // ordered arguments (x_min, x_max) = (x_c, x_r) since c <= r, as kgrad_reduce_kernel
      gh_eval_grad(prog, a.n_nodes, &xc[lc * nd], &xr[rr * nd], g);
      const double kin = -kt[rr * T + lc];
      const double aij = ar[rr] * ac[lc] - kin;
      const double w = (r == c) ? 0.5 * aij : aij;
      if (r == c) { a.diagA[b * n + r] = aij; a.alpha[b * n + r] = ar[rr]; }
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
    a.partial[((long)b * a.nblk + t) * P + p] = a.which[p] ? (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]) : 0.0;
  }
}
// grad[b][p]: the partial rows of member b summed by one workgroup in a fixed-order tree (kgrad_final_kernel's), so a member's
// result depends on nothing but its own rows.  Failed members: NaN.  blockIdx.x = member * P + p.
__global__ __launch_bounds__(256) void batch_kgrad_final_kernel(const double* partial, long nblk, int P, const long long* info,
                                                                double* grad) {
  __shared__ double s[256];
  const int b = blockIdx.x / P, p = blockIdx.x % P;
  if (member_failed(info, b)) {
    if (threadIdx.x == 0) grad[(long)b * P + p] = __longlong_as_double(0x7FF8000000000000LL);
    return;
  }
  const double* pb = partial + (long)b * nblk * P;
  double v = 0.0;
  for (long t = threadIdx.x; t < nblk; t += 256) v += pb[t * P + p];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) grad[(long)b * P + p] = s[0];
}

// ---------------------------------------------------------------------------------------------------- host
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// host results -> the caller's pointer, host or device
static int batch_put(void* dst, const void* src, size_t bytes) {
  if (gh_is_device_ptr(dst)) GH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  else memcpy(dst, src, bytes);
  return GH_OK;
}

// Device views of a call's inputs, staged by batch_stage.
struct BatchInputs {
  const GhNode* nodes;                           // (B, k->nodes.size()): member programs
  const GhFast* fast;                            // (B) fast forms, or nullptr when the structure has none
  const double* x; const double* yerr; const double* r; const double* xs;
};
// The host side both entry points share: member programs (k's structure with each row's parameters, gh_node_set_params: the bits
// of gh_kernel_create), their fast forms, and whichever of x, yerr, r and xs (m rows; none when m == 0) live on the host -- ONE
// host-to-device copy into bb->in, enqueued on st.
static int batch_stage(gh_kernel* k, GhBatchBufs* bb, hipStream_t st, const double* params, long B, const double* x, long n,
                       int ndim, const double* yerr, const double* r, const double* xs, long m, BatchInputs* out) {
  const int nn = (int)k->nodes.size();
  std::vector<double> prow;
  const double* P = params;
  if (k->size > 0 && gh_is_device_ptr(params)) {
    prow.resize((size_t)B * k->size);
    GH_HIP(hipMemcpy(prow.data(), params, prow.size() * sizeof(double), hipMemcpyDeviceToHost));
    P = prow.data();
  }
  const bool x_dev = gh_is_device_ptr(x), e_dev = gh_is_device_ptr(yerr), r_dev = gh_is_device_ptr(r);
  const bool s_dev = m == 0 || gh_is_device_ptr(xs);
  const size_t o_nodes = 0, o_fast = align256((size_t)B * nn * sizeof(GhNode));
  const size_t o_x = o_fast + align256((size_t)B * sizeof(GhFast));
  const size_t o_e = o_x + (x_dev ? 0 : align256((size_t)n * ndim * sizeof(double)));
  const size_t o_r = o_e + (e_dev ? 0 : align256((size_t)B * n * sizeof(double)));
  const size_t o_s = o_r + (r_dev ? 0 : align256((size_t)B * n * sizeof(double)));
  const size_t in_bytes = o_s + (s_dev ? 0 : align256((size_t)m * ndim * sizeof(double)));
  bb->stage.resize(in_bytes);
  char* h = bb->stage.data();
  GhNode* hn = (GhNode*)(h + o_nodes);
  GhFast* hf = (GhFast*)(h + o_fast);
  bool fast = true;
  for (long b = 0; b < B; ++b) {
    GhNode* nodes = hn + b * nn;
    memcpy(nodes, k->nodes.data(), (size_t)nn * sizeof(GhNode));
    const double* row = P + b * k->size;
    for (int i = 0; i < nn; ++i)
      if (nodes[i].op == GH_OP_LEAF) gh_node_set_params(nodes[i], row + nodes[i].poff, row + nodes[i].poff + nodes[i].npar);
    gh_fast_form(nodes, nn, hf + b);
    fast = fast && hf[b].ok;                     // (structural: the same for every member)
  }
  if (!x_dev) memcpy(h + o_x, x, (size_t)n * ndim * sizeof(double));
  if (!e_dev) memcpy(h + o_e, yerr, (size_t)B * n * sizeof(double));
  if (!r_dev) memcpy(h + o_r, r, (size_t)B * n * sizeof(double));
  if (!s_dev) memcpy(h + o_s, xs, (size_t)m * ndim * sizeof(double));
  // (grown once, re-used by every later call of the same or a smaller size)
  GH_CHECK(bb->in.ensure(in_bytes));
  char* d = (char*)bb->in.p;
  GH_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
  out->nodes = (const GhNode*)(d + o_nodes);
  out->fast = fast ? (const GhFast*)(d + o_fast) : nullptr;
  out->x = x_dev ? x : (const double*)(d + o_x);
  out->yerr = e_dev ? yerr : (const double*)(d + o_e);
  out->r = r_dev ? r : (const double*)(d + o_r);
  out->xs = s_dev ? xs : (const double*)(d + o_s);
  return GH_OK;
}

// The shape of one call's panels (the file header has the three).
struct BatchShape {
  long ld, rt;                                   // pitch (np, or np + 128: the corner tile is in the panel) and tile rows
  int rows;                                      // carried below the residual tile: 0 nothing, 1 test rows, 2 identity rows
  long carry0, carry1;                           // carried tile rows in play at step j: carry0 + carry1 * j
  long q; int kss;                               // output tiles per member; the K** ones among them: 0 none, 1 diagonal, 2 lower
  long blocks;                                   // the largest per-member grid of what follows the chain (the launch-size guard)
};
// A call's stream and buffers (gh_chol_batch_begin, by the entry point) and what batch_chain leaves to it, all on the device.
struct BatchChain {
  hipStream_t st; GhBatchBufs* bb; BatchInputs in;
  long B, np, nt, ld, stride;                    // member b's panel: A + b * stride
  double* A;
  double* O; long ostride;                       // member b's output tile u: O + b * ostride + u * 128 * 128
  double* logdet; double* quad; long long* info; // (B) each, contiguous: bb->out
};
// The launch-size guard: no grid of the call may pass 2^31 - 1 workgroups (the build's is the largest of the chain's).
static int batch_guard(const char* who, long B, long nt, const BatchShape& sh) {
  const long tiles = nt * (nt + 1) / 2 + (sh.rt - nt) * nt + sh.q;
  if (B * tiles * 4 > 0x7fffffffL || B * sh.blocks > 0x7fffffffL) {
    gh_set_error("%s: batch too large for one call", who);
    return GH_ERR_BAD_ARG;
  }
  return GH_OK;
}
// Prologue of all three entry points: the launch-size guard, ONE staging copy, the buffers of the panels and output tiles.
static int batch_prepare(gh_kernel* k, const char* who, const double* params, long B, const double* x, long n,
                       int ndim, const double* yerr, const double* r, const double* xs, long m, const BatchShape& sh,
                       BatchChain* c) {
  const long np = gh_round_up(n, T), nt = np / T, ld = sh.ld, tc = ld / T;
  const long stride = sh.rt * T * ld, dstride = nt * T * T;
  GH_CHECK(batch_guard(who, B, nt, sh));
  hipStream_t st = c->st;
  GhBatchBufs* bb = c->bb;
  GH_CHECK(batch_stage(k, bb, st, params, B, x, n, ndim, yerr, r, xs, m, &c->in));
  GH_CHECK(bb->A.ensure((size_t)B * stride * sizeof(double)));
  GH_CHECK(bb->dinv.ensure((size_t)B * dstride * sizeof(double)));
  GH_CHECK(bb->out.ensure((size_t)3 * B * sizeof(double)));
  const bool corner = tc > nt;                   // the one output tile is the panel's corner tile
  if (!corner) GH_CHECK(bb->O.ensure((size_t)B * sh.q * T * T * sizeof(double)));
  double* A = bb->A.d();
  double* dinv = bb->dinv.d();
  c->B = B; c->np = np; c->nt = nt; c->ld = ld; c->stride = stride;
  c->A = A;
  c->O = corner ? A + np * ld + np : bb->O.d();
  c->ostride = corner ? stride : sh.q * T * T;
  c->logdet = bb->out.d();
  c->quad = c->logdet + B;
  c->info = (long long*)(c->logdet + 2 * B);
  return GH_OK;
}
// Build and factorisation chain of all three entry points: every panel and output tile, then three launches per 128-column
// step over every member.
static int batch_chain(gh_kernel* k, long n, int ndim, long m, const BatchShape& sh, BatchChain* c) {
  const long B = c->B, np = c->np, nt = c->nt, ld = c->ld, tc = ld / T, stride = c->stride, dstride = nt * T * T;
  const long ktiles = nt * (nt + 1) / 2, ptiles = (sh.rt - nt) * nt, tiles = ktiles + ptiles + sh.q;
  hipStream_t st = c->st;
  double* A = c->A;
  double* dinv = c->bb->dinv.d();
  const long long* info = c->info;

  // ---- build: K, the residual tile and the carried rows below it, the output tiles
  BatchPBuild a;
  a.nodes = c->in.nodes; a.n_nodes = (int)k->nodes.size(); a.ndim = ndim;
  a.fast = c->in.fast;
  a.x = c->in.x; a.n = n; a.xs = c->in.xs; a.m = m;
  a.yerr = c->in.yerr; a.r = c->in.r;
  a.A = A; a.ld = ld; a.np = np; a.stride = stride;
  a.O = c->O; a.ostride = c->ostride;
  a.mt = (int)(sh.rt - nt - 1); a.kss = sh.kss;
  a.info = c->info; a.ktiles = ktiles; a.ptiles = ptiles; a.tiles = tiles;
  const dim3 gb((unsigned)(B * tiles * 4)), blk(256);
  void (*build)(BatchPBuild) =
      sh.rows == 0 ? (a.fast ? batch_pbuild_kernel<true, 0> : batch_pbuild_kernel<false, 0>)
      : sh.rows == 1 ? (a.fast ? batch_pbuild_kernel<true, 1> : batch_pbuild_kernel<false, 1>)
                     : (a.fast ? batch_pbuild_kernel<true, 2> : batch_pbuild_kernel<false, 2>);
  hipLaunchKernelGGL(build, gb, blk, 0, st, a);
  GH_HIP(hipGetLastError());

  // ---- factorisation of K, the residual tile and the carried rows in play carried along
  for (long j = 0; j < nt; ++j) {
    hipLaunchKernelGGL(batch_potf2_kernel, dim3((unsigned)B), blk, 0, st, A, ld, stride, dinv, dstride, c->info, (int)j);
    const long rows = nt + 1 + sh.carry0 + sh.carry1 * j;     // tile rows in play: K, the residual tile, the carried tiles
    const long below = rows - j - 1;
    hipLaunchKernelGGL(batch_trsm_kernel, dim3((unsigned)(B * below)), blk, 0, st, A, ld, stride, (const double*)dinv, dstride,
                       info, (int)j, (int)below);
    const long w = tc - j - 1;                   // trailing tile columns
    if (w > 0) {
      const long pairs = w * (w + 1) / 2 + (rows - tc) * w;   // their triangle, the rectangle of the rows below it
      hipLaunchKernelGGL(batch_trap_kernel, dim3((unsigned)(B * pairs)), blk, 0, st, A, ld, stride, info, (int)j, (int)tc, pairs);
    }
    GH_HIP(hipGetLastError());
  }
  return GH_OK;
}
// logdet[b] from the factor's diagonal and quad[b] = -(output tile 0)[0][0]
static void batch_logdet_quad(const BatchChain& c) {
  hipLaunchKernelGGL(batch_reduce_kernel, dim3((unsigned)c.B), dim3(256), 0, c.st, (const double*)c.A, c.ld, c.stride, c.np,
                     (const double*)c.O, c.ostride, (const long long*)c.info, c.logdet, c.quad);
}
// [logdet | quad | info]: one copy back, the call's one synchronisation, then the caller's pointers (logdet, quad: optional)
static int batch_finish(const BatchChain& c, double* logdet, double* quad, int64_t* info) {
  const size_t B = (size_t)c.B;
  c.bb->back.resize(3 * B);
  GH_HIP(hipMemcpyAsync(c.bb->back.data(), c.logdet, 3 * B * sizeof(double), hipMemcpyDeviceToHost, c.st));
  GH_HIP(hipStreamSynchronize(c.st));
  const double* hb = c.bb->back.data();
  if (logdet) GH_CHECK(batch_put(logdet, hb, B * sizeof(double)));
  if (quad) GH_CHECK(batch_put(quad, hb + B, B * sizeof(double)));
  GH_CHECK(batch_put(info, hb + 2 * B, B * sizeof(int64_t)));
  return GH_OK;
}
static hipMemcpyKind batch_from_device(const void* dst) {
  return gh_is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
}

extern "C" int gh_chol_objective_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                       const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                       double* logdet, double* quad, int64_t* info) {
  if (!s || !k || nbatch < 0 || n <= 0 || !x || !yerr || !r || !logdet || !quad || !info || (k->size > 0 && !params)) {
    gh_set_error("bad argument to objective_batch");
    return GH_ERR_BAD_ARG;
  }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (nbatch == 0) return GH_OK;
  const long np = gh_round_up(n, T), nt = np / T;
  BatchShape sh;
  sh.ld = np + T; sh.rt = nt + 1; sh.rows = 0; sh.carry0 = sh.carry1 = 0; sh.q = 1; sh.kss = 0; sh.blocks = 0;
  BatchChain c;
  GH_CHECK(gh_chol_batch_begin(s, &c.st, &c.bb));
  GH_CHECK(batch_prepare(k, "objective_batch", params, nbatch, x, n, ndim, yerr, r, nullptr, 0, sh, &c));
  GH_CHECK(batch_chain(k, n, ndim, 0, sh, &c));
  batch_logdet_quad(c);
  GH_HIP(hipGetLastError());
  return batch_finish(c, logdet, quad, info);
}

// tol[b] = m eps max(max_i k_b(xs_i, xs_i), 0): the default threshold of a member's pivoted Cholesky, on the scale of ITS prior
// (gh_chol_sample_conditional's rule).  One workgroup per member.
template <bool FAST>
__global__ __launch_bounds__(256) void batch_prior_tol_kernel(const GhNode* nodes, int n_nodes, const GhFast* fast, int ndim,
                                                              const double* xs, long m, double* tol) {
  __shared__ double sh[4];
  const int b = blockIdx.x;
  const GhNode* prog = nodes + (long)b * n_nodes;
  double v = 0.0;
  for (long i = threadIdx.x; i < m; i += 256) {
    const double* p = xs + i * ndim;
    v = fmax(v, FAST ? gh_fast_value(fast[b], p, p) : gh_eval_value(prog, n_nodes, p, p));
  }
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) tol[b] = ((double)m * 2.220446049250313e-16) * fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// gh_chol_predict_batch up to its results on the device: *d_mu (B, m) and *d_second, var (B, m) or cov (B, m, m) in the caller's
// layout (c.bb->res); kss: 2 cov, 1 var, 0 neither.  batch_finish() is left to the caller.
static int predict_batch_enqueue(gh_chol* s, gh_kernel* k, const double* params, long B, const double* x, int64_t n, int32_t ndim,
                                 const double* yerr, const double* r, const double* xs, int64_t m, int kss, BatchChain& c,
                                 double** d_mu_out, double** d_second_out, long* per_out) {
  const long np = gh_round_up(n, T), nt = np / T, mt = gh_round_up(m, T) / T;
  const long q = mt + 1 + (kss == 2 ? mt * (mt + 1) / 2 : kss == 1 ? mt : 0);     // output tiles per member
  const long per = m + (kss == 2 ? m * m : kss == 1 ? m : 0), fblocks = (per + 255) / 256;
  BatchShape sh;
  sh.ld = np; sh.rt = nt + 1 + mt; sh.rows = 1; sh.carry0 = mt; sh.carry1 = 0; sh.q = q; sh.kss = kss; sh.blocks = fblocks;
  GH_CHECK(gh_chol_batch_begin(s, &c.st, &c.bb));
  GH_CHECK(batch_prepare(k, "predict_batch", params, B, x, n, ndim, yerr, r, xs, m, sh, &c));
  GH_CHECK(batch_chain(k, n, ndim, m, sh, &c));
  if (per > 0) GH_CHECK(c.bb->res.ensure((size_t)B * per * sizeof(double)));
  double* d_mu = per > 0 ? c.bb->res.d() : nullptr;
  double* d_second = per > 0 ? d_mu + B * m : nullptr;            // var (B, m) or cov (B, m, m)
  hipStream_t st = c.st;
  const dim3 blk(256);

  // ---- the border: one launch of K = np tile products, then logdet and the caller's layout
  hipLaunchKernelGGL(batch_schur_kernel<false>, dim3((unsigned)(B * q)), blk, 0, st, (const double*)c.A, c.ld, c.stride, c.O,
                     c.ostride, (long)T, (const long long*)c.info, (int)nt, (int)mt, kss, q);
  batch_logdet_quad(c);
  if (per > 0)
    hipLaunchKernelGGL(batch_pfinal_kernel, dim3((unsigned)(B * fblocks)), blk, 0, st, (const double*)c.O, c.ostride,
                       (const long long*)c.info, (long)m, (int)mt, kss, per, fblocks, d_mu, d_second, d_second);
  GH_HIP(hipGetLastError());
  *d_mu_out = d_mu; *d_second_out = d_second; *per_out = per;
  return GH_OK;
}

extern "C" int gh_chol_predict_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                     const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                     const double* xs, int64_t m, double* mu, double* var, double* cov,
                                     double* logdet, double* quad, int64_t* info) {
  if (!s || !k || nbatch < 0 || n <= 0 || m < 0 || !x || !yerr || !r || (m > 0 && (!xs || !mu)) || !info || (var && cov) ||
      (k->size > 0 && !params)) {
    gh_set_error("bad argument to predict_batch");
    return GH_ERR_BAD_ARG;
  }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (nbatch == 0) return GH_OK;
  const long B = nbatch;
  const int kss = cov ? 2 : var ? 1 : 0;
  BatchChain c;
  double* d_mu = nullptr; double* d_second = nullptr; long per = 0;
  GH_CHECK(predict_batch_enqueue(s, k, params, B, x, n, ndim, yerr, r, xs, m, kss, c, &d_mu, &d_second, &per));
  hipStream_t st = c.st;

  // ---- results: straight into the caller's arrays
  double* second = kss == 2 ? cov : var;
  if (m > 0) GH_HIP(hipMemcpyAsync(mu, d_mu, (size_t)B * m * sizeof(double), batch_from_device(mu), st));
  if (kss) GH_HIP(hipMemcpyAsync(second, d_second, (size_t)B * (per - m) * sizeof(double), batch_from_device(second), st));
  return batch_finish(c, logdet, quad, info);
}

// B rounds of compute + gh_chol_sample_conditional: gh_chol_predict_batch's launches, then -- the covariances staying where they
// are, (B, m, m) in the caller's layout -- one batched pivoted Cholesky (gh_pstrf.hip; one launch for the whole chunk up to
// m = 512) and one GEMM per member for the draws.  A failed member has a NaN covariance: rank -1 and NaN draws.
extern "C" int gh_chol_sample_conditional_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                                const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                                const double* xs, int64_t m, const double* z, int64_t nz, double tol,
                                                double* mu, double* draws, double* fac, int64_t* rank, int64_t* info) {
  if (!s || !k || nbatch < 0 || n <= 0 || m <= 0 || nz <= 0 || !x || !yerr || !r || !xs || !z || !draws || !rank || !info ||
      (k->size > 0 && !params)) {
    gh_set_error("bad argument to sample_conditional_batch");
    return GH_ERR_BAD_ARG;
  }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (nbatch == 0) return GH_OK;
  const long B = nbatch;
  BatchChain c;
  double* d_mu = nullptr; double* d_cov = nullptr; long per = 0;
  GH_CHECK(predict_batch_enqueue(s, k, params, B, x, n, ndim, yerr, r, xs, m, 2, c, &d_mu, &d_cov, &per));
  hipStream_t st = c.st;
  const size_t head = align256((size_t)B * sizeof(double));
  GH_CHECK(c.bb->samp.ensure(head + gh_sample_work_bytes(m, nz, B)));
  double* tol_dev = c.bb->samp.d();
  if (tol < 0.0) {
    if (c.in.fast) hipLaunchKernelGGL(batch_prior_tol_kernel<true>, dim3((unsigned)B), dim3(256), 0, st, c.in.nodes,
                                      (int)k->nodes.size(), c.in.fast, (int)ndim, c.in.xs, (long)m, tol_dev);
    else           hipLaunchKernelGGL(batch_prior_tol_kernel<false>, dim3((unsigned)B), dim3(256), 0, st, c.in.nodes,
                                      (int)k->nodes.size(), c.in.fast, (int)ndim, c.in.xs, (long)m, tol_dev);
    GH_HIP(hipGetLastError());
  }
  if (mu) GH_HIP(hipMemcpyAsync(mu, d_mu, (size_t)B * m * sizeof(double), batch_from_device(mu), st));
  GhSample q{};
  q.cov = d_cov; q.lda = m; q.stride = m * m; q.m = m; q.nbatch = B;
  q.tol = tol; q.tol_dev = tol < 0.0 ? tol_dev : nullptr; q.mu = d_mu;
  q.z = z; q.nz = nz; q.draws = draws; q.fac = fac; q.rank = rank;
  q.work = (char*)c.bb->samp.p + head; q.work_bytes = c.bb->samp.bytes - head;
  GH_CHECK(gh_sample_enqueue(q, st));
  return batch_finish(c, nullptr, nullptr, info);
}

// B rounds of objective + gradient (gh_chol_objective with a gradient, gh_chol.hip): the chain turns the np identity rows into
// W = L^-T; one Schur launch leaves -z^T z, -alpha and the lower tiles of -K^-1 (batch_schur_kernel<true>); then logdet / quad
// and the gradient reduction over all members.
extern "C" int gh_chol_objective_grad_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                            const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                            const uint32_t* which, double* logdet, double* quad, double* grad,
                                            double* alpha, double* diagA, int64_t* info) {
  if (!s || !k || nbatch < 0 || n <= 0 || !x || !yerr || !r || !which || !logdet || !quad || !grad || !info ||
      (k->size > 0 && !params)) {
    gh_set_error("bad argument to objective_grad_batch");
    return GH_ERR_BAD_ARG;
  }
  if (k->size > GH_MAX_GRAD) { gh_set_error("too many kernel parameters (max %d)", GH_MAX_GRAD); return GH_ERR_BAD_ARG; }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (nbatch == 0) return GH_OK;
  const long B = nbatch, np = gh_round_up(n, T), nt = np / T;
  const long q = nt + 1 + nt * (nt + 1) / 2;                                   // output tiles per member
  const int P = k->size;
  const long gm = (n + GT - 1) / GT, nblk = gm * (gm + 1) / 2;
  BatchShape sh;
  sh.ld = np; sh.rt = 2 * nt + 1; sh.rows = 2; sh.carry0 = sh.carry1 = 1; sh.q = q; sh.kss = 2; sh.blocks = nblk;
  BatchChain c;
  GH_CHECK(batch_guard("objective_grad_batch", B, nt, sh));     // (before the handle is touched, as ever; batch_prepare repeats it)
  GH_CHECK(gh_chol_batch_begin(s, &c.st, &c.bb));
  GH_CHECK(batch_prepare(k, "objective_grad_batch", params, B, x, n, ndim, yerr, r, nullptr, 0, sh, &c));
  const size_t which_bytes = align256(sizeof(uint32_t) * (P > 0 ? P : 1));
  GH_CHECK(c.bb->res.ensure((size_t)B * (P + 2 * n) * sizeof(double)));
  GH_CHECK(c.bb->part.ensure(which_bytes + (size_t)B * nblk * (P > 0 ? P : 1) * sizeof(double)));
  double* d_grad = c.bb->res.d();
  double* d_alpha = d_grad + B * P;
  double* d_diagA = d_alpha + B * n;
  uint32_t* d_which = (uint32_t*)c.bb->part.p;
  double* partial = (double*)((char*)c.bb->part.p + which_bytes);
  hipStream_t st = c.st;
  const dim3 blk(256);
  if (P > 0)
    GH_HIP(hipMemcpyAsync(d_which, which, sizeof(uint32_t) * P,
                          gh_is_device_ptr(which) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  GH_CHECK(batch_chain(k, n, ndim, 0, sh, &c));

  // ---- -z^T z, -alpha and -K^-1 in one launch; logdet and quad; the gradient reduction
  hipLaunchKernelGGL(batch_schur_kernel<true>, dim3((unsigned)(B * q)), blk, 0, st, (const double*)c.A, c.ld, c.stride, c.O,
                     c.ostride, (long)T, (const long long*)c.info, (int)nt, (int)nt, 2, q);
  batch_logdet_quad(c);
  BatchGrad g;
  g.nodes = c.in.nodes; g.n_nodes = (int)k->nodes.size(); g.ndim = ndim; g.P = P;
  g.which = d_which; g.x = c.in.x; g.n = n;
  g.O = c.O; g.ostride = c.ostride; g.nt = nt;
  g.info = c.info; g.partial = partial; g.alpha = d_alpha; g.diagA = d_diagA; g.nblk = nblk;
  const dim3 gg((unsigned)(B * nblk));
  if (P <= 4)       hipLaunchKernelGGL(batch_kgrad_kernel<4>, gg, blk, 0, st, g);
  else if (P <= 16) hipLaunchKernelGGL(batch_kgrad_kernel<16>, gg, blk, 0, st, g);
  else              hipLaunchKernelGGL(batch_kgrad_kernel<GH_MAX_GRAD>, gg, blk, 0, st, g);
  if (P > 0)
    hipLaunchKernelGGL(batch_kgrad_final_kernel, dim3((unsigned)(B * P)), blk, 0, st, (const double*)partial, nblk, P,
                       (const long long*)c.info, d_grad);
  GH_HIP(hipGetLastError());

  // ---- results: straight into the caller's arrays
  if (P > 0) GH_HIP(hipMemcpyAsync(grad, d_grad, (size_t)B * P * sizeof(double), batch_from_device(grad), st));
  if (alpha) GH_HIP(hipMemcpyAsync(alpha, d_alpha, (size_t)B * n * sizeof(double), batch_from_device(alpha), st));
  if (diagA) GH_HIP(hipMemcpyAsync(diagA, d_diagA, (size_t)B * n * sizeof(double), batch_from_device(diagA), st));
  return batch_finish(c, logdet, quad, info);
}

