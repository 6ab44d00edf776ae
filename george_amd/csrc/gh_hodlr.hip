// gh_hodlr.hip -- level-batched HODLR solver on one MI355X.
//
// Replaces the reference's recursive, single-threaded HODLR factorisation
// (include/george/hodlr.h: Node ctor :29-66, low_rank_approx :136-221, compute :75-103,
// factorize :223-235, apply_inverse :237-254, solve :107-114; driver src/george/solvers/_hodlr.cpp
// :55-94).  The algebra is the same -- off-diagonal blocks compressed by partially-pivoted ACA with
// randomly chosen rows, leaves factored exactly, one Woodbury step per internal node -- but the
// recursion is turned inside out so that every kernel launch works on ALL nodes of a tree level:
//
//   * the binary tree (hodlr.h:48: internal iff size/2 >= min_size) is built on the host;
//   * ACA for all nodes of a level runs as one launch, one workgroup per node, evaluating kernel
//     rows/columns on the fly (gh_eval.h) -- the N x N matrix is never formed;
//   * (layout note) V is only ever read one level at a time, so VA is stored LEVEL-MAJOR: level l is a
//     contiguous N x R_l row-major block at element offset N * off_l; U is needed both ways -- all
//     shallower levels at once during the factorisation sweep (row-major N x Rtot, UA) and one level
//     at a time in every solve (a level-major copy UL made once at the end of compute()).  With both
//     in the row-major form every level pass of a solve touched all 5 cache lines of a 75-column row
//     for the 3-15 columns it needed.
//   * U and V of every level live in two N x Rtot row-major arrays (UA, VA): column block l holds
//     level l, row i the point i (rows [start, start+half) of a node hold its U_[0] / V_[0], the
//     rest U_[1] / V_[1], zero-padded to the level's max rank).  "Apply the inverse of level l to
//     the U's of all its ancestors" (hodlr.h:95-102) is then ONE multi-column solve on the
//     contiguous column range [0, off_l) of UA;
//   * leaves and the 2r x 2r Woodbury cores S are inverted explicitly once (batched Gauss-Jordan
//     with partial pivoting; log|det| = sum log|pivot| as hodlr.h:87-93), so that every apply is a
//     batched small dense product: reduce (V^T x per 128-row chunk) -> sum -> S^-1 -> update.
//
// Differences from the reference that stay inside its own tolerance criterion (tests compare to
// the dense answer with allclose): one RNG stream per node (the reference threads ONE mt19937
// through the pre-order construction, so the row choices differ); partial-pivot LU / Gauss-Jordan
// instead of Eigen FullPivLU / LDLT; a block whose residual rows have ALL dropped under the 1e-14
// pivot threshold keeps its low-rank factors where the reference switches to the exact block
// (hodlr.h:160-176; same block to 1e-14 per entry, rank r instead of min(rows, cols)).  Ranks grow
// as far as the tolerance asks, up to RANK_CAP = 1024 (the scratch starts at 256 columns and a
// level is redone with twice as many when a block is cut short); a block that would need more, or
// more than a caller-given opts.max_rank, is an ERROR (GH_ERR_BAD_ARG), never a silent truncation.
//
// This unit is the factorisation -- handle, tree, leaf stage, cores, compute().  The ACA kernels, the applies and solves, predict /
// gradient and the split over several devices are units of their own: gh_hodlr_impl.h has the map and what they share.
#include <math.h>
#include <atomic>
#include <memory>
#include "gh_hodlr_impl.h"
#include "gh_device_util.h"
#include "gh_gemm_tile.h"

// B (rows of this level's nodes x R, row-major, ld = R) <- first rank columns of Tcm, zero padded
// All levels in ONE launch (eleven launches of 10-38 us each at C4): workgroups [b0, b0 + nn * ny) belong to the
// level described by a segment; inside it, workgroup (node, y) as in hodlr_compact_kernel below.
struct CompactSeg { const double* Tcm; const LvlNode* nodes; const int* ranks; int R, ny; long off, offv, ldv; int b0, nblk; };
// (the segment table rides in the kernel arguments: uploading it was a copy from pageable memory -- staged and waited for -- between
//  the ranks' arrival on the host and this launch, on the critical path of every compute())
struct CompactSegs { int n; CompactSeg s[24]; };
__global__ void hodlr_compact_all_kernel(const CompactSegs segs, long N, double* UA, long ld, double* VA) {
  int q = 0;
  while (q + 1 < segs.n && (int)blockIdx.x >= segs.s[q].b0 + segs.s[q].nblk) ++q;
  const CompactSeg sg = segs.s[q];
  const int local = (int)blockIdx.x - sg.b0, node = local / sg.ny, by = local % sg.ny;
  const LvlNode nd = sg.nodes[node];
  const int rk = sg.ranks[node], R = sg.R;
  const long tot = (long)nd.size * R;
  for (long e = (long)by * blockDim.x + threadIdx.x; e < tot; e += (long)sg.ny * blockDim.x) {
    const int r = (int)(e / R), k = (int)(e % R);
    const long i = nd.start + r;
    const double v = (k < rk) ? sg.Tcm[(long)k * N + i] : 0.0;
    if (UA) UA[i * ld + sg.off + k] = v;          // (nullptr: the leaf product reads the level-major copy and writes U itself -- LeafSrc)
    VA[i * sg.ldv + sg.offv + k] = v;
  }
}
__global__ void hodlr_compact_kernel(const double* Tcm, long N, const LvlNode* nodes, const int* ranks,
                                     int R, double* UA, long ld, long off, double* VA, long ldv, long offv) {
  const LvlNode nd = nodes[blockIdx.x];
  const int rk = ranks[blockIdx.x];
  const long tot = (long)nd.size * R;
  // (element index split as (row, k), k fastest: the WRITES of a row's R columns are what must be
  //  coalesced -- with one thread per row and coalesced reads of the column-major Tcm the eleven
  //  launches took 558 instead of 185 us)
  for (long e = (long)blockIdx.y * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.y * blockDim.x) {
    const int r = (int)(e / R), k = (int)(e % R);
    const long i = nd.start + r;
    const double v = (k < rk) ? Tcm[(long)k * N + i] : 0.0;
    UA[i * ld + off + k] = v;
    if (VA) VA[i * ldv + offv + k] = v;
  }
}

// ======================================================================== leaves
// pitch == 0: leaf b is stored size x size at leaves[b].off; pitch > 0: in a pitch x pitch slot at
// b * pitch^2, identity-padded (the batched Cholesky path below wants 128 x 128 blocks)
__global__ void hodlr_leaf_build_kernel(const GhNode* __restrict__ prog, int n_prog, GhFast fast, int nd, const double* x,
                                        const double* yerr, const LeafDesc* leaves, double* Lf, int pitch) {
  const LeafDesc lf = leaves[blockIdx.x];
  if (pitch > 0) {
    // (round 5) the leaf's coordinates and noise through LDS first: with both points of every element fetched from global
    // memory inside the loop a thread's eight elements were eight dependent round trips -- 750-860 us for the 2048 leaves of
    // C4 (45 G elements/s; the dense build evaluates 700 G/s), the longest piece of the leaf chain and, through it, of the
    // whole first phase of a step.  Same evaluator, same ordered arguments: same bits.
    __shared__ double xs[256 * 8];
    __shared__ double es[256];
    const bool in_lds = nd <= 8 && lf.size <= 256;
    if (in_lds) {
      for (int t = threadIdx.x; t < lf.size * nd; t += blockDim.x) xs[t] = x[(long)lf.start * nd + t];
      for (int t = threadIdx.x; t < lf.size; t += blockDim.x) es[t] = yerr[lf.start + t];
      __syncthreads();
    }
    const double* const xb = in_lds ? (const double*)xs : x + (long)lf.start * nd;
    double* slot = Lf + (long)blockIdx.x * pitch * pitch;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < pitch * pitch; e += gridDim.y * blockDim.x) {
      const int r = e / pitch, c = e % pitch;
      double v = (r == c) ? 1.0 : 0.0;
      if (r < lf.size && c < lf.size) {
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const double* pa = xb + (long)lo * nd;
        const double* pb = xb + (long)hi * nd;
        v = fast.ok ? gh_fast_value(fast, pa, pb) : gh_eval_value(prog, n_prog, pa, pb);
        if (r == c) { const double e2 = in_lds ? es[r] : yerr[lf.start + r]; v += e2 * e2; }
      }
      slot[e] = v;
    }
    return;
  }
  const long tot = (long)lf.size * lf.size;
  for (long e = (long)blockIdx.y * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.y * blockDim.x) {
    const int r = (int)(e / lf.size), c = (int)(e % lf.size);
    const int lo = r < c ? r : c, hi = r < c ? c : r;        // ordered arguments: exactly symmetric
    const double* pa = x + (long)(lf.start + lo) * nd;
    const double* pb = x + (long)(lf.start + hi) * nd;
    double v = fast.ok ? gh_fast_value(fast, pa, pb) : gh_eval_value(prog, n_prog, pa, pb);
    if (r == c) { const double e2 = yerr[lf.start + r]; v += e2 * e2; }              // hodlr.h:125, _hodlr.cpp:76
    Lf[lf.off + e] = v;
  }
}

// out[b] = 2 * sum_i log L_ii of the b-th 128 x 128 factored slot (identity padding adds 0)
__global__ __launch_bounds__(128) void hodlr_leaf_logdet_kernel(const double* Lf, double* out) {
  __shared__ double sh[8];
  const double* slot = Lf + (long)blockIdx.x * 128 * 128;
  const double v = hw_block_sum(log(slot[threadIdx.x * 129]), sh);
  if (threadIdx.x == 0) out[blockIdx.x] = 2.0 * v;
}

// the same for a 256 x 256 slot factored as 2 x 2 blocks of 128 (both diagonal blocks hold their factors)
__global__ __launch_bounds__(256) void hodlr_leaf_logdet256_kernel(const double* Lf, double* out) {
  __shared__ double sh[8];
  const double* slot = Lf + (long)blockIdx.x * 256 * 256;
  const double v = hw_block_sum(log(slot[threadIdx.x * 257]), sh);
  if (threadIdx.x == 0) out[blockIdx.x] = 2.0 * v;
}

// ---- batched 128 x 128 products of the leaf stage on the dense solver's tile function (round 5)
// C_b (-)= A_b B_b^T for b < gridDim.x: A_b, B_b are 128 x K with k contiguous, one workgroup per product, the LDS-DMA /
// v_mfma_f64_16x16x4 tile of gh_gemm_tile.h.  The leaf stage's products went through hodlr_mm_kernel (a generic 32 x 64 x 32
// tile with register staging: 8-13 TFLOP/s -- 0.67 ms for the 2048 products K^-1 = L^-T L^-1 of C4, 1.1-2.2 ms for each of the
// nine products of 4096 leaves of 171 rows at N = 700000).
template <bool ACC>
__global__ __launch_bounds__(256, 2) void hodlr_bmm_nt_kernel(double* C, long ldc, long sc, const double* A, long lda, long sa,
                                                              const double* B, long ldb, long sb, long K) {
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  const long b = blockIdx.x;
  gh_tile128_nt_sp<ACC>(sm, C + b * sc, ldc, A + b * sa, lda, B + b * sb, ldb, K);
}
// dst_b = src_b^T (128 x 128 each): blockIdx.y = one of the sixteen 32 x 32 tiles, through a padded LDS tile (8.4 KiB: the
// first form staged the whole block -- 132 KiB, one workgroup per CU, 633 us for the 2048 leaves of C4)
__global__ __launch_bounds__(256) void hodlr_transpose128_kernel(const double* src, long lds_, long ss, double* dst, long ldd, long sd) {
  __shared__ double t[32 * 33];
  const double* s = src + (long)blockIdx.x * ss;
  double* d = dst + (long)blockIdx.x * sd;
  const int tr = (blockIdx.y >> 2) * 32, tc = (blockIdx.y & 3) * 32;
  const int c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
#pragma unroll
  for (int q = 0; q < 4; ++q) t[(r0 + 8 * q) * 33 + c] = s[(long)(tr + r0 + 8 * q) * lds_ + tc + c];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) d[(long)(tc + r0 + 8 * q) * ldd + tr + c] = t[c * 33 + r0 + 8 * q];
}

// Batched in-place inverse by Gauss-Jordan with partial (row) pivoting; one workgroup per matrix
// (row-major n x n at base + offs[b]).  logdet[b] = sum log|pivot|.  scratch: n doubles + n ints
// per matrix at sc_off[b].  When the launch provides dynamic LDS (`lds_doubles` >= n * (n|1) + n) the
// matrix is worked on in LDS with an odd row pitch and written back once: the n rank-1 updates
// are then n^3 LDS accesses instead of n^3 L2 round trips (2048 leaves of 128 x 128 at C4:
// 12.9 ms -> well under 1 ms).  Larger matrices (leaves can reach 2 min_size - 1 rows) fall back
// to working in place in HBM.
extern __shared__ double gj_lds[];
__global__ __launch_bounds__(256) void gj_inverse_kernel(double* base, const long* offs, const int* sizes,
                                                         double* scratch_d, int* scratch_i, const long* sc_off,
                                                         double* logdet, int* fail, int lds_doubles) {
  __shared__ double shd[4];
  __shared__ int shi[4];
  const int b = blockIdx.x, n = sizes[b], tid = threadIdx.x;
  double* M = base + offs[b];
  int* piv = scratch_i + sc_off[b];
  const int lane = tid & 63, wave = tid >> 6;
  const bool in_lds = (long)n * (n | 1) + n <= (long)lds_doubles;
  double* W = in_lds ? gj_lds : M;
  double* fcol = in_lds ? gj_lds + (long)n * (n | 1) : scratch_d + sc_off[b];
  const int P = in_lds ? (n | 1) : n;
  if (in_lds) {
    for (int i = wave; i < n; i += 4)
      for (int c = lane; c < n; c += 64) W[(long)i * P + c] = M[(long)i * n + c];
    __syncthreads();
  }
  double ld = 0.0;
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    double best = -1.0;
    int bi = -1;
    for (int i = k + tid; i < n; i += 256) {
      const double a = fabs(W[(long)i * P + k]);
      if (a > best) { best = a; bi = i; }
    }
    hw_block_argmax(best, bi, shd, shi);
    const int p = bi;
    if (!(best > 0.0) || p < 0) { bad = true; break; }     // singular or NaN (uniform)
    if (tid == 0) piv[k] = p;
    if (p != k)
      for (int c = tid; c < n; c += 256) {
        const double t = W[(long)k * P + c];
        W[(long)k * P + c] = W[(long)p * P + c];
        W[(long)p * P + c] = t;
      }
    __syncthreads();
    const double pv = W[(long)k * P + k];
    ld += log(fabs(pv));
    for (int i = tid; i < n; i += 256) fcol[i] = W[(long)i * P + k];
    __syncthreads();
    for (int c = tid; c < n; c += 256) W[(long)k * P + c] = ((c == k) ? 1.0 : W[(long)k * P + c]) / pv;
    for (int i = tid; i < n; i += 256) if (i != k) W[(long)i * P + k] = 0.0;
    __syncthreads();
    // rank-1 update, one wavefront per row (no index divisions; 512-byte row segments per access),
    // the pivot row held in registers
    for (int c0 = 0; c0 < n; c0 += 256) {
      const int c_lo = c0 + lane;
      double rk[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rk[q] = (c_lo + 64 * q < n) ? W[(long)k * P + c_lo + 64 * q] : 0.0;
      for (int i = wave; i < n; i += 4) {
        if (i == k) continue;
        const double fi = fcol[i];
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c_lo + 64 * q < n) W[(long)i * P + c_lo + 64 * q] -= fi * rk[q];
      }
    }
    __syncthreads();
  }
  if (bad) {
    if (tid == 0) { atomicExch(fail, b + 1); logdet[b] = 0.0; }
    return;
  }
  for (int k = n - 1; k >= 0; --k) {                        // undo the row swaps on the columns
    const int p = piv[k];
    if (p != k)
      for (int r = tid; r < n; r += 256) {
        const double t = W[(long)r * P + k];
        W[(long)r * P + k] = W[(long)r * P + p];
        W[(long)r * P + p] = t;
      }
    __syncthreads();
  }
  if (in_lds)
    for (int i = wave; i < n; i += 4)
      for (int c = lane; c < n; c += 64) M[(long)i * n + c] = W[(long)i * P + c];
  if (tid == 0) logdet[b] = ld;
}

// ---- the same inverse for SMALL matrices (n <= NMAX <= 32: the 2r x 2r Woodbury cores), one WAVEFRONT per
// matrix, no barriers, no LDS: lane i holds row i in registers.  gj_inverse_kernel above is built for leaves
// of up to 256 rows -- five workgroup barriers, a block-wide arg-max through LDS and a global write per
// pivot: 3 us per pivot step, 91 us for the 30 x 30 core of the root node, 0.42 ms over the eleven levels
// of C4.  Here a pivot step is a DPP row reduction for the pivot search (on the high words of |a|: as
// unsigned integers they order like the doubles), 2 n v_readlane for the pivot row and n FMAs.
// Rows are not swapped: pivot k is found among the rows not yet used and stays where it is (row p_k plays
// row k of P A); (P A)^-1 = A^-1 P^T, so lane p_r ends with A^-1[r][p_c] in column register c.
__device__ __forceinline__ double gj_bcast(double v, int src_lane) {         // src_lane: wave-uniform, not a constant
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ unsigned gj_row_max_u32(unsigned v) {            // max over the lane's 16-lane row, in every lane
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));   // row_half_mirror
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));   // row_mirror
  return v;
}
template <int NMAX>
// tsum != nullptr: the matrix is not read from `base` but built on the way in as the Woodbury core
// S = [[I, V1^T U1], [V0^T U0, I]] (hodlr.h:229-232) from rows [2 R b, 2 R b + 2 R) x columns [0, R) of tsum
// (pitch Cp) -- what hodlr_sbuild_kernel did in a launch of its own, eleven times per compute().
__global__ __launch_bounds__(256) void gj_small_kernel(double* base, const long* offs, const int* sizes, int nb,
                                                       double* logdet, int* fail, const double* tsum, long Cp, int R) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nb) return;                            // (the whole wavefront)
  const int n = __builtin_amdgcn_readfirstlane(sizes[b]);
  double* const M = base + offs[b];
  const bool row = lane < n;
  double m[NMAX];
  if (tsum) {
    const double* const tr = tsum + ((long)b * n + lane) * Cp;
#pragma unroll
    for (int c = 0; c < NMAX; ++c) {
      double v = (lane == c) ? 1.0 : 0.0;
      if (row && c < n) {
        if (lane < R && c >= R) v = tr[c - R];
        else if (lane >= R && c < R) v = tr[c];
      }
      m[c] = (row && c < n) ? v : 0.0;
    }
  } else {
#pragma unroll
    for (int c = 0; c < NMAX; ++c) m[c] = (row && c < n) ? M[(long)lane * n + c] : 0.0;
  }
  bool used = false, bad = false;
  int myk = 0, pc[NMAX];
  // (round 6) log|det| = sum_k log|pivot_k| in pivot order -- but not INSIDE the pivot loop, where every lane evaluated the same
  // f64 logarithm (~150 instructions) on the critical path of each of the n dependent steps: lane k keeps pivot k, all lanes take
  // their logarithm at once after the loop, lane 0 adds them in the same order (the same bits)
  double mypiv = 1.0;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) {
    if (k < n && !bad) {                          // (uniform)
      const bool cand = row && !used;
      const unsigned key = cand ? (unsigned)__double2hiint(fabs(m[k])) : 0u;
      const unsigned rm = gj_row_max_u32(key);
      const unsigned mx = max((unsigned)__builtin_amdgcn_readlane((int)rm, 0), (unsigned)__builtin_amdgcn_readlane((int)rm, 16));   // n <= 32: two rows
      const unsigned long long who = __builtin_amdgcn_ballot_w64(cand && key == mx);
      const int p = (int)__builtin_ctzll(who | (1ull << 63));
      const double pv = gj_bcast(m[k], p);
      if (who == 0ull || !(fabs(pv) > 0.0)) { bad = true; }
      else {
        pc[k] = p;
        if (lane == p) { used = true; myk = k; }
        if (lane == k) mypiv = pv;
        const double rinv = 1.0 / pv;
        const double f = m[k];
#pragma unroll
        for (int c = 0; c < NMAX; ++c) {
          if (c != k && c < n) {
            const double pr = gj_bcast(m[c], p) * rinv;
            m[c] = (lane == p) ? pr : fma(-f, pr, m[c]);
          }
        }
        m[k] = (lane == p) ? rinv : -f * rinv;
      }
    }
  }
  if (bad) {
    if (lane == 0) { atomicExch(fail, b + 1); logdet[b] = 0.0; }
    return;
  }
  if (row) {
#pragma unroll
    for (int c = 0; c < NMAX; ++c)
      if (c < n) M[(long)myk * n + pc[c]] = m[c];
  }
  {
    const double lg = log(fabs(mypiv));
    double ld = 0.0;
    for (int k = 0; k < n; ++k) ld += gj_bcast(lg, k);
    if (lane == 0) logdet[b] = ld;
  }
}

// The same inverse with ONE WORKGROUP per matrix, its columns dealt over the four wavefronts (column c on wavefront c & 3): for
// the levels with few nodes, where gj_small_kernel leaves one wavefront to walk all n pivots x n columns alone -- 42-46 us for each
// of the three 24..30-row cores at the top of C4's tree, 13-17 us for the 10..14-row ones below them.  The owner of column k
// finds the pivot and puts the column and the pivot row's index in LDS (double-buffered: one barrier per pivot); every
// wavefront then updates its own columns with exactly gj_small_kernel's operations -- a column's arithmetic does not depend
// on which wavefront holds it: the same bits.
template <int NMAX>
__global__ __launch_bounds__(256) void gj_small4_kernel(double* base, const long* offs, const int* sizes, int nb,
                                                        double* logdet, int* fail, const double* tsum, long Cp, int R) {
  constexpr int CW = NMAX / 4;
  __shared__ double fcol[2][64];
  __shared__ int sp[2];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x;
  const int n = __builtin_amdgcn_readfirstlane(sizes[b]);
  double* const M = base + offs[b];
  const bool row = lane < n;
  double m[CW];
  if (tsum) {
    const double* const tr = tsum + ((long)b * n + lane) * Cp;
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const int c = 4 * q + w;
      double v = (lane == c) ? 1.0 : 0.0;
      if (row && c < n) {
        if (lane < R && c >= R) v = tr[c - R];
        else if (lane >= R && c < R) v = tr[c];
      }
      m[q] = (row && c < n) ? v : 0.0;
    }
  } else {
#pragma unroll
    for (int q = 0; q < CW; ++q) { const int c = 4 * q + w; m[q] = (row && c < n) ? M[(long)lane * n + c] : 0.0; }
  }
  bool used = false, bad = false;
  int myk = 0, pcw[CW];
  double mypiv = 1.0;                             // (lane k keeps pivot k: the logarithms are taken after the loop -- see gj_small_kernel)
#pragma unroll
  for (int k = 0; k < NMAX; ++k) {
    if (k < n && !bad) {                          // (uniform over the workgroup: `bad` is set by all wavefronts together)
      const int buf = k & 1, own = k & 3, qk = k >> 2;
      if (w == own) {
        const bool cand = row && !used;
        const unsigned key = cand ? (unsigned)__double2hiint(fabs(m[qk])) : 0u;
        const unsigned rm = gj_row_max_u32(key);
        const unsigned mx = max((unsigned)__builtin_amdgcn_readlane((int)rm, 0), (unsigned)__builtin_amdgcn_readlane((int)rm, 16));
        const unsigned long long who = __builtin_amdgcn_ballot_w64(cand && key == mx);
        const int p = (int)__builtin_ctzll(who | (1ull << 63));
        const double pv = gj_bcast(m[qk], p);
        fcol[buf][lane] = m[qk];
        if (lane == 0) sp[buf] = (who == 0ull || !(fabs(pv) > 0.0)) ? -1 : p;
      }
      __syncthreads();
      const int p = __builtin_amdgcn_readfirstlane(sp[buf]);
      if (p < 0) { bad = true; }
      else {
        const double f = fcol[buf][lane];
        const double pv = fcol[buf][p];
        if (lane == p) { used = true; myk = k; }
        if (lane == k) mypiv = pv;
        const double rinv = 1.0 / pv;
#pragma unroll
        for (int q = 0; q < CW; ++q) {
          const int c = 4 * q + w;
          if (c == k) pcw[q] = p;
          if (c != k && c < n) {
            const double pr = gj_bcast(m[q], p) * rinv;
            m[q] = (lane == p) ? pr : fma(-f, pr, m[q]);
          }
        }
        if (w == own) m[qk] = (lane == p) ? rinv : -f * rinv;
      }
    }
  }
  if (bad) {
    if (threadIdx.x == 0) { atomicExch(fail, b + 1); logdet[b] = 0.0; }
    return;
  }
  if (row) {
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const int c = 4 * q + w;
      if (c < n) M[(long)myk * n + pcw[q]] = m[q];
    }
  }
  if (w == 0) {
    const double lg = log(fabs(mypiv));
    double ld = 0.0;
    for (int k = 0; k < n; ++k) ld += gj_bcast(lg, k);
    if (lane == 0) logdet[b] = ld;
  }
}

extern "C" int gh_hodlr_create(const gh_hodlr_opts* opts, gh_hodlr** out) {
  if (!out) { gh_set_error("null output"); return GH_ERR_BAD_ARG; }
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd HODLR solver needs an MI355X"); return GH_ERR_HIP; }
  gh_hodlr* h = new gh_hodlr();
  memset(&h->opts, 0, sizeof(h->opts));
  if (opts) h->opts = *opts;
  else { h->opts.min_size = 100; h->opts.tol = 0.1; h->opts.seed = 42; }
  if (h->opts.min_size < 1) h->opts.min_size = 1;
  if (h->opts.max_rank < 0) h->opts.max_rank = 0;              // 0: as much as the tolerance asks for, up to RANK_CAP
  if (h->opts.max_rank > RANK_CAP) h->opts.max_rank = RANK_CAP;
  if (hipSetDevice(h->opts.device) != hipSuccess) { delete h; gh_set_error("cannot initialise HIP device %d", opts ? opts->device : 0); return GH_ERR_HIP; }
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  if (gh_shared_streams(h->opts.device, shq) && shq[2] && shq[3]) {
    h->shared_streams = true;                 // the process-wide streams: main, and two side streams for compute()
    h->st = shq[0];
  } else if ((gh_prime_device(h->opts.device), hipStreamCreate(&h->st)) != hipSuccess) {
    delete h; gh_set_error("cannot initialise HIP device %d", opts ? opts->device : 0); return GH_ERR_HIP;
  }
  *out = h;
  return GH_OK;
}
extern "C" void gh_hodlr_destroy(gh_hodlr* h) {
  if (!h) return;
  (void)hipSetDevice(h->opts.device);
  // pooled blocks may be re-acquired by another handle on another stream: nothing of this handle's may
  // still be queued when they are released
  if (h->st) (void)hipStreamSynchronize(h->st);
  if (h->st_b) (void)hipStreamSynchronize(h->st_b);
  if (h->st_c) (void)hipStreamSynchronize(h->st_c);
  if (h->st_d) (void)hipStreamSynchronize(h->st_d);
  if (h->pin) (void)hipHostFree(h->pin);
  delete h;
}

// Ranks and failure flags of ALL levels into one staging buffer, for ONE device-to-host copy: as 22 small
// copies into pageable memory (two per level) they took 22 us each, back to back, with the GPU idle --
// 0.5 of the 6.7 ms of a C4 compute().
struct GatherItem { const int* src; int count, dst; };
__global__ void hodlr_gather_kernel(const GatherItem* items, int* out) {
  const GatherItem it = items[blockIdx.x];
  for (int i = threadIdx.x; i < it.count; i += blockDim.x) out[it.dst + i] = it.src[i];
}

// enqueue only: logdet[b] of matrix b goes to d_logdet[b] (device), a singular block raises h->flags[0]
// (tables: device copies of offs / sizes / scratch offsets kept by the caller; *tables_valid says they
//  already hold this batch's values)
// tsum / tsum_R: see gj_small_kernel (the caller then skips hodlr_sbuild_kernel)
// ---------------------------------------------------------------------------------------------------------------
// (round 6) "sum + core inverse + core product" of one level in ONE launch, a workgroup per node, for the levels with many small
// nodes (C4: levels 5-10, three launches of 5-15 us each per level for a few kFLOP per node):
//   Tsum (2R x C, in LDS only) = the node's chunk partials added up -- hodlr_sum_kernel's order: eight slices of consecutive chunks,
//        each summed from 0.0 in chunk order, then the slice sums in order;
//   S^-1 = the pivoted Gauss-Jordan of gj_small4_kernel (columns over the four wavefronts; a column's arithmetic does not depend on
//        which wavefront holds it), built from Tsum's own-level columns, written to `sinv` for the solves; log|det S| likewise;
//   Tout = S^-1 Tsum[:, 0:Cmm] on the matrix pipe with hodlr_mm_kernel's tile and k order.
// The same doubles through the same operations as the three launches: the same bits (tests/test_gpu_hodlr.py).
template <int NMAX>
__global__ __launch_bounds__(256) void hodlr_core_kernel(const double* __restrict__ P, const int* __restrict__ crange, int R, long Cp, int C,
                                                         int coff, int Cmm, double* __restrict__ sinv, double* __restrict__ logdet,
                                                         int* __restrict__ fail, double* __restrict__ Tout) {
  constexpr int CW = NMAX / 4;
  constexpr int TP = 129;                            // row pitch of the Tsum image (C <= 128)
  __shared__ double ts[NMAX * TP];
  __shared__ double ainv[NMAX * NMAX];
  __shared__ double fcol[2][64];
  __shared__ int sp[2];
  const int node = blockIdx.x, n = 2 * R, tid = threadIdx.x;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // ---- (1) Tsum
  for (int e = tid; e < n * C; e += 256) {
    const int row = e / C, c = e - row * C;
    const int half = row < R ? 1 : 0, k = row < R ? row : row - R;
    const int cb = crange[(node * 2 + half) * 2], ce = crange[(node * 2 + half) * 2 + 1];
    const int per = (ce - cb + SUM_NS - 1) / SUM_NS;
    double t = 0.0;
    for (int q = 0; q < SUM_NS; ++q) {
      const int lo = cb + q * per, hi = lo + per < ce ? lo + per : ce;
      double v = 0.0;
      for (int ch = lo; ch < hi; ++ch) v += P[((long)ch * R + k) * Cp + c];
      t += v;
    }
    ts[row * TP + c] = t;
  }
  __syncthreads();
  // ---- (2) S = [[I, V1^T U1], [V0^T U0, I]] (hodlr.h:229-232) and its inverse: gj_small4_kernel on the LDS image
  const bool row = lane < n;
  double m[CW];
#pragma unroll
  for (int q = 0; q < CW; ++q) {
    const int c = 4 * q + w;
    double v = (lane == c) ? 1.0 : 0.0;
    if (row && c < n) {
      if (lane < R && c >= R) v = ts[lane * TP + coff + c - R];
      else if (lane >= R && c < R) v = ts[lane * TP + coff + c];
    }
    m[q] = (row && c < n) ? v : 0.0;
  }
  bool used = false, bad = false;
  int myk = 0, pcw[CW];
  double mypiv = 1.0;
#pragma unroll
  for (int k = 0; k < NMAX; ++k) {
    if (k < n && !bad) {
      const int buf = k & 1, own = k & 3, qk = k >> 2;
      if (w == own) {
        const bool cand = row && !used;
        const unsigned key = cand ? (unsigned)__double2hiint(fabs(m[qk])) : 0u;
        const unsigned rm = gj_row_max_u32(key);
        const unsigned mx = max((unsigned)__builtin_amdgcn_readlane((int)rm, 0), (unsigned)__builtin_amdgcn_readlane((int)rm, 16));
        const unsigned long long who = __builtin_amdgcn_ballot_w64(cand && key == mx);
        const int p = (int)__builtin_ctzll(who | (1ull << 63));
        const double pv = gj_bcast(m[qk], p);
        fcol[buf][lane] = m[qk];
        if (lane == 0) sp[buf] = (who == 0ull || !(fabs(pv) > 0.0)) ? -1 : p;
      }
      __syncthreads();
      const int p = __builtin_amdgcn_readfirstlane(sp[buf]);
      if (p < 0) { bad = true; }
      else {
        const double f = fcol[buf][lane];
        const double pv = fcol[buf][p];
        if (lane == p) { used = true; myk = k; }
        if (lane == k) mypiv = pv;
        const double rinv = 1.0 / pv;
#pragma unroll
        for (int q = 0; q < CW; ++q) {
          const int c = 4 * q + w;
          if (c == k) pcw[q] = p;
          if (c != k && c < n) {
            const double pr = gj_bcast(m[q], p) * rinv;
            m[q] = (lane == p) ? pr : fma(-f, pr, m[q]);
          }
        }
        if (w == own) m[qk] = (lane == p) ? rinv : -f * rinv;
      }
    }
  }
  if (bad) {                                       // (uniform over the workgroup)
    if (tid == 0) { atomicExch(fail, node + 1); logdet[node] = 0.0; }
    return;
  }
  double* const M = sinv + (long)node * n * n;
  if (row) {
#pragma unroll
    for (int q = 0; q < CW; ++q) {
      const int c = 4 * q + w;
      if (c < n) { M[(long)myk * n + pcw[q]] = m[q]; ainv[myk * n + pcw[q]] = m[q]; }
    }
  }
  if (w == 0) {
    const double lg = log(fabs(mypiv));
    double ld = 0.0;
    for (int k = 0; k < n; ++k) ld += gj_bcast(lg, k);
    if (lane == 0) logdet[node] = ld;
  }
  __syncthreads();
  // ---- (3) Tout = S^-1 Tsum[:, 0:Cmm]: hodlr_mm_kernel's 32 x 64 tile (wavefront w: 16-row block w & 1, 16-column blocks
  //          2 (w >> 1), 2 (w >> 1) + 1), one 32-deep k block (2R <= 32)
  typedef double cm_v4d __attribute__((ext_vector_type(4)));
  const int fr = lane & 15, fk = lane >> 4, bi = w & 1, bj = 2 * (w >> 1);
  for (int c0 = 0; c0 < Cmm; c0 += 64) {
    cm_v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int ar = 16 * bi + fr, k = 4 * kk + fk;
      const double av = (ar < n && k < n) ? ainv[ar * n + k] : 0.0;
      const int cA = c0 + 16 * bj + fr, cB = cA + 16;
      const double b0 = (k < n && cA < Cmm) ? ts[k * TP + cA] : 0.0;
      const double b1 = (k < n && cB < Cmm) ? ts[k * TP + cB] : 0.0;
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rw = 16 * bi + fk + 4 * r;
      if (rw >= n) continue;
      double* const o = Tout + ((long)node * n + rw) * Cp + c0 + 16 * bj + fr;
      if (c0 + 16 * bj + fr < Cmm) o[0] = acc0[r];
      if (c0 + 16 * bj + 16 + fr < Cmm) o[16] = acc1[r];
    }
  }
}
static std::atomic<int> g_hodlr_core_fused{1};
extern "C" int gh_debug_set_hodlr_core_fused(int on) {
  return g_hodlr_core_fused.exchange(on ? 1 : 0);
}

static int batched_inverse(gh_hodlr* h, hipStream_t st, double* base, const std::vector<long>& offs, const std::vector<int>& sizes,
                           double* d_logdet, GhBuf* const* tables = nullptr, bool tables_valid = false,
                           const double* tsum = nullptr, int tsum_R = 0) {
  const int nb = (int)sizes.size();
  if (nb == 0) return GH_OK;
  std::vector<long> sc(nb);
  long tot = 0;
  for (int i = 0; i < nb; ++i) { sc[i] = tot; tot += sizes[i]; }
  GhPooledBuf l_offs, l_sizes, l_sc, d_sd, d_si;
  GhBuf& d_offs = tables ? *tables[0] : (GhBuf&)l_offs;
  GhBuf& d_sizes = tables ? *tables[1] : (GhBuf&)l_sizes;
  GhBuf& d_sc = tables ? *tables[2] : (GhBuf&)l_sc;
  if (!tables || !tables_valid) {
    GH_CHECK(upload(d_offs, offs, st));
    GH_CHECK(upload(d_sizes, sizes, st));
    GH_CHECK(upload(d_sc, sc, st));
  }
  int nmax = 0;
  for (int v : sizes) nmax = std::max(nmax, v);
  if (nmax <= 32 && nb <= 64) {   // few cores (the top levels): a workgroup per matrix, columns over its four wavefronts
    if (nmax <= 16) hipLaunchKernelGGL(gj_small4_kernel<16>, dim3(nb), dim3(256), 0, st, base, (const long*)d_offs.p, (const int*)d_sizes.p, nb, d_logdet, (int*)h->flags.p, tsum, (long)h->cpass, tsum_R);
    else hipLaunchKernelGGL(gj_small4_kernel<32>, dim3(nb), dim3(256), 0, st, base, (const long*)d_offs.p, (const int*)d_sizes.p, nb, d_logdet, (int*)h->flags.p, tsum, (long)h->cpass, tsum_R);
    GH_HIP(hipGetLastError());
    return GH_OK;
  }
  if (nmax <= 32) {                  // the Woodbury cores: one wavefront per matrix
    const dim3 grid((unsigned)((nb + 3) / 4));
    if (nmax <= 8) hipLaunchKernelGGL(gj_small_kernel<8>, grid, dim3(256), 0, st, base, (const long*)d_offs.p, (const int*)d_sizes.p, nb, d_logdet, (int*)h->flags.p, tsum, (long)h->cpass, tsum_R);
    else if (nmax <= 16) hipLaunchKernelGGL(gj_small_kernel<16>, grid, dim3(256), 0, st, base, (const long*)d_offs.p, (const int*)d_sizes.p, nb, d_logdet, (int*)h->flags.p, tsum, (long)h->cpass, tsum_R);
    else hipLaunchKernelGGL(gj_small_kernel<32>, grid, dim3(256), 0, st, base, (const long*)d_offs.p, (const int*)d_sizes.p, nb, d_logdet, (int*)h->flags.p, tsum, (long)h->cpass, tsum_R);
    GH_HIP(hipGetLastError());
    return GH_OK;
  }
  if (tsum) {                                     // (cores too big for the wavefront kernel: build them first)
    GH_CHECK(hodlr_launch_sbuild(tsum, (long)h->cpass, tsum_R, base, nb, st));
  }
  GH_CHECK(d_sd.ensure(tot * sizeof(double)));
  GH_CHECK(d_si.ensure(tot * sizeof(int)));
  // dynamic LDS for the in-LDS path: the largest matrix of the batch if it fits (<= 144 KiB), else none
  size_t lds_bytes = ((size_t)nmax * (nmax | 1) + nmax) * sizeof(double);
  if (lds_bytes > 144 * 1024) lds_bytes = 0;
  if (lds_bytes > 0) {
    static bool attr_set = false;
    if (!attr_set) {
      GH_HIP(hipFuncSetAttribute((const void*)gj_inverse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));
      attr_set = true;
    }
  }
  hipLaunchKernelGGL(gj_inverse_kernel, dim3(nb), dim3(256), lds_bytes, st, base, (const long*)d_offs.p, (const int*)d_sizes.p,
                     d_sd.d(), (int*)d_si.p, (const long*)d_sc.p, d_logdet, (int*)h->flags.p, (int)(lds_bytes / sizeof(double)));
  GH_HIP(hipGetLastError());
  return GH_OK;
}

// ---- the debug switches compute() reads (include/george_amd_debug.h); HodlrCall::sw snapshots them once per call
static std::atomic<int> g_hodlr_leaf_fused{1};      // 128-row leaves of fast-form kernels: evaluated inside the factorisation kernel (0: a build launch first)
extern "C" int gh_debug_set_hodlr_leaf_fused(int on) {
  return g_hodlr_leaf_fused.exchange(on ? 1 : 0);
}
static std::atomic<int> g_hodlr_coop_singles{1};    // clusterable levels that end up with one workgroup per node ride at the end of the cooperative launch
extern "C" int gh_debug_set_hodlr_coop_singles(int on) {
  return g_hodlr_coop_singles.exchange(on ? 1 : 0);
}
// The clusters BELOW the first clustered level get 1 / this of the workgroups the even-load rule deals them (never fewer than two).
// Even load per thread makes every cluster as fast as the root's -- but only the root's chain of ~20 ACA steps is the critical path
// of phase 1; the clusters below it finish earlier whatever they get, and every workgroup of a cluster holds its CU (registers:
// nothing else fits beside it) mostly waiting at cluster barriers.  Half as wide they take longer, still end before the root,
// and the CUs go to the one-workgroup nodes and the leaves: C4 3.48 -> 3.40 ms, 1 048 576 17.9 -> 17.4, never slower
// (profiles/r06/hodlr_coop_lower_ab.md; a quarter: 4.02 ms -- then they outlast the root).
static std::atomic<int> g_hodlr_coop_lower{2};
extern "C" int gh_debug_set_hodlr_coop_lower(int div) {
  return g_hodlr_coop_lower.exchange(div < 1 ? 2 : div);
}
static std::atomic<int> g_hodlr_u_from_v{1};        // the factorisation's leaf product reads the level-major V and writes U for the first time (no U from the compaction)
extern "C" int gh_debug_set_hodlr_u_from_v(int on) {
  return g_hodlr_u_from_v.exchange(on ? 1 : 0);
}
static std::atomic<int> g_hodlr_lpt{1};             // the one-workgroup ACA launch takes a level's nodes longest first (durations of the handle's previous compute())
extern "C" int gh_debug_set_hodlr_lpt(int on) {
  return g_hodlr_lpt.exchange(on ? 1 : 0);
}
static std::atomic<int> g_hodlr_coop_wgs{256};      // workgroups of the cooperative ACA launch (<= CUs: every cluster resident)
extern "C" int gh_debug_set_hodlr_coop_wgs(int n) {
  return g_hodlr_coop_wgs.exchange(n < 32 ? 32 : (n > 256 ? 256 : n));
}
// 1 (default): the deep levels whose blocks have <= 256 rows and columns through hodlr_aca_wave_kernel; 0: every level through the
// workgroup kernel (A/B and the same-bits test)
static std::atomic<int> g_hodlr_wave_aca{1};
extern "C" int gh_debug_set_hodlr_wave_aca(int on) {
  return g_hodlr_wave_aca.exchange(on ? 1 : 0);
}
// 1: leaves of 129 .. 256 rows through the pivoted Gauss-Jordan in place (the path every leaf of more than 256 rows takes)
// instead of the 2 x 2 blocked Cholesky: validation arm, tests/test_gpu_hodlr.py
static std::atomic<int> g_hodlr_leaf_gj{0};
extern "C" int gh_debug_set_hodlr_leaf_gj(int on) {
  return g_hodlr_leaf_gj.exchange(on ? 1 : 0);
}

// ================================================================================ compute()
// The HODLR switches as ONE compute() sees them, read once at its start (gh_hodlr_mgpu_compute runs compute() of several sub-tree
// handles on threads of their own: a setter that reached one of them halfway would give it a mix of settings).
struct HodlrSwitches { int leaf_fused, leaf_gj, coop_singles, coop_lower, coop_wgs, u_from_v, lpt, wave_aca, core_fused, passes; };
struct AcaLevel { GhPooledBuf Tcm, idx, sync, part; int G = 1, rcap = 0; int flags[2] = {0, 0}; char* syncp = nullptr; bool sync_cleared = false;
                  bool timed = false; };   // timed: its nodes wrote their durations behind the two flags (the one-workgroup launch)
// ACA_MULTI bit 0: batched candidate search (one-workgroup nodes); bit 1: clusters draw the next row before the norms barrier
static const int ACA_PSTRIDE = 8 + 2 * ACA_MAXR, ACA_FENCE = 0, ACA_MULTI = 3;   // (fence-free cluster barrier, 8 then 64 candidate rows per search pass: DESIGN.md section 4)

// What the phases of one compute() share.  The destructor is its one join point: on any way out but the successful one it
// synchronises every stream of the handle BEFORE the members below release their blocks into the process-wide cache, where
// another handle -- a sibling sub-tree thread of gh_hodlr_mgpu_compute among them -- may pick one up while a side stream still
// writes it.  A successful compute() has joined the side streams into h->st and synchronised that already.
struct HodlrCall {
  gh_hodlr* const h;
  gh_kernel* const k;
  const int64_t n;
  const int32_t ndim;
  const HodlrSwitches sw{g_hodlr_leaf_fused, g_hodlr_leaf_gj, g_hodlr_coop_singles, g_hodlr_coop_lower, g_hodlr_coop_wgs, g_hodlr_u_from_v,
                         g_hodlr_lpt, g_hodlr_wave_aca, g_hodlr_core_fused, hodlr_passes()};
  int l0 = 0, nlev = 0, rcap0 = 0;
  bool concurrent = false, user_cap = false;
  std::vector<AcaLevel> al;
  GhPooledBuf shared_Tcm;                              // serial mode: the scratch the levels take in turn
  GhPooledBuf sync_all;                                // the levels' barrier counters / selections / flags: one buffer, ONE memset
  std::vector<std::unique_ptr<GhPooledBuf>> levelB;   // serial mode: a level's factors parked in a compact buffer
  GhPooledBuf linv, lstk, l22b, lwk;                   // the leaf stage's work blocks (129..256-row leaves)
  size_t n_blocks = 0, ld_at = 0;                      // blocks whose log|det| goes to h->ld_all; the next free slot there
  std::vector<size_t> top_ld;                          // where in ld_all the core of pseudo-level l put its log|det|
  bool leaves_done = false, u_from_v = false, ok = false;
  HodlrCall(gh_hodlr* h_, gh_kernel* k_, int64_t n_, int32_t ndim_) : h(h_), k(k_), n(n_), ndim(ndim_) {}
  ~HodlrCall() { if (!ok) for (hipStream_t s : {h->st, h->st_b, h->st_c, h->st_d}) if (s) (void)hipStreamSynchronize(s); }
  // phase stamps on stderr (how the stalls of the split tree were found): a build-time aid, -DGH_HODLR_PHASE_MARKS
#ifdef GH_HODLR_PHASE_MARKS
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(const char* what) const {
    fprintf(stderr, "[hodlr %p] %s at %.2f ms\n", (void*)h, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
#else
  void mark(const char*) const {}
#endif
};

static int load_inputs(HodlrCall& c, const double* x, const double* yerr) {
  gh_hodlr* const h = c.h;
  GH_HIP(hipSetDevice(h->opts.device));
  GH_CHECK(c.k->upload());
  h->computed = false; h->n = c.n; h->ndim = c.ndim;
  GH_CHECK(h->x.ensure((size_t)c.n * c.ndim * sizeof(double)));
  GH_CHECK(h->yerr.ensure((size_t)c.n * sizeof(double)));
  GH_CHECK(gh_to_device(h->x.d(), x, (size_t)c.n * c.ndim, h->st));
  GH_CHECK(gh_to_device(h->yerr.d(), yerr, (size_t)c.n, h->st));
  GH_CHECK(h->scal.ensure(64));
  c.mark("inputs enqueued");
  return GH_OK;
}

// ---- tree (hodlr.h:47-64), breadth first; kept from the previous compute() when n and min_size are the same
static int build_tree(HodlrCall& c) {
  gh_hodlr* const h = c.h;
  const int64_t n = c.n;
  const int min_size = h->opts.min_size;
  const int l0 = c.l0 = h->sub.depth;            // levels [0, l0) are the pseudo-levels of a sub-tree handle (HSub)
  if (l0 > 0 && ((int)h->sub.half.size() != l0 || (int)h->sub.R.size() != l0 || (int)h->sub.T.size() != l0 || !h->sub.allreduce)) {
    gh_set_error("HODLR: incomplete sub-tree description"); return GH_ERR_BAD_ARG;
  }
  if (h->tree_n != n || h->tree_min != min_size || h->tree_sub != h->sub.sig()) {
    h->reset_tree();
    h->nodes.push_back({0, (int)n, (int)n / 2, l0, 0});
    for (size_t q = 0; q < h->nodes.size(); ++q) {
      HNode nd = h->nodes[q];
      if (nd.half >= min_size) {
        h->nodes.push_back({nd.start, nd.half, nd.half / 2, nd.level + 1, 0});
        h->nodes.push_back({nd.start + nd.half, nd.size - nd.half, (nd.size - nd.half) / 2, nd.level + 1, 0});
        if ((int)h->levels.size() <= nd.level) h->levels.resize(nd.level + 1, nullptr);
        if (!h->levels[nd.level]) h->levels[nd.level] = new HLevel();
        h->levels[nd.level]->node_ids.push_back((int)q);
      } else {
        h->nodes[q].is_leaf = 1;
        long off = h->leaves.empty() ? 0 : h->leaves.back().off + (long)h->leaves.back().size * h->leaves.back().size;
        h->leaves.push_back({nd.start, nd.size, off});
      }
    }
    // pseudo-levels: the ancestor at level l, cut down to the local rows -- one of its halves is empty here
    if ((int)h->levels.size() < l0) h->levels.resize(l0, nullptr);
    for (int l = 0; l < l0; ++l) {
      h->levels[l] = new HLevel();
      h->levels[l]->top = true;
      h->levels[l]->top_level = l;
      h->levels[l]->node_ids.push_back((int)h->nodes.size());
      h->nodes.push_back({0, (int)n, h->sub.half[l] == 0 ? (int)n : 0, l, 0});
    }
    h->tree_n = n; h->tree_min = min_size; h->tree_sub = h->sub.sig();
  }
  h->max_leaf = 0;
  for (auto& lf : h->leaves) h->max_leaf = std::max(h->max_leaf, lf.size);
  c.nlev = (int)h->levels.size();
  c.top_ld.assign(l0, (size_t)-1);
  // log|det| of every factored block (leaves, then the cores level by level) is collected in ld_all
  // on the device and summed on the host after the ONE synchronisation that ends compute(); failure
  // flags likewise (flags[0]: singular Gauss-Jordan block, flags[2..3]: leaf Cholesky info).
  c.n_blocks = h->leaves.size();
  for (auto* L : h->levels) c.n_blocks += L->node_ids.size();
  GH_CHECK(h->ld_all.ensure(std::max<size_t>(c.n_blocks, 1) * sizeof(double)));
  GH_CHECK(h->flags.ensure(4 * sizeof(int)));
  GH_HIP(hipMemsetAsync(h->ld_all.p, 0, std::max<size_t>(c.n_blocks, 1) * sizeof(double), h->st));
  GH_HIP(hipMemsetAsync(h->flags.p, 0, 4 * sizeof(int), h->st));
  c.mark("tree built");
  return GH_OK;
}

// ---- leaves: exact blocks -> explicit inverses + log-dets (hodlr.h:223-227, 87-89), all on stream st.
// The leaf stage (build, batched Cholesky + inverse, K^-1 = L^-T L^-1: 1.4 ms at C4) depends on nothing the ACA produces, so
// it is issued on a side stream under the ACA of the top levels when the levels run concurrently.
// The leaf job table: leaf i's inverse at i * slot, or at its own offset lf.off (slot 0).
static std::vector<MMJob> leaf_jobs(const gh_hodlr* h, size_t slot) {
  std::vector<MMJob> jobs;
  for (const LeafDesc& lf : h->leaves) jobs.push_back({slot ? (long)(jobs.size() * slot) : lf.off, lf.start, lf.start, lf.size, lf.size});
  return jobs;
}
// Leaves are symmetric positive definite and fit the dense solver's 128 x 128 diagonal-block
// kernel: build them identity-padded into 128 x 128 slots, factor + invert the factors as ONE
// batched launch of potf2_inv_mfma_kernel (79 us per block, a workgroup each), log-det from the
// factor's diagonal, K^-1 = L^-T L^-1 as one batched product.  (Gauss-Jordan with pivoting, the
// general path below, spends 7 ms on the 2048 leaves of C4; this one ~1.5 ms.)
static int leaves_128(HodlrCall& c, hipStream_t st) {
  gh_hodlr* const h = c.h;
  const int nl = (int)h->leaves.size();
  const size_t slot = (size_t)128 * 128;
  GH_CHECK(h->leaf_inv.ensure(nl * slot * sizeof(double)));
  long long* d_info = (long long*)((int*)h->flags.p + 2);
  if (!h->leaf_tab_up) GH_CHECK(upload(h->d_leaves, h->leaves, st));
  // K_leaf^-1 = L^-T L^-1 and log|K_leaf| in ONE launch per batch: gh_potf2.hip, potf2_kinv_kernel (round 6; it was the build + the
  // batched factorisation + a log-det kernel + a batched transpose + a batched product: five launches, 2.3 GB through the L2s).
  // Kernels of the a + b F(r^2) form are evaluated INSIDE that launch; the others keep the build launch in front of it.
  static_assert(sizeof(LeafDesc) == 16, "potf2_kinv_kernel reads LeafDesc as {int start, size; long off}");
  if (c.k->fast.ok && c.sw.leaf_fused) {
    GH_CHECK(gh_launch_potf2_kinv_kernel_batched(h->leaf_inv.d(), 128, (int64_t)slot, h->ld_all.d() + c.ld_at, d_info, nl, c.k->fast,
                                                 h->x.d(), h->yerr.d(), c.ndim, h->d_leaves.p, st));
  } else {
    hipLaunchKernelGGL(hodlr_leaf_build_kernel, dim3(nl, 8), dim3(256), 0, st, c.k->d_nodes, (int)c.k->nodes.size(), c.k->fast, c.ndim,
                       h->x.d(), h->yerr.d(), (const LeafDesc*)h->d_leaves.p, h->leaf_inv.d(), 128);
    GH_HIP(hipGetLastError());
    GH_CHECK(gh_launch_potf2_kinv_batched(h->leaf_inv.d(), 128, (int64_t)slot, h->ld_all.d() + c.ld_at, d_info, nl, st));
  }
  c.ld_at += nl;
  if (!h->leaf_tab_up) { GH_CHECK(upload(h->d_leaf_jobs, leaf_jobs(h, slot), st)); h->leaf_tab_up = true; }
  h->leaf_pitch = 128;
  return GH_OK;
}
// Leaves of 129 .. 256 rows -- the reference's tree stops splitting below 2 min_size, so with min_size = 100 most problem
// sizes have leaves of up to 199 rows (N = 50000: 256 leaves of 195 / 196) -- went through the pivoted Gauss-Jordan in place
// in HBM: 14 of the 17 ms of a step at N = 50000 (round 5 profile).  Same recipe as above on 256 x 256 identity-padded slots,
// as 2 x 2 blocks of 128 with the batched kernels there are:  L11 = chol(A11);  W = L21^T = L11^-1 A12;  A22 -= W^T W;
// L22 = chol(A22);  L^-1 = [[L11^-1, 0], [X, L22^-1]],  X = -L22^-1 L21 L11^-1;  K^-1 = L^-T L^-1 block by block
// (the full symmetric matrix is stored: the products read rows and, by symmetry, columns).
static int leaves_256(HodlrCall& c, hipStream_t st) {
  gh_hodlr* const h = c.h;
  const int nl = (int)h->leaves.size();
  const size_t slot = (size_t)256 * 256, blk = (size_t)128 * 128;
  GH_CHECK(h->leaf_inv.ensure(nl * slot * sizeof(double)));
  GH_CHECK(c.lstk.ensure(nl * 2 * blk * sizeof(double)));        // per leaf Z = [L11^-T | X'^T]  (128 x 256), X' = L22^-1 L21 L11^-1 = -X
  GH_CHECK(c.l22b.ensure(nl * 2 * blk * sizeof(double)));        // L22^-1, L22^-T
  GH_CHECK(c.lwk.ensure(nl * 2 * blk * sizeof(double)));         // L21, T^T
  long long* d_info = (long long*)((int*)h->flags.p + 2);
  if (!h->leaf_tab_up) GH_CHECK(upload(h->d_leaves, h->leaves, st));
  hipLaunchKernelGGL(hodlr_leaf_build_kernel, dim3(nl, 16), dim3(256), 0, st, c.k->d_nodes, (int)c.k->nodes.size(), c.k->fast, c.ndim,
                     h->x.d(), h->yerr.d(), (const LeafDesc*)h->d_leaves.p, h->leaf_inv.d(), 256);
  GH_HIP(hipGetLastError());
  double* const S = h->leaf_inv.d();
  if (!h->leaf_tab_up) { GH_CHECK(upload(h->d_leaf_jobs, leaf_jobs(h, slot), st)); h->leaf_tab_up = true; }
  // work blocks per leaf: Z = [L11^-T | X'^T] (128 x 256, k contiguous), L11^-1, L21 then T^T, L22^-1, L22^-T
  GH_CHECK(c.linv.ensure(nl * blk * sizeof(double)));          // L11^-1 (row-major, from the factorisation kernel)
  double* const Z = c.lstk.d();                                // pitch 256
  double* const W = c.lwk.d();                                 // block 0: L21, block 1: T^T   (pitch 128)
  double* const L22 = c.l22b.d();
  const long s2 = (long)slot, sZ = (long)(2 * blk), sW = (long)(2 * blk), sb = (long)blk;
#define GH_BMM(ACC, C_, ldc_, sc_, A_, lda_, sa_, B_, ldb_, sb_, K_)                                                              \
  hipLaunchKernelGGL(hodlr_bmm_nt_kernel<ACC>, dim3(nl), dim3(256), 0, st, C_, (long)(ldc_), (long)(sc_), (const double*)(A_), (long)(lda_), (long)(sa_), \
                     (const double*)(B_), (long)(ldb_), (long)(sb_), (long)(K_))
  GH_CHECK(gh_launch_potf2_batched(S, 256, (int64_t)slot, c.linv.d(), (int64_t)blk, d_info, nl, st));                            // L11 in place, L11^-1
  hipLaunchKernelGGL(hodlr_transpose128_kernel, dim3(nl, 16), dim3(256), 0, st, (const double*)c.linv.d(), 128L, sb, Z, 256L, sZ); // Z[:, 0:128] = L11^-T
  GH_BMM(false, W, 128, sW, S + 128 * 256, 256, s2, c.linv.d(), 128, sb, 128);                                                   // L21 = A21 L11^-T
  GH_BMM(true, S + 128 * 256 + 128, 256, s2, W, 128, sW, W, 128, sW, 128);                                                       // A22 -= L21 L21^T
  GH_CHECK(gh_launch_potf2_batched(S + 128 * 256 + 128, 256, (int64_t)slot, L22, (int64_t)(2 * blk), d_info, nl, st));          // L22 in place, L22^-1
  hipLaunchKernelGGL(hodlr_leaf_logdet256_kernel, dim3(nl), dim3(256), 0, st, (const double*)S, h->ld_all.d() + c.ld_at);
  c.ld_at += nl;
  hipLaunchKernelGGL(hodlr_transpose128_kernel, dim3(nl, 16), dim3(256), 0, st, (const double*)L22, 128L, sZ, L22 + blk, 128L, sZ); // L22^-T
  GH_BMM(false, W + blk, 128, sW, Z, 256, sZ, W, 128, sW, 128);                                                                   // T^T = L11^-T L21^T   (T = L21 L11^-1)
  GH_BMM(false, Z + 128, 256, sZ, W + blk, 128, sW, L22, 128, sZ, 128);                                                           // X'^T = T^T L22^-T    (X' = L22^-1 T = -X)
  GH_HIP(hipMemsetAsync(S, 0, nl * slot * sizeof(double), st));                                                                  // (both factors are used up; K21, K12 are formed by subtraction)
  GH_BMM(false, S, 256, s2, Z, 256, sZ, Z, 256, sZ, 256);                                                                         // K11 = L11^-T L11^-1 + X^T X
  GH_BMM(false, S + 128 * 256 + 128, 256, s2, L22 + blk, 128, sZ, L22 + blk, 128, sZ, 128);                                       // K22 = L22^-T L22^-1
  GH_BMM(true, S + 128 * 256, 256, s2, L22 + blk, 128, sZ, Z + 128, 256, sZ, 128);                                                // K21 = L22^-T X = -L22^-T X'
  GH_BMM(true, S + 128, 256, s2, Z + 128, 256, sZ, L22 + blk, 128, sZ, 128);                                                      // K12 = K21^T
#undef GH_BMM
  GH_HIP(hipGetLastError());
  h->leaf_pitch = 256;
  return GH_OK;
}
// Every other leaf set (leaves of more than 256 rows, and the leaf_gj validation arm): the pivoted Gauss-Jordan in place, each
// inverse at pitch = its own size, then repacked to pitch max_leaf when the sizes differ (hodlr_mm_kernel takes one A pitch
// per launch)
static int leaves_gj(HodlrCall& c, hipStream_t st) {
  gh_hodlr* const h = c.h;
  const int nl = (int)h->leaves.size();
  const long tot = h->leaves.back().off + (long)h->leaves.back().size * h->leaves.back().size;
  GH_CHECK(h->leaf_inv.ensure(tot * sizeof(double)));
  GH_CHECK(upload(h->d_leaves, h->leaves, st));
  hipLaunchKernelGGL(hodlr_leaf_build_kernel, dim3(nl, 8), dim3(256), 0, st, c.k->d_nodes, (int)c.k->nodes.size(), c.k->fast, c.ndim,
                     h->x.d(), h->yerr.d(), (const LeafDesc*)h->d_leaves.p, h->leaf_inv.d(), 0);
  GH_HIP(hipGetLastError());
  std::vector<long> offs(nl); std::vector<int> sizes(nl);
  for (int i = 0; i < nl; ++i) { offs[i] = h->leaves[i].off; sizes[i] = h->leaves[i].size; }
  GH_CHECK(upload(h->d_leaf_jobs, leaf_jobs(h, 0), st));
  GH_CHECK(batched_inverse(h, st, h->leaf_inv.d(), offs, sizes, h->ld_all.d() + c.ld_at));
  c.ld_at += nl;
  bool uniform = true;
  for (auto& lf : h->leaves) if (lf.size != h->max_leaf) uniform = false;
  if (!uniform) {
    const int ml = h->max_leaf;
    GhBuf packed;
    GH_CHECK(packed.ensure((size_t)nl * ml * ml * sizeof(double)));
    GH_HIP(hipMemsetAsync(packed.p, 0, (size_t)nl * ml * ml * sizeof(double), st));
    for (int i = 0; i < nl; ++i) {
      const LeafDesc& lf = h->leaves[i];
      GH_HIP(hipMemcpy2DAsync(packed.d() + (size_t)i * ml * ml, ml * sizeof(double), h->leaf_inv.d() + lf.off,
                              lf.size * sizeof(double), lf.size * sizeof(double), lf.size, hipMemcpyDeviceToDevice, st));
    }
    GH_HIP(hipStreamSynchronize(st));
    std::swap(h->leaf_inv.p, packed.p);
    std::swap(h->leaf_inv.bytes, packed.bytes);
    GH_CHECK(upload(h->d_leaf_jobs, leaf_jobs(h, (size_t)ml * ml), st));
  }
  h->leaf_pitch = h->max_leaf;
  return GH_OK;
}
static int leaf_stage(HodlrCall& c, hipStream_t st) {
  const int ml = c.h->max_leaf;
  GH_CHECK(ml <= 128 ? leaves_128(c, st) : ml <= 256 && !c.sw.leaf_gj ? leaves_256(c, st) : leaves_gj(c, st));
  c.leaves_done = true;
  return GH_OK;
}

// side stream `which` of the handle (1: st_b, 2: st_c -- its own or the process-wide ones; 3: st_d -- the process-wide chain
// stream only) and its event, made on first use; one that cannot be had stays null
static void ensure_side_stream(gh_hodlr* h, int which) {
  hipStream_t& s = which == 1 ? h->st_b : which == 2 ? h->st_c : h->st_d;
  hipEvent_t& e = which == 1 ? h->ev_b : which == 2 ? h->ev_c : h->ev_d;
  if (s) return;
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  if (h->shared_streams) { if (gh_shared_streams(h->opts.device, shq)) s = shq[which == 1 ? 2 : which == 2 ? 3 : 1]; }
  else if (which < 3 && hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
  if (s && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) s = nullptr;
  if (!s) (void)hipGetLastError();
}

// ---- ACA of every level into column-major scratch, ranks back to the host
// Column capacity of the scratch: the caller's cap, else 256 to start with (doubled, up to RANK_CAP,
// for a level one of whose blocks is cut short by it -- that level is then redone).
// The levels are independent, so they are all ENQUEUED before the host looks at any result: the
// clustered levels (several workgroups per node, spin barriers: they must not share the chip with
// another spinning grid) one after the other on the solver's stream, the one-workgroup-per-node
// levels beside them on a second stream; one synchronisation instead of one per level (each cost
// a ~60 us bubble, and levels 8-10 of C4 -- 1.4 ms -- now run under levels 0-7).  Every level
// gets its own n x rcap scratch; if that is more than 12 GiB in total the levels share one and go
// one at a time.
static int plan_aca(HodlrCall& c) {
  gh_hodlr* const h = c.h;
  const int nlev = c.nlev, l0 = c.l0;
  c.user_cap = h->opts.max_rank > 0;
  c.rcap0 = c.user_cap ? h->opts.max_rank : std::min(256, RANK_CAP);
  // (round 5: "more than 12 GiB" was a 64-GB-card habit; an MI355X has 288 GB.  Above 12 GiB the question is put to the device:
  //  all levels at once while their scratch fits in 40 % of what is free now -- N = 700000 went one level at a time, 34 ms)
  c.concurrent = nlev - l0 > 1;
  const double need = (double)c.n * c.rcap0 * sizeof(double) * (nlev - l0);
  if (c.concurrent && need > 12.0 * (1u << 30)) {
    size_t free_b = 0, tot_b = 0;
    if (hipMemGetInfo(&free_b, &tot_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    // (blocks parked in the pool by the previous compute() of this handle count as used there and are what will be handed out again)
    c.concurrent = need <= 0.4 * (double)free_b + (double)gh_pool_parked_bytes();
  }
  if (c.concurrent) { ensure_side_stream(h, 1); c.concurrent = h->st_b != nullptr; }   // (no second stream: one level at a time)
  c.al.resize(nlev);
  c.levelB.resize(nlev);
  if ((int)h->wave_bad.size() != nlev) h->wave_bad.assign(nlev, 0);
  h->Rtot = 0; h->maxR = 0; h->max_chunks = 0;
  for (int l = 0; l < nlev; ++l) {
    HLevel* L = h->levels[l];
    const int nn = (int)L->node_ids.size();
    std::vector<LvlNode> ln(nn);
    const int seed_off = (l >= l0 && l - l0 < (int)h->sub.seed_off.size()) ? h->sub.seed_off[l - l0] : 0;
    for (int q = 0; q < nn; ++q) { const HNode& nd = h->nodes[L->node_ids[q]]; ln[q] = {nd.start, nd.half, nd.size, seed_off}; }
    if (!L->nodes_up) { GH_CHECK(upload(L->d_nodes, ln, h->st)); L->nodes_up = true; }
    GH_CHECK(L->d_ranks.ensure(nn * sizeof(int)));
    if (L->top) {                                        // no ACA here: its "rank" is the level's, the staged factors are zero-padded to it
      GH_HIP(hipMemcpyAsync(L->d_ranks.p, &h->sub.R[l], sizeof(int), hipMemcpyHostToDevice, h->st));
      c.al[l].G = 1;
      continue;
    }
    // cluster size: as many workgroups per node as keep the whole grid resident (nodes * G <= 256)
    // and leave every thread `ept` columns (measured at C4 with a switch that went in round 4: 2 -> 12.5 ms,
    // 4 -> 13.1, 8 -> 14.1, 16 -> 16.0: the step is bound by per-thread memory latency, not by the
    // barriers, so more and smaller workgroups win)
    const int ept = 2;
    int G = 1, min_half = INT32_MAX;
    for (int q = 0; q < nn; ++q) min_half = std::min(min_half, ln[q].half);
    while (G * 2 * nn <= 256 && (long)(G * 2) * ACA_THREADS * ept <= min_half) G *= 2;
    c.al[l].G = G;
  }
  return GH_OK;
}

// 0: level l goes through the workgroup kernel; 64 / 128 / 256: every block of the level has at most that many rows and
// columns and the level goes through hodlr_aca_wave_kernel
static int wave_mr(const HodlrCall& c, int l) {
  const gh_hodlr* h = c.h;
  if (!c.sw.wave_aca || h->wave_bad[l] || h->levels[l]->top || c.al[l].G != 1) return 0;
  int mx = 0;
  for (int id : h->levels[l]->node_ids) { const HNode& nd = h->nodes[id]; mx = std::max(mx, std::max(nd.half, nd.size - nd.half)); }
  // (the interpreter's registers beside 128 of mirrors would spill: kernels off the a + b F(r^2) form stop at 128 x 128)
  return mx <= 64 ? 64 : mx <= 128 ? 128 : (mx <= 256 && c.k->fast.ok) ? 256 : 0;
}
static GhBuf& aca_scratch(HodlrCall& c, int l) { return c.concurrent ? (GhBuf&)c.al[l].Tcm : (GhBuf&)c.shared_Tcm; }
// buffers of level l for column capacity rc, counters cleared on stream sx
static int prepare_level(HodlrCall& c, int l, int rc, hipStream_t sx) {
  AcaLevel& a = c.al[l];
  const int nn = (int)c.h->levels[l]->node_ids.size();
  a.rcap = rc;
  GH_CHECK(aca_scratch(c, l).ensure((size_t)c.n * rc * sizeof(double)));
  GH_CHECK(a.idx.ensure((size_t)c.n * sizeof(int)));
  GH_CHECK(a.part.ensure((size_t)nn * a.G * ACA_PSTRIDE * sizeof(double)));
  if (a.sync_cleared) {                                  // (its slice of sync_all was cleared with all the others)
    a.sync_cleared = false;
  } else {
    GH_CHECK(a.sync.ensure((size_t)nn * (sizeof(unsigned) + 2 * sizeof(int)) + 2 * sizeof(int)));
    a.syncp = (char*)a.sync.p;
    GH_HIP(hipMemsetAsync(a.syncp, 0, (size_t)nn * (sizeof(unsigned) + 2 * sizeof(int)) + 2 * sizeof(int), sx));
  }
  return GH_OK;
}
// enqueue the ACA of level l with column capacity rc on stream sx (no synchronisation)
static int enqueue_level(HodlrCall& c, int l, int rc, hipStream_t sx) {
  gh_hodlr* const h = c.h;
  gh_kernel* const k = c.k;
  HLevel* L = h->levels[l];
  AcaLevel& a = c.al[l];
  const int nn = (int)L->node_ids.size();
  GH_CHECK(prepare_level(c, l, rc, sx));
  GhBuf& T = aca_scratch(c, l);
  unsigned* d_bars = (unsigned*)a.syncp;
  int* d_sel = (int*)(d_bars + nn);
  int* d_fail = d_sel + nn;
  if (const int mr = wave_mr(c, l))                      // blocks of <= 256 x 256: a wavefront per node
    return hodlr_launch_aca_wave(h, k, c.ndim, (const LvlNode*)L->d_nodes.p, nn, mr, T.d(), (long)c.n, rc, (int*)L->d_ranks.p, l, d_fail + 1, sx);
  AcaLaunch al{};
  al.x = h->x.d(); al.N = (long)c.n; al.ndim = c.ndim;
  al.nodes = (const LvlNode*)L->d_nodes.p; al.Tcm = T.d(); al.idx = (int*)a.idx.p; al.ranks = (int*)L->d_ranks.p;
  al.bars = d_bars; al.part = a.part.d(); al.sel = d_sel; al.fail = d_fail; al.trunc = d_fail + 1;
  al.nwg = nn * a.G; al.G = a.G; al.level = l; al.rc = rc; al.pstride = ACA_PSTRIDE; al.multi = ACA_MULTI; al.fence = ACA_FENCE;
  al.ones_only = a.G == 1;
  return hodlr_launch_aca(h, k, al, sx);
}
// all levels `cl` as ONE launch of segments (the clustered ones: at most 256 workgroups, al[l].G already balanced)
static int enqueue_fused(HodlrCall& c, const std::vector<int>& cl, int rc, hipStream_t sx, GhBuf& segbuf) {
  gh_hodlr* const h = c.h;
  gh_kernel* const k = c.k;
  std::vector<AcaSeg> segs;
  int wg = 0;
  bool ones_only = true;                                 // (one-workgroup nodes only: the launch carries the LDS mirrors)
  for (int l : cl) ones_only = ones_only && c.al[l].G == 1;
  for (int l : cl) {
    HLevel* L = h->levels[l];
    AcaLevel& a = c.al[l];
    const int nn = (int)L->node_ids.size();
    GH_CHECK(prepare_level(c, l, rc, sx));
    unsigned* d_bars = (unsigned*)a.syncp;
    int* d_sel = (int*)(d_bars + nn);
    int* d_fail = d_sel + nn;
    int* d_dur = nullptr;
    const int* d_order = nullptr;
    if (ones_only && c.sw.lpt) {
      // The nodes of a level differ in cost by 4x (C4, level 8: 205 us on average, ~800 us for the few whose search runs dry
      // first), and a long one dispatched late is the end of phase 1: every node reports how long it took, and the next
      // compute() of the handle launches the level longest first.  Inside an optimiser loop the costs hardly move.
      d_dur = d_fail + 2;
      a.timed = true;
      if ((int)L->aca_dur.size() == nn) {
        std::vector<int> ord(nn);
        for (int q = 0; q < nn; ++q) ord[q] = q;
        std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return L->aca_dur[x] > L->aca_dur[y]; });
        GH_CHECK(upload(L->d_order, ord, sx));
        d_order = (const int*)L->d_order.p;
      }
    }
    segs.push_back({(const LvlNode*)L->d_nodes.p, a.Tcm.d(), (int*)a.idx.p, (int*)L->d_ranks.p, d_bars, a.part.d(), d_sel,
                    d_fail, d_fail + 1, l, a.G, wg, nn * a.G, d_dur, d_order});
    wg += nn * a.G;
  }
  GH_CHECK(upload(segbuf, segs, sx));
  AcaLaunch al{};                                        // (every per-level field null: the segments carry them)
  al.x = h->x.d(); al.N = (long)c.n; al.ndim = c.ndim;
  al.segs = (const AcaSeg*)segbuf.p; al.nseg = (int)segs.size();
  al.nwg = wg; al.G = 1; al.level = 0; al.rc = rc; al.pstride = ACA_PSTRIDE; al.multi = ACA_MULTI; al.fence = ACA_FENCE;
  al.ones_only = ones_only;
  return hodlr_launch_aca(h, k, al, sx);
}
// flags and ranks of level l back to the host (a device-to-host copy into pageable memory holds the
// host until the stream gets there, so these are issued only after EVERY level has been enqueued)
static int fetch_level(HodlrCall& c, int l, hipStream_t sx) {
  HLevel* L = c.h->levels[l];
  AcaLevel& a = c.al[l];
  const int nn = (int)L->node_ids.size();
  int* d_fail = (int*)((unsigned*)a.syncp + nn) + nn;
  L->ranks.resize(nn);
  GH_HIP(hipMemcpyAsync(a.flags, d_fail, 2 * sizeof(int), hipMemcpyDeviceToHost, sx));
  GH_HIP(hipMemcpyAsync(L->ranks.data(), L->d_ranks.p, nn * sizeof(int), hipMemcpyDeviceToHost, sx));
  return GH_OK;
}
// after a synchronisation: validate level l, redo it with more columns while a block is cut short
static int settle_level(HodlrCall& c, int l) {
  gh_hodlr* const h = c.h;
  AcaLevel& a = c.al[l];
  for (;;) {
    if (a.flags[0]) { gh_set_error("HODLR: cluster barrier of the ACA kernel timed out at level %d", l); return GH_ERR_HIP; }
    if (!a.flags[1]) return GH_OK;
    if (a.flags[1] >= 2) {
      // a block of this level asked the wavefront-per-node kernel for more than AW_RW_OF(E) columns: the level again, with the
      // workgroup kernel (same draws, same results), and the handle remembers it for its next compute()
      h->wave_bad[l] = 1;
      GH_CHECK(enqueue_level(c, l, a.rcap, h->st));
      GH_CHECK(fetch_level(c, l, h->st));
      GH_HIP(hipStreamSynchronize(h->st));
      continue;
    }
    // hodlr.h:147 lets the rank grow to min(rows, cols); a cut-short block would be a silently wrong answer
    if (c.user_cap || a.rcap >= RANK_CAP) {
      gh_set_error("HODLR: an off-diagonal block of level %d needs a rank above %d to reach tol = %g (%s); "
                   "the factorisation is not usable", l, a.rcap, h->opts.tol,
                   c.user_cap ? "opts.max_rank" : "the solver's ceiling: loosen tol, raise min_size or use the dense solver");
      return c.user_cap ? GH_ERR_BAD_ARG : GH_ERR_RANK;
    }
    GH_CHECK(enqueue_level(c, l, std::min(2 * a.rcap, RANK_CAP), h->st));
    GH_CHECK(fetch_level(c, l, h->st));
    GH_HIP(hipStreamSynchronize(h->st));
  }
}
static void rank_of_level(gh_hodlr* h, int l) {
  HLevel* L = h->levels[l];
  if (L->top) L->ranks.assign(1, h->sub.R[l]);         // (given: the ACA of the ancestor ran elsewhere)
  L->R = 0;
  for (int r : L->ranks) L->R = std::max(L->R, r);
  L->off = h->Rtot;
  h->Rtot += L->R;
  h->maxR = std::max(h->maxR, L->R);
}
// serial mode only (one scratch shared by the levels): park the level's factors in a compact buffer
static int compact_level(HodlrCall& c, int l) {
  HLevel* L = c.h->levels[l];
  const int nn = (int)L->node_ids.size();
  const int64_t n = c.n;
  rank_of_level(c.h, l);
  if (L->R > 0) {
    c.levelB[l] = std::make_unique<GhPooledBuf>();
    GH_CHECK(c.levelB[l]->ensure((size_t)n * L->R * sizeof(double)));
    GH_HIP(hipMemsetAsync(c.levelB[l]->p, 0, (size_t)n * L->R * sizeof(double), c.h->st));
    hipLaunchKernelGGL(hodlr_compact_kernel, dim3(nn, std::max(8, std::min(512, 2048 / nn))), dim3(256), 0, c.h->st, c.shared_Tcm.d(), (long)n, (const LvlNode*)L->d_nodes.p,
                       (const int*)L->d_ranks.p, L->R, c.levelB[l]->d(), (long)L->R, 0L, (double*)nullptr, 0L, 0L);
    GH_HIP(hipGetLastError());
  }
  return GH_OK;
}
// the levels one at a time through ONE shared scratch (when the levels' scratch would not fit side by side)
static int run_aca_serial(HodlrCall& c) {
  for (int l = 0; l < c.l0; ++l) rank_of_level(c.h, l);
  c.mark("serial ACA starts");
  for (int l = c.l0; l < c.nlev; ++l) {
    GH_CHECK(enqueue_level(c, l, c.rcap0, c.h->st));
    c.mark("  level enqueued");
    GH_CHECK(fetch_level(c, l, c.h->st));
    GH_HIP(hipStreamSynchronize(c.h->st));
    c.mark("  level synchronised");
    GH_CHECK(settle_level(c, l));
    GH_CHECK(compact_level(c, l));
  }
  return GH_OK;
}

// The cooperative launch's budget: the 256 workgroup slots dealt over the clustered levels `cl` so that the per-thread load is as
// even as it gets (start from <= 32 workgroups per level, then keep doubling the cluster of the level whose threads carry most
// columns).  gmax[l]: level l's cluster size before (1: not clustered); fused: the levels of the cooperative launch; single: the
// clusterable levels left to the one-workgroup launch.
static void coop_budget(HodlrCall& c, const std::vector<int>& cl, std::vector<int>& gmax, std::vector<int>& fused, std::vector<int>& single) {
  const gh_hodlr* h = c.h;
  std::vector<AcaLevel>& al = c.al;
  const int wgs = c.sw.coop_wgs;
  std::vector<int> half(c.nlev, 1);
  gmax.assign(c.nlev, 1);
  int total = 0;
  for (int l : cl) {
    const int nn = (int)h->levels[l]->node_ids.size();
    gmax[l] = al[l].G;
    int mh = INT32_MAX;
    for (int id : h->levels[l]->node_ids) mh = std::min(mh, h->nodes[id].half);
    half[l] = mh;
    int G = 1;
    while (G * 2 <= gmax[l] && nn * G * 2 <= wgs / 8) G *= 2;
    al[l].G = G;
    // (round 6: a clusterable level left with one workgroup per node -- level 5 of C4: 32 blocks of 4096 x 4096, 0.54 ms per
    //  node -- stays in the cooperative launch as one-workgroup segments at its end while the launch still fits the chip: in
    //  the one-workgroup launch its nodes found no SIMD with room beside a cooperative workgroup before ~0.5 ms and were the
    //  tail of phase 1, profiles/r06/hodlr_phase1_registers.md)
    if (G > 1 || (c.sw.coop_singles && nn <= wgs / 8)) total += nn * G;       // (reserved: the doubling below stays inside the budget)
  }
  for (;;) {
    int best = -1;
    double load = 0.0;
    for (int l : cl) {
      const int nn = (int)h->levels[l]->node_ids.size();
      if (al[l].G < 2 || al[l].G * 2 > gmax[l] || total + nn * al[l].G > wgs) continue;
      const double ld = (double)half[l] / al[l].G;
      if (ld > load) { load = ld; best = l; }
    }
    if (best < 0) break;
    total += (int)h->levels[best]->node_ids.size() * al[best].G;
    al[best].G *= 2;
  }
  // (the clusters below the root at 1 / coop_lower of that width: see gh_debug_set_hodlr_coop_lower)
  for (size_t q = 1; q < cl.size(); ++q) { int& G = al[cl[q]].G; int d = c.sw.coop_lower; while (d > 1 && G >= 4) { G /= 2; d /= 2; } }
  int used = 0;
  for (int l : cl) if (al[l].G > 1) used += (int)h->levels[l]->node_ids.size() * al[l].G;
  for (int l : cl) {
    const int nn = (int)h->levels[l]->node_ids.size();
    if (al[l].G > 1) fused.push_back(l);
    // (G = 1 segments.  With the clusters below the root at half width there is room for a second such level -- C4: level 6,
    //  64 blocks of 2048 x 2048, which start at 0 instead of waiting ~0.24 ms for a CU: 3.40 -> 3.31 ms)
    else if (c.sw.coop_singles && nn <= wgs / 4 && used + nn <= wgs) { fused.push_back(l); used += nn; }
    else single.push_back(l);
  }
}
// record the next timing event of the side items on sx
static int stamp(gh_hodlr* h, hipStream_t sx) {
  if (h->aca_ev_used == h->aca_ev.size()) { hipEvent_t e; GH_HIP(hipEventCreate(&e)); h->aca_ev.push_back(e); }
  GH_HIP(hipEventRecord(h->aca_ev[h->aca_ev_used++], sx));
  return GH_OK;
}
// two or more clustered levels: the cooperative launch on the solver's stream, everything else of phase 1 beside it
static int enqueue_coop(HodlrCall& c, const std::vector<int>& cl) {
  gh_hodlr* const h = c.h;
  const hipStream_t st = h->st;
  const int nlev = c.nlev;
  std::vector<int> gmax, fused, single;
  coop_budget(c, cl, gmax, fused, single);
  if (h->aca_fused_ev[0] == nullptr) { GH_HIP(hipEventCreate(&h->aca_fused_ev[0])); GH_HIP(hipEventCreate(&h->aca_fused_ev[1])); }
  GH_HIP(hipEventRecord(h->aca_fused_ev[0], st));
  GH_CHECK(enqueue_fused(c, fused, c.rcap0, st, h->d_aca_segs));
  GH_HIP(hipEventRecord(h->aca_fused_ev[1], st));
  h->aca_timed = true;
  // The one-workgroup-per-node levels and the leaf stage are independent of the fused launch and of
  // each other, but HIP multiplexes streams onto 4 hardware queues (3 seen by this library: more
  // streams than that just share a queue and serialise -- measured: a "fourth stream" ran its kernels
  // behind the fused launch).  So: three queues -- the solver's stream (fused launch first) and two
  // side streams -- and the items are dealt longest-first onto the least loaded queue, with the
  // durations MEASURED in the previous compute() of this handle (HIP events; a default guess the
  // first time): ranks, and with them the cost profile, hardly move inside an optimiser loop.
  ensure_side_stream(h, 2);
  if (h->st_c) ensure_side_stream(h, 3);
  std::vector<int> ones = single;
  for (int l = c.l0; l < nlev; ++l) if (gmax[l] == 1) ones.push_back(l);
  // The one-workgroup-per-node levels as ONE launch too (segments in order of decreasing block size: the long
  // workgroups are dispatched first): launched one per queue they were balanced by hand over three queues with last
  // compute()'s durations, and the queue that drew the two slowest levels ended 0.4 ms after the others.  One grid
  // leaves the balancing to the dispatcher: C4 5.36 -> 5.24 ms.  (EVERY level in one grid, clustered segments first, was
  // no better: 5.30.)
  // the deep levels that take the wavefront-per-node kernel: launches of their own, first, on the fourth queue (the
  // process-wide chain stream: high priority) where there is one
  bool wave_on_d = false;
  std::vector<int> keep;
  const hipStream_t sw = h->st_d ? h->st_d : h->st_b;
  for (int l : ones) {
    if (!wave_mr(c, l)) { keep.push_back(l); continue; }
    if (sw == h->st_d && !wave_on_d) { GH_HIP(hipStreamWaitEvent(h->st_d, h->ev_b, 0)); wave_on_d = true; }
    GH_CHECK(enqueue_level(c, l, c.rcap0, sw));
  }
  ones.swap(keep);
  if (wave_on_d) { GH_HIP(hipEventRecord(h->ev_d, h->st_d)); GH_HIP(hipStreamWaitEvent(st, h->ev_d, 0)); }
  if (ones.size() >= 2 && h->st_c) {
    std::sort(ones.begin(), ones.end());
#ifdef ACA_ONES_DEEPEST_FIRST
    std::reverse(ones.begin(), ones.end());
#endif
#ifdef ACA_ONES_LAST_FIRST
    std::rotate(ones.begin(), ones.end() - 1, ones.end());       // deepest level first, then by decreasing block size
#endif
    GH_HIP(hipStreamWaitEvent(h->st_c, h->ev_b, 0));
    if (h->st_d) GH_HIP(hipStreamWaitEvent(h->st_d, h->ev_b, 0));
    // (round 5, measured and left out -- HISTORY.md: the leaf chain first and this launch behind it: +1.5 %; the levels with
    //  blocks of <= 256 rows as a launch of their own with 256 / 128 / 64 threads per workgroup: 0 / +2.4 / +8 %.  The three
    //  pieces of this phase are bound by what they ask of the chip together, not by their order or their shapes.)
    GH_CHECK(enqueue_fused(c, ones, c.rcap0, h->st_b, h->d_aca_segs1));
    GH_CHECK(leaf_stage(c, h->st_c));
    GH_HIP(hipEventRecord(h->ev_c, h->st_c));
    GH_HIP(hipStreamWaitEvent(st, h->ev_c, 0));
    h->aca_timed = false;
    ones.clear();
  }
  struct Item { int level; double cost; };             // level -1: the leaf stage
  std::vector<Item> items;
  const bool have = (int)h->aca_ms.size() == nlev + 2;     // [0..nlev): levels, [nlev]: fused launch, [nlev+1]: leaf stage
  for (int l : ones) items.push_back({l, have && h->aca_ms[l] > 0 ? h->aca_ms[l] : 1.0});
  if (!c.leaves_done) items.push_back({-1, have && h->aca_ms[nlev + 1] > 0 ? h->aca_ms[nlev + 1] : 1.2});
  std::sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.cost > y.cost; });
  hipStream_t qs[4] = {st, h->st_b, h->st_c ? h->st_c : h->st_b, h->st_d ? h->st_d : h->st_b};
  double load[4] = {have && h->aca_ms[nlev] > 0 ? h->aca_ms[nlev] : 1.5, 0.0, h->st_c ? 0.0 : 1e30, h->st_d ? 0.0 : 1e30};
  if (h->st_c) GH_HIP(hipStreamWaitEvent(h->st_c, h->ev_b, 0));
  if (h->st_d) GH_HIP(hipStreamWaitEvent(h->st_d, h->ev_b, 0));
  h->aca_ev_used = 0;
  h->aca_items.clear();
  // (the fused launch was enqueued above, between two stamps on st)
  for (const Item& it : items) {
    int q = 0;
    for (int w = 1; w < 4; ++w) if (load[w] < load[q]) q = w;
    load[q] += it.cost;
    GH_CHECK(stamp(h, qs[q]));
    if (it.level >= 0) GH_CHECK(enqueue_level(c, it.level, c.rcap0, qs[q])); else GH_CHECK(leaf_stage(c, qs[q]));
    GH_CHECK(stamp(h, qs[q]));
    h->aca_items.push_back(it.level);
  }
  if (h->st_c) { GH_HIP(hipEventRecord(h->ev_c, h->st_c)); GH_HIP(hipStreamWaitEvent(st, h->ev_c, 0)); }
  if (h->st_d) { GH_HIP(hipEventRecord(h->ev_d, h->st_d)); GH_HIP(hipStreamWaitEvent(st, h->ev_d, 0)); }
  return GH_OK;
}
#ifdef GH_ACA_TIMES
// per-level node durations of the one-workgroup launches (from the ACA kernel's partials), once, at the third compute()
static void print_aca_times(HodlrCall& c) {
  static int calls = 0;                           // (the third compute(): the durations of the handle's previous one are in use)
  if (++calls != 3) return;
  for (int l = c.l0; l < c.nlev; ++l) {
    if (c.al[l].G != 1) { fprintf(stderr, "[aca] level %d: G = %d\n", l, c.al[l].G); continue; }
    const int nn = (int)c.h->levels[l]->node_ids.size();
    std::vector<double> hp((size_t)nn * ACA_PSTRIDE);
    (void)hipMemcpy(hp.data(), c.al[l].part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost);
    double mx = 0, sum = 0, t0min = 1e300, t1max = 0, ps = 0, rem = 0;
    int who = 0;
    for (int q = 0; q < nn; ++q) {
      const double* e = hp.data() + (size_t)q * ACA_PSTRIDE;
      sum += e[0]; ps += e[3]; rem += e[2];
      if (e[0] > mx) { mx = e[0]; who = q; }
      t0min = std::min(t0min, e[4]); t1max = std::max(t1max, e[4] + e[0]);
    }
    const double* w = hp.data() + (size_t)who * ACA_PSTRIDE;
    fprintf(stderr, "[aca] level %2d: %4d nodes  per-node us mean %8.1f max %8.1f (node %d: rank %d, rows left %d, passes %d)  mean passes %.1f "
            "mean rows left %.1f  first start %.1f .. last end %.1f us (100 MHz clock)\n", l, nn, sum / nn * 0.01, mx * 0.01, who, (int)w[1], (int)w[2], (int)w[3],
            ps / nn, rem / nn, t0min * 0.01, t1max * 0.01);
  }
}
#endif
// every level at once: all of phase 1 enqueued, then ONE synchronisation for the ranks and flags of every level
static int run_aca_concurrent(HodlrCall& c) {
  gh_hodlr* const h = c.h;
  const hipStream_t st = h->st;
  const int nlev = c.nlev, l0 = c.l0;
  std::vector<AcaLevel>& al = c.al;
  // (a memset per level in front of every launch: thirteen ~7 us fill kernels, 100 us before the one-workgroup levels started)
  size_t off = 0;
  std::vector<size_t> slice(nlev, 0);
  for (int l = l0; l < nlev; ++l) {
    if (h->levels[l]->top) continue;
    slice[l] = off;
    off += (size_t)gh_round_up((int64_t)(h->levels[l]->node_ids.size() * (sizeof(unsigned) + 2 * sizeof(int)) + 2 * sizeof(int)), 256);   // bars | sel | fail, trunc | dur
  }
  GH_CHECK(c.sync_all.ensure(std::max<size_t>(off, 256)));
  GH_HIP(hipMemsetAsync(c.sync_all.p, 0, std::max<size_t>(off, 256), st));
  for (int l = l0; l < nlev; ++l) if (!h->levels[l]->top) { al[l].syncp = (char*)c.sync_all.p + slice[l]; al[l].sync_cleared = true; }
  GH_HIP(hipEventRecord(h->ev_b, st));                   // x and the node tables are uploaded
  GH_HIP(hipStreamWaitEvent(h->st_b, h->ev_b, 0));
  std::vector<int> cl;
  for (int l = l0; l < nlev; ++l) if (al[l].G > 1) cl.push_back(l);
  if (cl.size() >= 2) {
    GH_CHECK(enqueue_coop(c, cl));
  } else {
    for (int l = l0; l < nlev; ++l) GH_CHECK(enqueue_level(c, l, c.rcap0, al[l].G > 1 ? st : h->st_b));
    GH_CHECK(leaf_stage(c, h->st_b));
  }
  GH_HIP(hipEventRecord(h->ev_b, h->st_b));
  GH_HIP(hipStreamWaitEvent(st, h->ev_b, 0));
  // one gather launch + one copy into pinned memory for the ranks and the two failure flags of every level
  std::vector<GatherItem> items;
  int tot = 0;
  for (int l = l0; l < nlev; ++l) {
    HLevel* L = h->levels[l];
    const int nn = (int)L->node_ids.size();
    items.push_back({(const int*)L->d_ranks.p, nn, tot}); tot += nn;
    items.push_back({(const int*)((unsigned*)al[l].syncp + nn) + nn, 2 + (al[l].timed ? nn : 0), tot}); tot += 2 + (al[l].timed ? nn : 0);
  }
  // (pinned host memory, read by the kernel in place: the item table needs no copy of its own)
  const size_t need = (size_t)tot + 4 + items.size() * (sizeof(GatherItem) / sizeof(int));
  if (need > h->h_gather_cap) {
    if (h->h_gather) (void)hipHostFree(h->h_gather);
    h->h_gather = nullptr; h->h_gather_cap = 0;
    GH_HIP(hipHostMalloc((void**)&h->h_gather, need * 2 * sizeof(int), hipHostMallocDefault));
    h->h_gather_cap = need * 2;
  }
  GatherItem* const h_items = (GatherItem*)(h->h_gather + ((tot + 3) / 4) * 4);       // (16-byte aligned, behind the results)
  memcpy(h_items, items.data(), items.size() * sizeof(GatherItem));
  GH_CHECK(h->d_gather.ensure((size_t)tot * sizeof(int)));
  hipLaunchKernelGGL(hodlr_gather_kernel, dim3((unsigned)items.size()), dim3(256), 0, st, (const GatherItem*)h_items, (int*)h->d_gather.p);
  GH_HIP(hipGetLastError());
  GH_HIP(hipMemcpyAsync(h->h_gather, h->d_gather.p, (size_t)tot * sizeof(int), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  int at = 0;
  for (int l = l0; l < nlev; ++l) {
    HLevel* L = h->levels[l];
    const int nn = (int)L->node_ids.size();
    L->ranks.assign(h->h_gather + at, h->h_gather + at + nn); at += nn;
    al[l].flags[0] = h->h_gather[at]; al[l].flags[1] = h->h_gather[at + 1]; at += 2;
    if (al[l].timed) { L->aca_dur.assign(h->h_gather + at, h->h_gather + at + nn); at += nn; }
  }
  if (h->aca_timed) {                                 // durations for the next compute()'s schedule
    h->aca_ms.assign(nlev + 2, 0.0);
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->aca_fused_ev[0], h->aca_fused_ev[1]) == hipSuccess) h->aca_ms[nlev] = ms;
    for (size_t q = 0; q < h->aca_items.size() && 2 * q + 1 < h->aca_ev_used; ++q) {
      if (hipEventElapsedTime(&ms, h->aca_ev[2 * q], h->aca_ev[2 * q + 1]) != hipSuccess) { (void)hipGetLastError(); continue; }
      const int lv = h->aca_items[q];
      h->aca_ms[lv >= 0 ? lv : nlev + 1] = ms;
    }
    h->aca_timed = false;
  }
#ifdef GH_ACA_TIMES
  print_aca_times(c);
#endif
  for (int l = 0; l < nlev; ++l) { if (l >= l0) GH_CHECK(settle_level(c, l)); rank_of_level(c.h, l); }
  return GH_OK;
}

// chunk / job tables of level L (cached: they depend on the tree and on (R, off, Rtot) only)
static int level_tables(gh_hodlr* h, HLevel* L, long Rtot) {
  const int R = L->R, nn = (int)L->node_ids.size();
  if (L->tab_R == R && L->tab_off == L->off && L->tab_Rtot == Rtot) { h->max_chunks = std::max(h->max_chunks, L->nchunks); return GH_OK; }
  std::vector<Chunk> chunks;
  std::vector<int> crange(nn * 4);
  std::vector<MMJob> red, upd, updl, smul(nn);
  for (int q = 0; q < nn; ++q) {
    const HNode& nd = h->nodes[L->node_ids[q]];
    for (int half = 0; half < 2; ++half) {
      const int r0 = half == 0 ? nd.start : nd.start + nd.half;
      const int cnt = half == 0 ? nd.half : nd.size - nd.half;
      crange[(q * 2 + half) * 2] = (int)chunks.size();
      for (int s = 0; s < cnt; s += HCH) {
        const int nr = std::min(HCH, cnt - s);
        const int ch = (int)chunks.size();
        chunks.push_back({q, half, r0 + s, nr});
        red.push_back({(long)(r0 + s) * R, r0 + s, ch * R, R, nr});                    // A = V_l rows (level-major block, transposed access)
        upd.push_back({(long)(r0 + s) * Rtot, q * 2 * R + (half == 0 ? 0 : R), r0 + s, nr, R});
        updl.push_back({(long)(r0 + s) * R, q * 2 * R + (half == 0 ? 0 : R), r0 + s, nr, R});      // same against UL
      }
      crange[(q * 2 + half) * 2 + 1] = (int)chunks.size();
    }
    smul[q] = {(long)q * 4 * R * R, q * 2 * R, q * 2 * R, 2 * R, 2 * R};
  }
  L->nchunks = (int)chunks.size();
  L->chunk_geom.clear();
  for (const Chunk& ch : chunks) { L->chunk_geom.push_back(ch.row0); L->chunk_geom.push_back(ch.nrows); }
  h->max_chunks = std::max(h->max_chunks, L->nchunks);
  GH_CHECK(upload(L->d_chunks, chunks, h->st));
  GH_CHECK(upload(L->d_crange, crange, h->st));
  GH_CHECK(upload(L->d_red_jobs, red, h->st));
  GH_CHECK(upload(L->d_upd_jobs, upd, h->st));
  GH_CHECK(upload(L->d_updl_jobs, updl, h->st));
  GH_CHECK(upload(L->d_smul_jobs, smul, h->st));
  L->tab_R = R; L->tab_off = L->off; L->tab_Rtot = Rtot;
  return GH_OK;
}
// ---- UA / VA (n x Rtot) from the ACA scratch, the per-level chunk / job tables, the work arrays of the sweep
static int assemble_factors(HodlrCall& c) {
  gh_hodlr* const h = c.h;
  const hipStream_t st = h->st;
  const int64_t n = c.n;
  const int nlev = c.nlev, l0 = c.l0;
  c.shared_Tcm.release();
  c.mark("ACA done, ranks known");
  const long Rtot = std::max(h->Rtot, 1);
  GH_CHECK(h->UA.ensure((size_t)n * Rtot * sizeof(double)));
  GH_CHECK(h->VA.ensure((size_t)n * Rtot * sizeof(double)));
  // UA / VA are written in full by the compaction when every level's nodes cover all n rows (a complete tree: level l
  // has 2^l internal nodes -- the case of C4); only then can the two memsets (157 MB each at C4) be skipped
  bool complete = true;
  for (int l = l0; l < nlev; ++l) if (h->levels[l]->node_ids.size() != ((size_t)1 << (l - l0))) complete = false;   // (a pseudo-level covers every local row)
  bool fused_compact = nlev <= 24;                     // (CompactSegs)
  for (int l = 0; l < nlev; ++l) if (c.levelB[l]) fused_compact = false;
  // (round 6) the compaction writes the level-major copy only and the leaf product -- the first thing that touches U -- reads that and
  // writes the row-major U itself, where that product is ONE pass of the 128-row-leaf kernel over all columns (LeafSrc)
  c.u_from_v = c.sw.u_from_v && fused_compact && complete && l0 == 0 && nlev <= 24 && h->leaf_pitch == 128 && h->max_leaf <= 128 &&
               h->Rtot > MV_C && h->Rtot <= 128;
  if (!(complete && fused_compact)) {
    GH_HIP(hipMemsetAsync(h->UA.p, 0, (size_t)n * Rtot * sizeof(double), st));
    GH_HIP(hipMemsetAsync(h->VA.p, 0, (size_t)n * Rtot * sizeof(double), st));
  }
  if (fused_compact) {
    std::vector<CompactSeg> segs;
    int b0 = 0;
    for (int l = 0; l < nlev; ++l) {
      HLevel* L = h->levels[l];
      if (L->R == 0) continue;
      const int nn = (int)L->node_ids.size(), ny = std::max(8, std::min(512, 2048 / nn));
      segs.push_back({L->top ? h->sub.T[l] : c.al[l].Tcm.d(), (const LvlNode*)L->d_nodes.p, (const int*)L->d_ranks.p, L->R, ny, (long)L->off, (long)n * L->off,
                      (long)L->R, b0, nn * ny});
      b0 += nn * ny;
    }
    if (b0 > 0) {
      CompactSegs cs;
      cs.n = (int)segs.size();
      for (int q = 0; q < cs.n; ++q) cs.s[q] = segs[q];
      hipLaunchKernelGGL(hodlr_compact_all_kernel, dim3((unsigned)b0), dim3(256), 0, st, cs,
                         (long)n, c.u_from_v ? (double*)nullptr : h->UA.d(), (long)Rtot, h->VA.d());
      GH_HIP(hipGetLastError());
    }
  }
  for (int l = 0; l < nlev; ++l) {
    HLevel* L = h->levels[l];
    if (L->R == 0) continue;
    const int R = L->R, nn = (int)L->node_ids.size();
    if (c.levelB[l]) {
      // (serial mode) scatter the compact level buffer into column block [off, off+R) of UA and VA
      GH_HIP(hipMemcpy2DAsync(h->UA.d() + L->off, Rtot * sizeof(double), c.levelB[l]->p, R * sizeof(double), R * sizeof(double), n, hipMemcpyDeviceToDevice, st));
      GH_HIP(hipMemcpyAsync(h->VA.d() + (long)n * L->off, c.levelB[l]->p, (size_t)n * R * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else if (!fused_compact) {                         // (else done above, all levels in one launch)
      // every rank is known by now: the level's scratch goes straight into its column block (22 strided
      // device copies per compute() before)
      hipLaunchKernelGGL(hodlr_compact_kernel, dim3(nn, std::max(8, std::min(512, 2048 / nn))), dim3(256), 0, st, L->top ? h->sub.T[l] : c.al[l].Tcm.d(), (long)n, (const LvlNode*)L->d_nodes.p,
                         (const int*)L->d_ranks.p, R, h->UA.d(), (long)Rtot, (long)L->off, h->VA.d(), (long)R, (long)n * L->off);
      GH_HIP(hipGetLastError());
    }
    GH_CHECK(L->sinv.ensure((size_t)nn * 4 * R * R * sizeof(double)));
    GH_CHECK(level_tables(h, L, Rtot));
  }
  c.mark("tables enqueued");
  // The ACA scratch (n x 256 doubles per level: 6 GB at C4, 12 GB for a 524288-row sub-tree) goes back to the block
  // cache NOW, not when compute() returns, in a SPLIT tree: the next sub-tree of this device starts while this one waits
  // for the others in its top levels, and found the cache empty -- tens of GB of hipMalloc / hipFree per compute(),
  // stalls of 1.4-2.8 s at N = 2M over four sub-trees on one GPU.  That takes a host synchronisation (another handle may pick the
  // blocks up on a stream of its own), 20 us in the middle of a 3.4-ms step: a handle that owns its whole tree keeps the scratch
  // until the end of compute() instead (HodlrCall).
  if (l0 > 0) {
    GH_HIP(hipStreamSynchronize(st));
    c.mark("U, V assembled");
    for (auto& a : c.al) { a.Tcm.release(); a.idx.release(); a.sync.release(); a.part.release(); }
    c.sync_all.release();
    for (auto& b : c.levelB) b.reset();
  }
  size_t maxnodes = 1;
  for (auto* L : h->levels) maxnodes = std::max(maxnodes, L->node_ids.size() * (size_t)std::max(L->R, 1));
  h->cpass = std::max(CPASS, (h->maxR + 63) / 64 * 64);       // the core build handles a level's R columns in ONE pass
  GH_CHECK(h->P.ensure((size_t)std::max(h->max_chunks, 1) * std::max(h->maxR, 1) * h->cpass * sizeof(double)));
  GH_CHECK(h->Tsum.ensure(maxnodes * 2 * h->cpass * sizeof(double)));
  GH_CHECK(h->Tout.ensure(maxnodes * 2 * h->cpass * sizeof(double)));
  GH_CHECK(h->Y.ensure((size_t)n * h->cpass * sizeof(double)));
  return GH_OK;
}

// ---- factorisation sweep (hodlr.h:75-103, level-batched): leaves into every U, then levels bottom-up
// Level l's core product is in Tout: U[:, 0:off) of the shallower levels -= U_l Tout.  Where the next shallower level with R > 0
// can share that pass over U, it forms that level's chunk products as well (hodlr_updred_kernel) and *red_ready says so.
static int update_shallower(HodlrCall& c, int l, bool* red_ready) {
  gh_hodlr* const h = c.h;
  const HLevel* L = h->levels[l];
  const long Rtot = std::max(h->Rtot, 1);
  const HLevel* nx = nullptr;
  for (int q = l - 1; q >= 0 && !nx; --q) if (h->levels[q]->R > 0) nx = h->levels[q];
  if (hodlr_updred_possible(c.sw.passes, L, nx, L->off, h->cpass)) {
    GH_CHECK(hodlr_launch_updred(h, L, nx, h->UA.d() + L->off, Rtot, h->Tout.d(), h->cpass, h->UA.d(), Rtot, L->off,
                           h->VA.d() + (long)c.n * nx->off, h->P.d(), h->cpass));
    *red_ready = true;
    return GH_OK;
  }
  return hodlr_launch_upd(h, (const MMJob*)L->d_upd_jobs.p, L->nchunks, L->R, h->UA.d() + L->off, Rtot, h->Tout.d(), h->cpass, h->UA.d(), Rtot, L->off);
}
static int factor_sweep(HodlrCall& c) {
  gh_hodlr* const h = c.h;
  const hipStream_t st = h->st;
  const int64_t n = c.n;
  const int nlev = c.nlev, l0 = c.l0;
  const long Rtot = std::max(h->Rtot, 1);
  bool red_ready = false;                            // the chunk products of the next level to be processed are in P already
  if (h->Rtot > 0) {
    const HLevel* deepest = nullptr;
    for (int q = nlev - 1; q >= 0 && !deepest; --q) if (h->levels[q]->R > 0) deepest = h->levels[q];
    LeafSrc ls;
    if (c.u_from_v) {
      ls.VA = h->VA.d(); ls.nlev = nlev;
      for (int q = 0; q < nlev; ++q) { ls.off[q] = h->levels[q]->off; ls.R[q] = h->levels[q]->R; ls.offv[q] = (long)n * h->levels[q]->off; }
    }
    GH_CHECK(hodlr_apply_leaves(h, c.sw.passes, h->UA.d(), Rtot, 0, h->Rtot, deepest, &red_ready, c.u_from_v ? &ls : nullptr));
  }
  bool local_done = (l0 == 0);
  for (int l = nlev - 1; l >= 0; --l) {
    HLevel* L = h->levels[l];
    if (l < l0 && !local_done) {
      // everything below needs the other devices: tell the owner of the split that this one has finished on its own
      c.mark("local sweep enqueued");
      GH_HIP(hipStreamSynchronize(st));
      c.mark("local sweep done");
      local_done = true;
      if (h->sub.local_done) GH_CHECK(h->sub.local_done(h->sub.ctx));
    }
    if (L->R == 0) continue;
    const int R = L->R, nn = (int)L->node_ids.size();
    GhBuf* const tabs[3] = {&L->d_gj_offs, &L->d_gj_sizes, &L->d_gj_sc};
    if (L->top) {
      // The ancestor's core: V^T U over its own columns, each device the rows it holds, completed over the devices below
      // the ancestor; every one of them then inverts the same 2R x 2R matrix and updates its own rows of the shallower U's.
      GH_CHECK(hodlr_launch_red(h, (const MMJob*)L->d_red_jobs.p, L->nchunks, R, h->VA.d() + (long)n * L->off,
                          h->UA.d(), Rtot, L->off, h->P.d(), h->cpass, 0, R));
      GH_CHECK(hodlr_launch_sum(h, L, R));
      GH_CHECK(h->sub.allreduce(h->sub.ctx, l, h->Tsum.d(), 2 * R, R, (long)h->cpass, st));
      GH_CHECK(batched_inverse(h, st, L->sinv.d(), {0L}, {2 * R}, h->ld_all.d() + c.ld_at, tabs, L->gj_R == R, h->Tsum.d(), R));
      L->gj_R = R;
      c.top_ld[l] = c.ld_at;
      c.ld_at += 1;
      GH_CHECK(hodlr_apply_level(h, L, h->UA.d(), Rtot, 0, L->off, h->UA.d(), Rtot));
      continue;
    }
    // S = I + [0, V1^T U1; V0^T U0, 0] with the CURRENT U of this level.  The products V_l^T U that the
    // core needs (columns [off, off + R)) and the ones that applying this level's inverse to the shallower
    // levels' U needs (columns [0, off)) read the same V_l chunks and neighbouring columns of the same U
    // rows: ONE reduce + sum over columns [0, off + R) serves both (two launches fewer per level).
    const int Call = L->off + R;
    const bool merged = Call <= h->cpass;
    // (round 6) levels of many small nodes: sum + core inverse + core product in one launch (hodlr_core_kernel)
    const bool core_fused = c.sw.core_fused && merged && L->off > 0 && nn >= 32 && 2 * R <= 32 && Call <= 128 &&
                            L->nchunks <= 128 * nn;      // (a workgroup adds up ITS node's chunk partials: few chunks per node)
    if (merged) {
      // (red_ready: the deeper level's update pass has already formed this level's chunk products -- hodlr_updred_kernel)
      if (!red_ready)
        GH_CHECK(hodlr_launch_red(h, (const MMJob*)L->d_red_jobs.p, L->nchunks, R, h->VA.d() + (long)n * L->off,
                            h->UA.d(), Rtot, 0, h->P.d(), h->cpass, 0, Call));
      red_ready = false;
    }
    if (core_fused) {
#define GH_CORE_LAUNCH(NM) hipLaunchKernelGGL(hodlr_core_kernel<NM>, dim3(nn), dim3(256), 0, st, h->P.d(), (const int*)L->d_crange.p, R, (long)h->cpass, Call, \
                                            L->off, L->off, L->sinv.d(), h->ld_all.d() + c.ld_at, (int*)h->flags.p, h->Tout.d())
      if (2 * R <= 8) GH_CORE_LAUNCH(8); else if (2 * R <= 16) GH_CORE_LAUNCH(16); else GH_CORE_LAUNCH(32);
#undef GH_CORE_LAUNCH
      GH_HIP(hipGetLastError());
      L->gj_R = -1;                                    // (the separate launch's tables were not refreshed)
      c.ld_at += nn;
      GH_CHECK(update_shallower(c, l, &red_ready));
      continue;
    }
    if (merged) {
      GH_CHECK(hodlr_launch_sum(h, L, Call));
    } else {
      GH_CHECK(hodlr_launch_red(h, (const MMJob*)L->d_red_jobs.p, L->nchunks, R, h->VA.d() + (long)n * L->off,
                          h->UA.d(), Rtot, L->off, h->P.d(), h->cpass, 0, R));
      GH_CHECK(hodlr_launch_sum(h, L, R));
    }
    const double* const core_src = h->Tsum.d() + (merged ? L->off : 0);      // V_l^T U[:, own columns]: the core is built from it inside the inverse
    std::vector<long> offs(nn);
    for (int q = 0; q < nn; ++q) offs[q] = (long)q * 4 * R * R;
    GH_CHECK(batched_inverse(h, st, L->sinv.d(), offs, std::vector<int>(nn, 2 * R), h->ld_all.d() + c.ld_at, tabs, L->gj_R == R, core_src, R));
    L->gj_R = R;
    c.ld_at += nn;
    // apply this level's inverse to the U's of all shallower levels: columns [0, off)
    if (merged && L->off > 0) {
      // (Tsum already holds V_l^T U[:, 0:off]: core product and update only)
      GH_CHECK(hodlr_launch_mm(h, st, (const MMJob*)L->d_smul_jobs.p, nn, 2 * R, L->sinv.d(), 2 * R, 1,
                         h->Tsum.d(), h->cpass, 0, h->Tout.d(), h->cpass, 0, L->off, false));
      GH_CHECK(update_shallower(c, l, &red_ready));
    } else {
      GH_CHECK(hodlr_apply_level(h, L, h->UA.d(), Rtot, 0, L->off, h->UA.d(), Rtot));
    }
  }
  // (the level-major copy of the final U that the WIDE solves multiply from is made when one of them asks for it -- ensure_ul;
  //  the narrow solve of a log-likelihood reads the row-major U: 90 us of every C4 step for a copy nothing read)
  h->ul_valid = false;
  c.mark("sweep enqueued");
  return GH_OK;
}

// ---- every log|det| and the failure flags back in ONE copy, into PINNED host memory (a copy to pageable memory is staged
// and waited for inside the call -- two of them were ~45 us between the last kernel and the return); the sum in a fixed order
static int finish(HodlrCall& c, double* logdet_out) {
  gh_hodlr* const h = c.h;
  const size_t nld = std::max<size_t>(c.n_blocks, 1);
  if (h->pin_doubles < nld + 2) {
    if (h->pin) (void)hipHostFree(h->pin);
    h->pin = nullptr; h->pin_doubles = 0;
    GH_HIP(hipHostMalloc((void**)&h->pin, (nld + 2 + 1024) * sizeof(double), hipHostMallocDefault));
    h->pin_doubles = nld + 2 + 1024;
  }
  double* const ld_host = h->pin;
  int fl[4] = {0, 0, 0, 0};
  GH_HIP(hipMemcpyAsync(ld_host, h->ld_all.p, nld * sizeof(double), hipMemcpyDeviceToHost, h->st));
  GH_HIP(hipMemcpyAsync(ld_host + nld, h->flags.p, 4 * sizeof(int), hipMemcpyDeviceToHost, h->st));
  GH_HIP(hipStreamSynchronize(h->st));
  memcpy(fl, ld_host + nld, 4 * sizeof(int));
  long long leaf_info = 0;
  memcpy(&leaf_info, fl + 2, sizeof(long long));
  if (leaf_info != 0) { gh_set_error("HODLR: a leaf block is not positive definite"); return GH_ERR_NOT_PD; }
  if (fl[0] != 0) { gh_set_error("HODLR: singular block encountered (matrix %d of its batch)", fl[0] - 1); return GH_ERR_NOT_PD; }
  // (a sub-tree handle reports the blocks it owns alone; the ancestors' cores, the same on every device below them,
  //  are handed to the owner of the split separately)
  h->sub.ld_top.assign(c.l0, 0.0);
  for (int l = 0; l < c.l0; ++l) if (c.top_ld[l] != (size_t)-1) { h->sub.ld_top[l] = ld_host[c.top_ld[l]]; ld_host[c.top_ld[l]] = 0.0; }
  double logdet = 0.0;
  for (size_t i = 0; i < c.ld_at; ++i) logdet += ld_host[i];        // leaves first, then the cores bottom-up: fixed order
  h->logdet = logdet;
  h->computed = true;
  if (logdet_out) *logdet_out = logdet;
  return GH_OK;
}

extern "C" int gh_hodlr_compute(gh_hodlr* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                                const double* yerr, double* logdet_out) {
  if (!h || !k || !x || !yerr || n <= 0) { gh_set_error("bad argument to compute"); return GH_ERR_BAD_ARG; }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (n > 0x3fffffffL) { gh_set_error("HODLR: n too large"); return GH_ERR_BAD_ARG; }
  HodlrCall c(h, k, n, ndim);
  GH_CHECK(load_inputs(c, x, yerr));
  GH_CHECK(build_tree(c));
  GH_CHECK(plan_aca(c));
  GH_CHECK(c.concurrent ? run_aca_concurrent(c) : run_aca_serial(c));
  GH_CHECK(assemble_factors(c));
  // ---- leaves (enqueued beside the ACA when the levels run concurrently)
  if (!c.leaves_done) GH_CHECK(leaf_stage(c, h->st));
  c.mark("work arrays, leaf stage enqueued");
  GH_CHECK(factor_sweep(c));
  GH_CHECK(finish(c, logdet_out));
  c.ok = true;                                     // (finish() has synchronised h->st, which waits for every side stream)
  return GH_OK;
}

extern "C" int gh_hodlr_ranks(const gh_hodlr* h, int32_t* ranks_out, int32_t max_out, int32_t* n_out) {
  if (!h || !n_out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  int cnt = 0;
  for (auto* L : h->levels)
    for (int r : L->ranks) { if (ranks_out && cnt < max_out) ranks_out[cnt] = r; ++cnt; }
  *n_out = cnt < max_out ? cnt : max_out;
  return GH_OK;
}
