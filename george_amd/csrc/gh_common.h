// gh_common.h -- shared host-side plumbing for libgeorge_amd.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <functional>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/george_amd.h"
#include "gh_eval.h"

#define GH_TILE 128             // tile edge of every blocked kernel; device matrices are padded to it

void gh_set_error(const char* fmt, ...);

#define GH_HIP(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      gh_set_error("HIP error %d (%s) at %s:%d: %s", (int)e_, hipGetErrorString(e_),   \
                   __FILE__, __LINE__, #expr);                                         \
      return GH_ERR_HIP;                                                               \
    }                                                                                  \
  } while (0)

#define GH_CHECK(expr)                 \
  do {                                 \
    int rc_ = (expr);                  \
    if (rc_ != GH_OK) return rc_;      \
  } while (0)

static inline int64_t gh_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// true when p is device (HBM) memory
bool gh_is_device_ptr(const void* p);

// Cache of released device blocks for TRANSIENT buffers.  hipMalloc / hipFree cost 20-100 us each
// and hipFree synchronises the device; the HODLR compute() makes ~180 short-lived allocations
// (per-level job tables, batched-inverse scratch), 6 of its 28 ms.  Pooled buffers hand their block
// back to the cache instead; a later request takes the smallest cached block that fits (and is not
// more than 4x too large).  Only for buffers whose users all run on ONE stream (a block may be
// reused while the previous user's kernels are still queued -- stream order then protects it).
void* gh_pool_acquire(size_t bytes, size_t* capacity);     // nullptr on allocation failure
void gh_pool_release(void* p, size_t capacity);
void gh_pool_trim();                                       // really free every cached block of the current device
size_t gh_pool_parked_bytes();                             // released blocks parked in the current device's cache

// RAII device buffer
struct GhBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool pooled = false;           // release into / acquire from the block cache above
  ~GhBuf() { release(); }
  void release() {
    if (!p) return;
    if (pooled) gh_pool_release(p, bytes); else (void)hipFree(p);
    p = nullptr; bytes = 0;
  }
  int ensure(size_t nbytes) {
    if (nbytes <= bytes && p) return GH_OK;
    release();
    if (pooled) {
      size_t cap = 0;
      p = gh_pool_acquire(nbytes ? nbytes : 8, &cap);
      if (!p) { gh_set_error("hipMalloc of %zu bytes failed", nbytes); return GH_ERR_NOMEM; }
      bytes = cap;
      return GH_OK;
    }
    hipError_t e = hipMalloc(&p, nbytes ? nbytes : 8);
    if (e != hipSuccess) {                                  // (the block cache may hold tens of GB of released blocks: drop them, once)
      (void)hipGetLastError();
      gh_pool_trim();
      e = hipMalloc(&p, nbytes ? nbytes : 8);
    }
    if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); gh_set_error("hipMalloc of %zu bytes failed: %s", nbytes, hipGetErrorString(e)); return GH_ERR_NOMEM; }
    bytes = nbytes;
    return GH_OK;
  }
  double* d() const { return (double*)p; }
};
struct GhPooledBuf : GhBuf { GhPooledBuf() { pooled = true; } };

// copy `count` doubles from src (host or device) into device memory dst
int gh_to_device(double* dst, const double* src, size_t count, hipStream_t st);
// copy `count` doubles from device src into dst (host or device)
int gh_from_device(double* dst, const double* src, size_t count, hipStream_t st);

// --------------------------------------------------------------- kernel handle
struct gh_kernel {
  std::vector<GhNode> nodes;   // postfix program (host copy)
  int ndim = 0;
  int size = 0;                // full parameter count
  int device = -1;
  GhNode* d_nodes = nullptr;   // device copy (lazily uploaded per device)
  GhFast fast;                 // affine single-leaf form a + b*F(r2), fast.ok != 0 when it exists
  ~gh_kernel() { if (d_nodes) (void)hipFree(d_nodes); }
  int upload();                // ensure d_nodes valid on the current device
};

// raw parameters -> a leaf node's p / m / q (gh_kmat.hip; d.ktype, npar, mtype, nmet set), and the a + b F(r^2) form of a
// program (f->ok == 0 when it has none, or when GEORGE_AMD_NO_FAST_KERNEL is set)
void gh_node_set_params(GhNode& d, const double* params, const double* metric);
void gh_fast_form(const GhNode* nodes, int n_nodes, GhFast* f);

// the buffers of gh_chol_objective_batch / gh_chol_predict_batch / gh_chol_objective_grad_batch (gh_batch.hip), owned by a
// gh_chol handle
struct GhBatchBufs;
GhBatchBufs* gh_batch_new();
size_t gh_batch_bytes(const GhBatchBufs* b);
void gh_batch_free(GhBatchBufs* b);
// gh_batch.hip's view of a handle: sets its device, marks it not computed, returns its main stream and its batch buffers
int gh_chol_batch_begin(gh_chol* s, hipStream_t* st, GhBatchBufs** bufs);

// ----------------------------------------------------------------- launchers
// (all device pointers; sizes need not be tile multiples unless noted)
// out[r*ldo + c] = k(x1[r], x2[c]) for r < n1, c < n2; rows/cols up to (rows_p, cols_p) are
// zero-filled (identity when `sym`).  sym: x1 == x2, evaluate with ordered arguments
// (k(x_min, x_max), mirroring kernel_interface.cpp:62-77), add yerr[r]^2 on the diagonal when
// yerr != NULL; lower_only: build only 128-tiles on/below the diagonal.
int gh_launch_kmat(const gh_kernel* k, const double* x1, int64_t n1, const double* x2, int64_t n2,
                   const double* yerr, double* out, int64_t ldo, int64_t rows_p, int64_t cols_p,
                   int64_t row0, int64_t col0, bool sym, bool lower_only, hipStream_t st);
int gh_launch_kdiag(const gh_kernel* k, const double* x1, const double* x2, int64_t n, double* out, hipStream_t st);
int gh_launch_kgrad(const gh_kernel* k, const uint32_t* which_host, const double* x1, int64_t n1,
                    const double* x2, int64_t n2, bool sym, double* out, hipStream_t st);
int gh_launch_kxgrad(const gh_kernel* k, int which_arg, const double* x1, int64_t n1,
                     const double* x2, int64_t n2, double* out, hipStream_t st);
// grad[p] = sum_{i>=j} w_ij (alpha_i alpha_j - Kinv[i][j]) dK_ij/dtheta_p, w = 1/2 on the diagonal, 1 below
// (== 1/2 sum_ij A_ij dK_ij/dtheta_p, gp.py:437,465-466); diagA[i] = alpha_i^2 - Kinv[i][i].
int gh_launch_kgrad_reduce(const gh_kernel* k, const uint32_t* which_host, const double* x, int64_t n,
                           const double* alpha, const double* kinv, int64_t ld, double* grad_dev /* size */,
                           double* diagA /* n or NULL */, GhBuf& scratch, hipStream_t st);
// the leave-one-out form (gh_chol_loo): grad[p] = sum_{i>=j} w_ij B_ij dK_ij/dtheta_p, B_ij = 1/2 (alpha_i beta_j + beta_i alpha_j) - M[i][j],
// w = 1 on the diagonal, 2 below (== sum_ij B_ij dK_ij/dtheta_p); diagB[i] = B_ii.  alpha_beta: alpha, and beta `ld` doubles
// behind it.  Same tiles, same fixed-order sums.
int gh_launch_kgrad_reduce_loo(const gh_kernel* k, const uint32_t* which_host, const double* x, int64_t n,
                               const double* alpha_beta, const double* m, int64_t ld, double* grad_dev /* size */,
                               double* diagB /* n or NULL */, GhBuf& scratch, hipStream_t st);

// grad_dev[p] = sum over the nblk rows of partial (nblk x P) in a fixed-order tree: bitwise reproducible (the second stage of
// gh_launch_kgrad_reduce, and of the strip form in gh_hodlr_predict.hip)
int gh_launch_kgrad_final(const double* partial, int64_t nblk, int P, double* grad_dev, hipStream_t st);

// Input derivatives of the prediction (gh_predgrad.hip): dmu[c][d] = sum_i G_cid alpha_i and, when dvar != NULL,
// dvar[c][d] = D_cd - 2 sum_i G_cid W[i * ldw + c], with G the x1-gradient of k at (xs_c, x_i) and D the sum of its x1- and
// x2-gradient at (xs_c, xs_c); G is evaluated and reduced in one kernel and never stored.  Rows i >= n and columns c >= m of
// W are not read.  partial: gh_predgrad_work_doubles(n, m, ndim, dvar != NULL) doubles.  Fixed-order sums, no atomics.
size_t gh_predgrad_work_doubles(int64_t n, int64_t m, int ndim, bool want_var);
int gh_launch_predgrad(const gh_kernel* k, const double* x, int64_t n, const double* xs, int64_t m, const double* alpha,
                       const double* W /* or NULL */, int64_t ldw, double* dmu /* m*ndim */, double* dvar /* m*ndim or NULL */,
                       double* partial, hipStream_t st);
// The weighted input-gradient reduction on the same tile: out[c][d] = (add ? out[c][d] : 0) + scale * sum_i Wt[i * ld + c] G_cid,
// G the x1-gradient of k at (t_c, x_i), for nt points t and nx points x.  Rows i >= nx and columns c >= nt of Wt are neither
// evaluated nor read.  partial: gh_wxgrad_work_doubles(nx, nt, ndim) doubles.  Fixed-order sums, no atomics.
size_t gh_wxgrad_work_doubles(int64_t nx, int64_t nt, int ndim);
int gh_launch_wxgrad(const gh_kernel* k, const double* t, int64_t nt, const double* x, int64_t nx, const double* Wt, int64_t ld,
                     double scale, bool add, double* out /* nt*ndim */, double* partial, hipStream_t st);

// The pieces of gh_chol_fisher (gh_fisher.hip).  A "plane" is a dense np x np matrix of pitch np, np a multiple of 128.
#define GH_FISHER_GROUP 4                   // planes per side of one contraction launch (4 x 4 pairs from registers)
#define GH_FISHER_MAX_DIAG 64               // diagonal parameters of one call
struct GhFisherSel { int n; short idx[GH_MAX_GRAD]; };                          // kernel parameters to store, plane s = idx[s]
struct GhFisherMap { int q, ptot; short out[GH_MAX_GRAD + GH_FISHER_MAX_DIAG]; };   // active plane -> row / column of the result
struct GhFisherPairs {
  const double* a[GH_FISHER_GROUP]; const double* b[GH_FISHER_GROUP];
  int na, nb, same;                         // same: the b side IS the a side (b is not read); pairs i <= j only
  int col[GH_FISHER_GROUP * GH_FISHER_GROUP];   // column of partial for the pair (a[i], b[j]), -1: not wanted
  long ld, ncols;
  double* partial;                          // (number of lower 128-tiles) x ncols
};
// column of the pair a <= b among q active planes (upper triangle by rows)
static inline __host__ __device__ int gh_fisher_pair(int a, int b, int q) { return a * q - a * (a - 1) / 2 + (b - a); }
// planes[s] (s < sel.n) = dK/dtheta_{sel.idx[s]} over the n points x, zero in rows and columns >= n
int gh_launch_fisher_planes(const gh_kernel* k, const GhFisherSel& sel, const double* x, int64_t n, int64_t np, double* planes,
                            hipStream_t st);
// out = linv diag(d): d has np entries, zero from n on
int gh_launch_fisher_scale(const double* linv, int64_t np, const double* d, double* out, hipStream_t st);
// partial[tile][pair(a_idx[i], b_idx[j])] = the weighted lower-triangle sum of a[i] .* b[j] over the tile, for every i, j
// (b == nullptr: the set a with itself, pairs i <= j), in launches of GH_FISHER_GROUP x GH_FISHER_GROUP pairs.  a_idx / b_idx:
// the planes' indices among the q_active active ones (host arrays).
int gh_launch_fisher_pairs(const double* const* a, const int* a_idx, int na, const double* const* b, const int* b_idx, int nb,
                           int q_active, int64_t np, double* partial, hipStream_t st);
// F (ptot x ptot, zeroed by the caller) <- the pair sums, mirrored
int gh_launch_fisher_mirror(const double* pairsum, const GhFisherMap& m, double* F, hipStream_t st);

// The pieces of gh_chol_loo and gh_chol_lgo (gh_cv.hip).  All pointers are device memory; np is a multiple of 128.
// c[i] = sum_k Linv[k][i]^2, the diagonal of K^-1 from L^-1 (lower, row-major): nchunks row chunks in part (nchunks * np doubles),
// added in index order
int gh_launch_loo_colsumsq(const double* Linv, int64_t np, int64_t nchunks, double* part, double* c, hipStream_t st);
// resid, var, lpd, sw = sqrt(w) and u (a second copy of resid, or NULL) per point from alpha and c_i = c[i * cstride]; zeros in rows >= n
int gh_launch_loo_point(const double* alpha, const double* c, int64_t cstride, int64_t n, int64_t np, double* resid, double* u,
                        double* var, double* lpd, double* sw, hipStream_t st);
// S (np x np, full) = W diag(sw) from the lower triangle of the symmetric W
int gh_launch_loo_mirror_scale(const double* W, int64_t np, const double* sw, double* S, hipStream_t st);
// Leave-group-out: a slot is GH_LGO_SLOT consecutive entries of the tables: whole groups, in group-sorted ("permuted") order, then
// padding.
#define GH_LGO_SLOT 128
struct GhLgoSlots {
  const int* idx;            // (nslots * 128) the point at a slot position, -1: padding
  const int* grp;            // (nslots * 128) its group, -1: padding
  const int* minj;           // (nslots) the slot's smallest point index
  const int* pos0;           // (nslots) the permuted position of the slot's first entry
  const long long* start;    // (ngroups + 1) the groups' offsets in permuted order
  const long long* covoff;   // (ngroups + 1) ... and in the packed covariance blocks: sum of m_g^2 before the group
  int nslots;
};
// row chunks of the Gram step (their partial sums are added in index order); part holds chunks * nslots * 128 * 128 doubles
int gh_lgo_gram_chunks(int64_t n, int nslots, int64_t* rows_per);
// Cs[slot] = the slot's block-diagonal, identity-padded matrix of K^-1 entries: from L^-1 (np x np, lower; rows >= n are not
// read) as the Gram matrix of its gathered columns, or gathered from the lower triangle of K^-1
int gh_launch_lgo_gram(const double* Linv, int64_t np, int64_t n, const GhLgoSlots& t, double* part, double* Cs, hipStream_t st);
int gh_launch_lgo_gather(const double* Kinv, int64_t np, const GhLgoSlots& t, double* Cs, hipStream_t st);
// from R = chol(Cs[slot]) and Rinv = R^-1 (gh_launch_potf2_batched): resid, var, u_pt (or NULL) by point, lpd by group, and when
// not NULL cov (packed group blocks) and Ws[slot] = 1/2 (Cs^-1 + u u^T) inside the groups, the identity elsewhere
int gh_launch_lgo_slots(const double* R, const double* Rinv, const GhLgoSlots& t, const double* alpha, double* resid, double* var,
                        double* u_pt, double* lpd, double* cov, double* Ws, hipStream_t st);
// S (np x np) = K^-1[:, J] blockdiag(Tm) from the lower triangle of K^-1: n columns in permuted order, zero from column n and row n on
int gh_launch_lgo_block_scale(const double* Kinv, int64_t np, int64_t n, const GhLgoSlots& t, const double* Tm, double* S,
                              hipStream_t st);

// gh_potf2.hip: batched 128x128 Cholesky + inverse of the factor (block b at A + b*stride_a: the factor in place, zeros above the
// diagonal; its inverse at dinv + b*stride_d, pitch 128).  A block that is not positive definite sets *info; the blocks after it stop.
int gh_launch_potf2_batched(double* A, int64_t lda, int64_t stride_a, double* dinv, int64_t stride_d, long long* info,
                            int nbatch, hipStream_t st);

// fp64 GEMM family on the MFMA pipe: C = beta*C + alpha * op(A) * op(B)^T-ish.  See gh_gemm.hip.
struct GhGemm {
  double* C; int64_t ldc;
  const double* A; int64_t lda;   // a_km: A(m,k) at A[m*lda + k];  else at A[k*lda + m]
  const double* B; int64_t ldb;   // b_km: B(n,k) at B[n*ldb + k];  else at B[k*ldb + n]
  int64_t M, N, K;                // M, N multiples of 128; K multiple of 16
  double alpha, beta;
  bool a_km, b_km;
  bool lower;                     // square C: only tiles with tile_row >= tile_col
  bool klo_max;                   // k starts at max(row0, col0) of the tile (operands lower-triangular in k)
  bool khi_col;                   // k ends at col0 + 128            (B lower-triangular: B(n,k) = 0 for k > n)
  bool khi_row;                   // k ends at row0 + 128            (A lower-triangular: A(m,k) = 0 for k > m)
  bool small_lds;                 // keep to <= 32 KiB of LDS per workgroup: the launch runs beside a SYRK that owns every CU
  // "staircase" C (gh_dev_gemm_nt_stair): M = stair_n * stair_rows; row group g (stair_rows rows) takes columns [0, stair_cols[g]),
  // non-decreasing in g; N = the widest group.  One launch for all groups; stair_n == 0: a plain rectangle / trapezoid.
  int stair_n = 0;
  int64_t stair_rows = 0;
  const int64_t* stair_cols = nullptr;       // host array
};
#define GH_GEMM_STAIR_MAX 128
int gh_launch_gemm(const GhGemm& g, hipStream_t st);

// What the solvers' predict calls share (gh_predict.hip).
// m test points of ndim coordinates on the device: *xs_dev is xs where that is device memory, else a copy that `own` owns
int gh_stage_points(const double* xs, int64_t m, int ndim, GhBuf& own, hipStream_t st, const double** xs_dev);
// rows x cols doubles between row-pitched arrays (pitches in doubles) of which the caller's -- src when from_caller, else dst --
// may be host or device memory
int gh_copy_rows(double* dst, int64_t ldd, const double* src, int64_t lds, int64_t cols, int64_t rows, bool from_caller, hipStream_t st);
// Column reduction over row-major operands of row pitch ld, in nchunks chunks of rows_per rows (partials: nchunks x ldp each):
//   mu[j] = sum_i A[i][j] z[i],   var[j] = var[j] - sum_i P[i][j] Q[i][j]      for j < cols, i < nrows
// P == nullptr: the mean only; else P is A or Q (an operand is loaded once per row).  var may be nullptr with P set (the second
// moment then stays in pvar).  Rows ascending inside a chunk, chunks in ascending order: the same bits whatever `threads` (the
// workgroup size, 64 .. 256) and whatever the other columns hold.
int gh_launch_colreduce(const double* A, const double* z, const double* P, const double* Q, int64_t ld, int64_t nrows, int64_t rows_per,
                        int64_t nchunks, int64_t cols, double* pmu, double* pvar, int64_t ldp, double* mu, double* var, int threads,
                        hipStream_t st);
// predict over column strips for a solver without buffers of its own: mu = Kx^T alpha and, with S = make_second(Kx) and
// F = first_second ? Kx : S, var = diag K(xs, xs) - colsum(F .* S) or cov = K(xs, xs) - F^T S, where Kx = K(x, xs) is built
// strip_cols columns at a time (with cov: whole, with the padding the product needs).  make_second gets a strip sK (np rows of
// pitch ld, cw columns in use, strip_bytes in all) and fills sSecond, of the same shape, on st.  x, alpha, xs_dev: device
// memory; mu, var, cov: the caller's, host or device.  Synchronises st.
typedef std::function<int(const double* sK, double* sSecond, int64_t ld, int64_t np, int cw, size_t strip_bytes)> GhMakeSecond;
int gh_predict_strips(gh_kernel* k, const double* x, int64_t n, int ndim, const double* alpha, const double* xs_dev, int64_t m,
                      int64_t strip_cols, int64_t red_rows, int64_t red_chunks, double* mu, double* var, double* cov, hipStream_t st,
                      bool first_second, const GhMakeSecond& make_second);
// Diagonally pivoted Cholesky with rank truncation, batched (gh_pstrf.hip; the definition is at the top of that file).
// All pointers are device memory.  The launcher enqueues on st; for m > 512 it also synchronises st once per 128 pivots.
struct GhPstrf {
  double* A; int64_t lda, stride_a;       // nbatch symmetric m x m matrices; destroyed
  int64_t m, nbatch;
  double tol; const double* tol_dev;      // stop threshold; tol_dev (nbatch) replaces tol when not null; < 0: m eps max(d_0, 0)
  double* L; int64_t ldl, stride_l;       // the factors; rows_l x cols_l (>= m each) of every member are zeroed first
  int64_t rows_l, cols_l;
  long long* piv; long long* rank;        // (nbatch, m) and (nbatch)
  double* resid;                          // (nbatch) largest remaining diagonal entry, or nullptr
  void* work; size_t work_bytes;          // >= gh_pstrf_work_bytes(m, nbatch)
};
size_t gh_pstrf_work_bytes(int64_t m, int64_t nbatch);
int gh_launch_pstrf(const GhPstrf& p, hipStream_t st);
// draws[b] (nz, m) = mu[b] + z[b] L_b^T with L_b the pivoted factor of cov[b] (gh_pstrf.hip): the tail of every sampling
// entry point.  cov, mu (nbatch, m; or nullptr: zero mean), tol_dev and work are device memory; z (nbatch, nz, m), draws
// (nbatch, nz, m), fac (nbatch, m, m; or nullptr) and rank (nbatch, int64) may be host or device memory.  Copies to host
// memory are enqueued: the caller synchronises st.
struct GhSample {
  double* cov; int64_t lda, stride;       // destroyed
  int64_t m, nbatch;
  double tol; const double* tol_dev;
  const double* mu;
  const double* z; int64_t nz;
  double* draws; double* fac; int64_t* rank;
  void* work; size_t work_bytes;          // >= gh_sample_work_bytes(m, nz, nbatch)
};
size_t gh_sample_work_bytes(int64_t m, int64_t nz, int64_t nbatch);
int gh_sample_enqueue(const GhSample& q, hipStream_t st);
// tol_dev[0] = m eps max(max_i diag[i], 0)
int gh_launch_prior_tol(const double* diag, int64_t m, double* tol_dev, hipStream_t st);
// Process-wide streams of a device, shared by every solver handle (gh_chol.hip): q[0] main (blocking,
// normal priority), q[1..3] non-blocking high-priority.  nullptr where creation failed.  Never destroyed.
// Why shared: HIP maps streams onto a few hardware queues; every further handle with streams of its
// own moved the others' onto different queues and a dense compute() at N <= 16384 ran 20-40 % slower
// with a second handle (or two application streams) alive (scripts/dev/queue_pattern.py) -- and a
// CU-masked stream takes ~1 s to create.  (Per-handle streams were an environment switch until round 4.)
bool gh_shared_streams(int device, hipStream_t q[4]);
// Once per device and process, BEFORE the library creates its first stream there: one empty kernel on the null stream
// and a device synchronisation.  Measured (scripts/dev/no_torch_step.py, stream_order_probe.py): when this library's
// streams are the first thing a process creates on the device -- any george user who does not import torch first -- the
// panel chain of every mid-size factorisation runs at half speed (N = 8192: 13.0 instead of 7.0 ms per
// compute()+log_likelihood(), N = 4096 4.5 instead of 2.7, N = 16384 40 instead of 30); once the null stream has had a
// launch first (what `torch.zeros(1, device="cuda")` happens to do) it does not.  The pairwise overlap of the streams
// is the same in both cases (gh_debug_stream_overlap), so it is not queue sharing; which hardware queue the runtime
// hands out first is not visible from here.  GEORGE_AMD_NO_NULL_PRIME=1 skips it (A/B).
void gh_prime_device(int device);
// measured when the process-wide streams of `device` were made: does the main stream share a dispatcher with the chain,
// rows-below or near stream?  (gh_chol.hip, factor_lookahead_deep: where a look-ahead factorisation is joined)
bool gh_shared_main_crowded(int device);
// do one-workgroup kernels of one stream complete while a grid far larger than the chip runs on the other, both ways round?
// (streams of the current device; ~8 ms)
bool gh_streams_dispatch_independently(hipStream_t a, hipStream_t b);
hipStream_t gh_shared_masked_stream(int device, int reserve_cus);
bool gh_use_mfma();               // false when GEORGE_AMD_NO_MFMA=1 (VALU validation path)

