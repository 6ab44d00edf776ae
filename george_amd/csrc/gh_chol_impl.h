// gh_chol_impl.h -- what the three units of the dense solver share (host side, private to them):
//   gh_chol.hip         the factorisation: handle, streams, tile operations, panel schedules, compute
//   gh_chol_solve.hip   work on a computed factor: sweeps, solve .. fisher, objective, and the cross-validation driver (loo,
//                       loo_objective, lgo; its kernels: gh_cv.hip).  predict's column reduction, the staging of test points and
//                       the pitched copy to the caller are shared with the other solvers: gh_predict.hip (gh_common.h)
//   gh_chol_update.hip  moving and editing a factor: export / import, append / truncate / set_yerr, remove
// A kernel is launched only from the unit that defines it; what another unit needs of it is a launcher declared here.
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"
#include "gh_chol_plan.h"

#define T 128                 // tile edge
#define LP 129                // LDS row pitch of the potf2 tile (odd -> conflict-free columns)
#define CHAIN_THREADS 512     // workgroup size of the chained sweeps

struct EvPair { hipEvent_t a, b; };

struct gh_chol {
  gh_chol_opts opts;
  hipStream_t st = nullptr;
  hipStream_t st2 = nullptr;             // high-priority panel stream (look-ahead)
  hipStream_t st3 = nullptr;             // second panel stream: rows-below TRSM beside the potf2 chain
  bool shared_streams = false;           // st, st2, st3, st4, st_mask belong to the process (gh_shared_streams): not destroyed here
  hipStream_t st4 = nullptr;             // third panel stream: in-panel rows >= j+2 (everything off the potf2 chain)
  hipEvent_t ev_diag[32] = {};             // one per 128-column step of a panel (panels of up to 4096 columns)
  hipEvent_t ev_aux = nullptr, ev_aux2 = nullptr;
  std::vector<hipEvent_t> ev_p, ev_w, ev_nf;   // deep look-ahead: panel j factored / W(j) done / U(j, j+2) done
  GhCholPlan plan;                         // two-level driver: the launch list (rebuilt only when Np, the panel starts or the group maximum change)
  std::vector<hipEvent_t> ev_plan;         // ... and its events, owned by index in the list
  hipStream_t st_mask = nullptr;         // main-stream stand-in that leaves CUs to the panel chain (small N)
  hipStream_t tail = nullptr;            // where the last factor() ended: the stream on which its results are complete in stream order
  int mask_reserved = -1;                // CUs st_mask leaves out (-1: not created yet, 0: creation failed)
  hipEvent_t ev_xfer = nullptr;
  hipEvent_t ev_sync[3] = {nullptr, nullptr, nullptr};
  int64_t n = 0, np = 0;
  int ndim = 0;
  bool have_yerr = false;                // yerr holds the n error bars of compute() / append() (import_factor brings none: gh_chol_set_yerr)
  hipEvent_t ev_lay[2] = {nullptr, nullptr};   // profile: the relayout of the last append()
  bool computed = false;
  int64_t info = 0;
  double logdet = 0.0;
  GhBuf A, dinv, x, yerr, v0, v1, v2, scal, rhs, work, work2, scratch, chain;
  GhBuf A_spare;                         // the buffer the factor left when append / truncate last moved it: where the next move goes (freed by trim)
  GhBuf samp;                            // gh_chol_sample_conditional: prior diagonal, threshold and the factor / draw work arrays (freed by trim)
  GhBuf fish;                            // gh_chol_fisher's planes (freed by trim)
  GhBuf lgo;                             // gh_chol_lgo's slot matrices, their inverses, partial sums and tables (freed by trim)
  GhBuf lv;                              // gh_chol_loo's N-vectors: resid, var, lpd, sqrt(w), c, alpha, v (7 Np doubles)
  long long* d_info = nullptr;           // = (long long*)(scal + 2): the failure word lives beside the scalars (set in compute_enqueue)
  bool build_on_chain = false;           // this compute(): inputs + kernel-matrix build were enqueued on the chain stream (st2)
  GhBatchBufs* batch = nullptr;          // gh_chol_objective_batch's buffers (gh_batch.hip), grown once and re-used
  gh_chol_profile prof;
  std::vector<EvPair> ev_pool;
  size_t ev_used = 0;
  std::vector<size_t> ev_trailing, ev_panel, ev_update;   // ev_update: EVERY trailing-update launch (wide SYRKs and block-column GEMMs)
  std::vector<double> ev_update_flops;                    // algorithmic flops of each ev_update launch
  std::vector<double> upd_intervals;                      // last compute(): (start ms, end ms, flops) per trailing-update launch
  // returns an index into ev_pool (the vector may grow, so never keep pointers), or -1
  long next_ev() {
    if (ev_used == ev_pool.size()) {
      EvPair p;
      if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return -1;
      ev_pool.push_back(p);
    }
    return (long)ev_used++;
  }
  ~gh_chol() {
    for (auto& p : ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto& e : ev_sync) if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_lay) if (e) (void)hipEventDestroy(e);
    if (ev_xfer) (void)hipEventDestroy(ev_xfer);
    if (ev_aux) (void)hipEventDestroy(ev_aux);
    if (ev_aux2) (void)hipEventDestroy(ev_aux2);
    for (auto* v : {&ev_p, &ev_w, &ev_nf, &ev_plan}) for (auto e : *v) (void)hipEventDestroy(e);
    for (auto& e : ev_diag) if (e) (void)hipEventDestroy(e);
    if (st4 && !shared_streams) (void)hipStreamDestroy(st4);
    if (st3 && !shared_streams) (void)hipStreamDestroy(st3);
    if (st_mask && !shared_streams) (void)hipStreamDestroy(st_mask);
    if (st2 && !shared_streams) (void)hipStreamDestroy(st2);
    if (st && !shared_streams) (void)hipStreamDestroy(st);
    gh_batch_free(batch);
  }
};

// ---- the flag words of the chained sweeps, s->chain: [0, nt] forward, [nt + 1, 2 nt + 1] backward (nt = Np / 128 block rows), the
// time-out word last in each set (the words before it are no longer used: the flag-per-block-row kernels are retired).  The ONLY
// place that knows the layout.  gh_chol_append's own sweeps report into word 0.
static inline int chain_ensure(gh_chol* s, int64_t nt) { return s->chain.ensure((size_t)(2 * nt + 2) * sizeof(unsigned)); }
static inline unsigned* fwd_flags(const gh_chol* s) { return (unsigned*)s->chain.p; }
static inline unsigned* bwd_flags(const gh_chol* s) { return (unsigned*)s->chain.p + (s->np / T + 1); }
static inline int* fwd_fail(const gh_chol* s) { return (int*)(fwd_flags(s) + s->np / T); }
static inline int* bwd_fail(const gh_chol* s) { return (int*)(bwd_flags(s) + s->np / T); }
static inline int* append_fail(const gh_chol* s) { return (int*)s->chain.p; }

// ---- the scalars, s->scal: [0] log-det, [1] quadratic form / sum, [2] the failure word's bits, [3] a chained sweep's time-out flag
static inline int read_scalars(const gh_chol* s, double* host, int count, hipStream_t st) {
  GH_HIP(hipMemcpyAsync(host, s->scal.d(), (size_t)count * sizeof(double), hipMemcpyDeviceToHost, st));
  return GH_OK;
}
static inline long long info_from_bits(double word) { long long info = 0; memcpy(&info, &word, sizeof(long long)); return info; }

// the fields every product sets; lower / klo_max / khi_* / small_lds are the call site's
static inline GhGemm gemm_desc(double* C, int64_t ldc, const double* A, int64_t lda, bool a_km, const double* B, int64_t ldb, bool b_km,
                               int64_t M, int64_t N, int64_t K, double alpha, double beta) {
  GhGemm g{};
  g.C = C; g.ldc = ldc; g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
  g.alpha = alpha; g.beta = beta; g.a_km = a_km; g.b_km = b_km;
  return g;
}

// ---- gh_chol.hip
int gh_chol_set_device(gh_chol* s);
int gh_chol_need_computed(gh_chol* s);                  // null handle, not computed, or the device cannot be set
// C = alpha A B^T + beta C on k-major operands, with the factorisation's LDS choice (t_gemm_small_lds)
int gh_gemm_nt(hipStream_t st, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
               int64_t M, int64_t N, int64_t K, double alpha, double beta, bool lower);
// in-place lower Cholesky of the n x n block at A (n multiple of 128) + diagonal-block inverses
int gh_chol_potrf_block(hipStream_t st, double* A, int64_t ld, int64_t n, double* dinv, long long* d_info, long long base);
// Everything of compute() up to and including the log-det launch, enqueued without a host synchronisation (it ends on s->tail);
// gh_chol_compute_finish() takes the scalars read back after that stream has been synchronised.
struct ComputeCtx { long e_all = -1, e_build = -1; };
int gh_chol_compute_enqueue(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr, ComputeCtx& c);
int gh_chol_compute_finish(gh_chol* s, const ComputeCtx& c, double ld_host, long long info_host, double* logdet_out);

// ---- gh_potf2.hip: MFMA-blocked 128x128 Cholesky + inverse
int gh_launch_potf2_mfma(double* A, int64_t lda, double* dinv, long long* info, long long base, hipStream_t st);

// ---- gh_chol_solve.hip
// out[0] (+)= 2 * sum_i log(A[i][i]); part: RED_SLICES doubles.  accumulate: one workgroup, out[0] += (the tile ABI's form)
int gh_launch_logdet(const double* A, long lda, long n, double* out, double* part, hipStream_t st);
int gh_launch_logdet_accum(const double* A, long lda, long n, double* out, hipStream_t st);
// Linv (np x np) <- L^-1 for a factor L of pitch np (np a multiple of 128) with the inverses dinv of its diagonal blocks, as
// gh_chol_potrf_block leaves them: forward substitution on the identity in GEMMs, no handle (gh_chol's own L^-1, and gh_inducing.hip)
int gh_chol_linv(hipStream_t st, const double* L, const double* dinv, int64_t np, double* Linv);
// z = L^-1 w / x = L^-T w as one chained launch; flags[nt] = the time-out flag (cleared here).  w is read only and must not be
// the output (which is pre-filled with the sentinel).
int gh_launch_trsv_fwd_chain(const double* L, long ld, const double* dinv, int64_t nt, const double* w, double* z, unsigned* flags, hipStream_t st);
int gh_launch_trsv_bwd_chain(const double* L, long ld, const double* dinv, int64_t nt, const double* w, double* x, unsigned* flags, hipStream_t st);
// gh_chol_append: m right-hand sides (rows of Y, ldy apart) against the nt0 leading tiles of L, into rows of Z (ldz apart, pre-filled
// with the sentinel by the caller); multi: four and two at a time while they last.  *fail is not cleared here.
int gh_launch_trsv_fwd_chain_rows(const double* L, long ld, const double* dinv, int64_t nt0, const double* Y, long ldy, double* Z, long ldz,
                                  int64_t m, bool multi, int* fail, hipStream_t st);
// GH_OK when neither sweep gave up, else the error.  who == nullptr: a plain solve, which names the sweep.
int gh_chain_timeout(const char* who, bool forward_failed, bool backward_failed);
