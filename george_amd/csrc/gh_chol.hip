// gh_chol.hip -- dense blocked Cholesky solver on one MI355X.
//
// Replaces BasicSolver (reference src/george/solvers/basic.py:51-121) and the
// SciPy/LAPACK dpotrf/dpotrs behind it.  The covariance matrix is built on the
// device (gh_kmat.hip), lives in HBM as one row-major Np x Np array (Np = N
// rounded up to 128, identity-padded) of which only the LOWER triangle is ever
// touched (K = L L^T; the reference's upper factor U is L^T), and is factorised
// in place:
//
//   for each outer panel of NB columns:
//     for each 128-column step of the panel:
//        potf2_inv   : 128x128 diagonal block -> L_jj and L_jj^-1 (one workgroup, all in LDS)
//        trsm (gemm) : rows below <- rows * L_jj^-T            (MFMA, in place)
//        update(gemm): remaining panel columns -= ...          (MFMA)
//     trailing SYRK   : A22 -= L21 L21^T, K = NB, lower tiles  (MFMA; >95 % of the flops)
//
// This unit is the factorisation: the handle, the process-wide streams, the tile operations, the panel schedules and
// compute().  What is done with a computed factor is in gh_chol_solve.hip, what moves or edits one in gh_chol_update.hip
// (gh_chol_impl.h).
#include <math.h>
#include <chrono>
#include "gh_chol_impl.h"
#include "../../include/george_amd_debug.h"

// ============================================================= potf2 + inverse
// One workgroup factorises a 128x128 block held entirely in LDS (129 KiB) and
// inverts the triangular factor; `dinv` receives L^-1 (row-major 128x128, zeros
// above the diagonal).  info: 0 = ok so far; set to base+j+1 at the first
// non-positive pivot (LAPACK dpotrf `info`), after which every later call is a no-op.
__global__ __launch_bounds__(256) void potf2_inv_kernel(double* A, long lda, double* dinv,
                                                        long long* info, long long base) {
  __shared__ double s[T * LP];
  __shared__ int fail_at;
  const int tid = threadIdx.x;
  if (*info != 0) return;               // uniform: an earlier block already failed
  if (tid == 0) fail_at = -1;
  for (int idx = tid; idx < T * T; idx += 256) {
    const int i = idx >> 7, j = idx & 127;
    s[i * LP + j] = A[(long)i * lda + j];
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;       // 16x16 cyclic ownership of the trailing block
  for (int j = 0; j < T; ++j) {
    const double d = s[j * LP + j];
    if (!(d > 0.0)) {                            // also catches NaN
      if (tid == 0) fail_at = j;
      break;                                     // uniform: every thread read the same d
    }
    const double ajj = sqrt(d);
    __syncthreads();                             // everyone has read d before it is overwritten
    if (tid < T) {
      if (tid > j) s[tid * LP + j] /= ajj;
      else if (tid == j) s[j * LP + j] = ajj;
    }
    __syncthreads();
    // rank-1 update of the trailing lower triangle
    for (int i = j + 1 + ((ty - (j + 1)) & 15); i < T; i += 16) {
      const double lij = s[i * LP + j];
      for (int k = j + 1 + ((tx - (j + 1)) & 15); k <= i; k += 16)
        s[i * LP + k] -= lij * s[k * LP + j];
    }
    __syncthreads();
  }
  __syncthreads();
  if (fail_at >= 0) {
    if (tid == 0) *info = base + fail_at + 1;
    return;
  }
  // write the factor back, zeroing the strict upper triangle of the tile
  for (int idx = tid; idx < T * T; idx += 256) {
    const int i = idx >> 7, j = idx & 127;
    A[(long)i * lda + j] = (j <= i) ? s[i * LP + j] : 0.0;
  }
  __syncthreads();
  // L^-1, column by column: lane pair (c, h) owns column c, h splits the dot product by
  // k parity; x_i (i > c) is kept in the unused upper triangle at s[c][i].  No workgroup
  // barrier: a column only depends on itself, and the two lanes sit in one wavefront
  // (LDS operations of a wavefront execute in program order; volatile stops the compiler
  // from caching or reordering them).
  {
    volatile double* vs = s;
    const int c = tid >> 1, h = tid & 1;
    const double xc = 1.0 / vs[c * LP + c];
    for (int i = c + 1; i < T; ++i) {
      double acc = (h == 0) ? vs[i * LP + c] * xc : 0.0;
      for (int k = c + 1 + h; k < i; k += 2) acc += vs[i * LP + k] * vs[c * LP + k];
      acc += __shfl_xor(acc, 1, 64);
      const double xi = -acc / vs[i * LP + i];
      if (h == 0) vs[c * LP + i] = xi;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < T * T; idx += 256) {
    const int i = idx >> 7, j = idx & 127;       // dinv[i][j] = x_i of column j
    double v;
    if (j < i) v = s[j * LP + i];
    else if (j == i) v = 1.0 / s[i * LP + i];
    else v = 0.0;
    dinv[idx] = v;
  }
}

// ---- the process-wide streams (see gh_common.h)
#include <map>
#include <mutex>
namespace {
struct SharedStreams {
  hipStream_t q[4] = {nullptr, nullptr, nullptr, nullptr};
  bool made = false;
  bool main_crowded = false;       // the main stream shares a dispatcher with the chain, rows-below or near stream (measured when they are made)
  std::map<int, hipStream_t> masked;
};
std::mutex g_ss_mu;
std::map<int, SharedStreams> g_ss;
}
// (Where the runtime puts these streams matters more than which streams there are: DESIGN.md, "One set of streams per
//  process" -- gh_prime_device() takes care of the common case, gh_debug_stream_dispatch() shows the placement.)
namespace {
__global__ void place_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}
// ms until a one-workgroup kernel on `small` has completed when it is launched right after a ~1 ms grid (2^17 workgroups,
// far more than the chip holds) on `big`: ~0.05 when the two queues dispatch independently, the grid's duration when not
double dispatch_wait_ms(hipStream_t big, hipStream_t small) {
  (void)hipDeviceSynchronize();
  hipLaunchKernelGGL(place_spin_kernel, dim3(1 << 17), dim3(64), 0, big, 5000LL);
  const auto t0 = std::chrono::steady_clock::now();
  hipLaunchKernelGGL(place_spin_kernel, dim3(1), dim3(64), 0, small, 0LL);
  (void)hipStreamSynchronize(small);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  (void)hipDeviceSynchronize();
  return ms;
}
}  // namespace
// do kernels of `a` and `b` (streams of the current device) dispatch side by side?  (gh_mgpu.hip: two communicators at once)
bool gh_streams_dispatch_independently(hipStream_t a, hipStream_t b) {
  if (!a || !b || a == b) return false;
  hipLaunchKernelGGL(place_spin_kernel, dim3(1), dim3(64), 0, a, 0LL);          // (queues are made at first use)
  hipLaunchKernelGGL(place_spin_kernel, dim3(1), dim3(64), 0, b, 0LL);
  (void)hipDeviceSynchronize();
  const bool ok = dispatch_wait_ms(a, b) <= 0.3 && dispatch_wait_ms(b, a) <= 0.3;
  (void)hipGetLastError();
  return ok;
}
bool gh_shared_main_crowded(int device) {
  std::lock_guard<std::mutex> lk(g_ss_mu);
  auto it = g_ss.find(device);
  return it != g_ss.end() && it->second.main_crowded;
}
bool gh_shared_streams(int device, hipStream_t q[4]) {
  std::lock_guard<std::mutex> lk(g_ss_mu);
  SharedStreams& ss = g_ss[device];
  if (!ss.made) {
    ss.made = true;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return false; }
    gh_prime_device(device);
    if (hipStreamCreate(&ss.q[0]) != hipSuccess) { ss.q[0] = nullptr; (void)hipGetLastError(); }
    int lo = 0, hi = 0;                    // numerically lowest value = highest priority
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    // (the rows-below and near streams at normal or low priority instead of the chain's: no difference, 6.98 / 7.07 / 7.02 ms at N = 8192)
    for (int i = 1; i < 4 && ss.q[0]; ++i)
      if (hipStreamCreateWithPriority(&ss.q[i], hipStreamNonBlocking, hi) != hipSuccess) { ss.q[i] = nullptr; (void)hipGetLastError(); break; }
    // Does the main stream share a dispatcher with one of the panel streams?  (Which queues end up together depends on how
    // many the process made before: never in a process that made none, with the rows-below stream after five application
    // streams, with the chain stream after six.)  Decides where a look-ahead factorisation is joined: factor_lookahead_deep.
    if (ss.q[0] && ss.q[1] && ss.q[2] && ss.q[3]) {
      for (int i = 0; i < 4; ++i) hipLaunchKernelGGL(place_spin_kernel, dim3(1), dim3(64), 0, ss.q[i], 0LL);   // (queues are made at first use)
      (void)hipDeviceSynchronize();
      for (int i = 1; i < 4 && !ss.main_crowded; ++i)
        ss.main_crowded = dispatch_wait_ms(ss.q[0], ss.q[i]) > 0.3 || dispatch_wait_ms(ss.q[i], ss.q[0]) > 0.3;
      (void)hipGetLastError();
    }
  }
  for (int i = 0; i < 4; ++i) q[i] = ss.q[i];
  return ss.q[0] != nullptr;
}
hipStream_t gh_shared_masked_stream(int device, int reserve_cus) {
  std::lock_guard<std::mutex> lk(g_ss_mu);
  SharedStreams& ss = g_ss[device];
  auto it = ss.masked.find(reserve_cus);
  if (it != ss.masked.end()) return it->second;
  hipStream_t st = nullptr;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 2 * reserve_cus) {
    const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
    std::vector<uint32_t> mask(words, 0u);
    for (int c = reserve_cus; c < ncu; ++c) mask[c / 32] |= (1u << (c % 32));
    if (hipExtStreamCreateWithCUMask(&st, words, mask.data()) != hipSuccess) { st = nullptr; (void)hipGetLastError(); }
  }
  ss.masked[reserve_cus] = st;             // (a failed creation is not retried)
  return st;
}

int gh_chol_set_device(gh_chol* s) {
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd solver needs an MI355X"); return GH_ERR_HIP; }
  GH_HIP(hipSetDevice(s->opts.device));
  return GH_OK;
}

extern "C" int gh_chol_create(const gh_chol_opts* opts, gh_chol** out) {
  if (!out) { gh_set_error("null output"); return GH_ERR_BAD_ARG; }
  gh_chol* s = new gh_chol();
  memset(&s->opts, 0, sizeof(s->opts));
  memset(&s->prof, 0, sizeof(s->prof));
  if (opts) s->opts = *opts;
  if (s->opts.nb < 0) s->opts.nb = 0;       // 0 = choose per problem size (panel_width())
  if (s->opts.nb % T) { delete s; gh_set_error("nb must be a multiple of 128"); return GH_ERR_BAD_ARG; }
  int rc = gh_chol_set_device(s);
  if (rc != GH_OK) { delete s; return rc; }
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  if (gh_shared_streams(s->opts.device, shq)) {
    s->shared_streams = true;
    s->st = shq[0];
  } else {
    gh_prime_device(s->opts.device);
    if (hipStreamCreate(&s->st) != hipSuccess) { delete s; gh_set_error("hipStreamCreate failed"); return GH_ERR_HIP; }
  }
  if (s->opts.lookahead) {
    int lo = 0, hi = 0;                    // numerically lowest value = highest priority
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (s->shared_streams) s->st2 = shq[1];
    else if (hipStreamCreateWithPriority(&s->st2, hipStreamNonBlocking, hi) != hipSuccess) { s->st2 = nullptr; (void)hipGetLastError(); }
    for (auto& e : s->ev_sync)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete s; gh_set_error("hipEventCreate failed"); return GH_ERR_HIP; }
    if (s->st2) {
      if (s->shared_streams) s->st3 = shq[2];
      bool ok = (s->shared_streams ? s->st3 != nullptr : hipStreamCreateWithPriority(&s->st3, hipStreamNonBlocking, hi) == hipSuccess) &&
                hipEventCreateWithFlags(&s->ev_aux, hipEventDisableTiming) == hipSuccess;
      for (auto& e : s->ev_diag) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
      if (!ok) { (void)hipGetLastError(); if (s->st3 && !s->shared_streams) (void)hipStreamDestroy(s->st3); s->st3 = nullptr; }
      if (s->st3) {
        if (s->shared_streams) s->st4 = shq[3];
        bool ok4 = (s->shared_streams ? s->st4 != nullptr : hipStreamCreateWithPriority(&s->st4, hipStreamNonBlocking, hi) == hipSuccess) &&
                   hipEventCreateWithFlags(&s->ev_aux2, hipEventDisableTiming) == hipSuccess;
        if (!ok4) { (void)hipGetLastError(); if (s->st4 && !s->shared_streams) (void)hipStreamDestroy(s->st4); s->st4 = nullptr; }
      }
    }
  }
  *out = s;
  return GH_OK;
}
// Which of the handle's streams really run side by side?  HIP maps streams onto a few hardware queues
// and two streams on one queue serialise.  out[i * 6 + j] (i < j) = milliseconds for a 300-us spin
// kernel on stream i and one on stream j launched together (0.3 = concurrent, 0.6 = one queue);
// streams: 0 the caller's null stream, 1 main, 2 chain, 3 rows-below, 4 near, 5 CU-masked trailing.
__global__ void spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) {}
}
extern "C" int gh_debug_stream_overlap(gh_chol* s, double* out, int n) {
  if (!s || !out || n < 36) { gh_set_error("bad argument"); return GH_ERR_BAD_ARG; }
  int rc = gh_chol_set_device(s);
  if (rc != GH_OK) return rc;
  hipStream_t q[6] = {nullptr, s->st, s->st2, s->st3, s->st4, s->st_mask};
  for (int i = 0; i < 36; ++i) out[i] = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = i + 1; j < 6; ++j) {
      if ((i > 0 && !q[i]) || !q[j]) { out[i * 6 + j] = -1.0; continue; }
      GH_HIP(hipDeviceSynchronize());
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, q[i], 30000LL);
      hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, q[j], 30000LL);
      GH_HIP(hipDeviceSynchronize());
      out[i * 6 + j] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  return GH_OK;
}
// The other way two streams can be in each other's way: a grid with far more workgroups than the chip holds keeps
// its queue's dispatcher busy for its whole duration.  out[i * 6 + j] (i != j) = milliseconds until a ONE-workgroup
// kernel launched on stream j right after such a grid on stream i (2^18 workgroups of 64 threads spinning ~50 us:
// ~2 ms) has completed: tens of microseconds when the two queues dispatch independently, the grid's duration when the
// small kernel has to wait for the big one's dispatch to end.  Streams as in gh_debug_stream_overlap.
extern "C" int gh_debug_stream_dispatch(gh_chol* s, double* out, int n) {
  if (!s || !out || n < 36) { gh_set_error("bad argument"); return GH_ERR_BAD_ARG; }
  int rc = gh_chol_set_device(s);
  if (rc != GH_OK) return rc;
  hipStream_t q[6] = {nullptr, s->st, s->st2, s->st3, s->st4, s->st_mask};
  for (int i = 0; i < 36; ++i) out[i] = 0.0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      if (i == j) continue;
      if ((i > 0 && !q[i]) || (j > 0 && !q[j])) { out[i * 6 + j] = -1.0; continue; }
      GH_HIP(hipDeviceSynchronize());
      hipLaunchKernelGGL(spin_kernel, dim3(1 << 18), dim3(64), 0, q[i], 5000LL);
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, q[j], 0LL);
      GH_HIP(hipStreamSynchronize(q[j]));
      out[i * 6 + j] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      GH_HIP(hipDeviceSynchronize());
    }
  return GH_OK;
}
extern "C" void gh_chol_destroy(gh_chol* s) {
  if (!s) return;
  (void)hipSetDevice(s->opts.device);
  // entry points that were handed DEVICE output pointers return with copies still queued: drain the
  // handle's streams before its buffers go back to the allocator / the block cache
  for (hipStream_t st : {s->st, s->st2, s->st3, s->st4, s->st_mask}) if (st) (void)hipStreamSynchronize(st);
  delete s;
}
extern "C" int64_t gh_chol_info(const gh_chol* s) { return s ? s->info : 0; }
extern "C" int64_t gh_chol_size(const gh_chol* s) { return s ? s->n : 0; }
extern "C" int64_t gh_chol_device_bytes(const gh_chol* s) {
  if (!s) return 0;
  size_t tot = 0;
  for (const GhBuf* b : {&s->A, &s->A_spare, &s->dinv, &s->x, &s->yerr, &s->v0, &s->v1, &s->v2, &s->scal, &s->rhs, &s->work, &s->work2,
                         &s->scratch, &s->chain, &s->lv, &s->samp, &s->fish, &s->lgo}) tot += b->p ? b->bytes : 0;
  return (int64_t)(tot + gh_batch_bytes(s->batch));
}
int gh_chol_batch_begin(gh_chol* s, hipStream_t* st, GhBatchBufs** bufs) {
  GH_CHECK(gh_chol_set_device(s));
  s->computed = false;
  s->info = 0;
  if (!s->batch) s->batch = gh_batch_new();
  *st = s->st;
  *bufs = s->batch;
  return GH_OK;
}
extern "C" int gh_chol_get_update_intervals(const gh_chol* s, double* out, int32_t max_launches, int32_t* n_out) {
  if (!s || !n_out || (max_launches > 0 && !out)) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  const int32_t have = (int32_t)(s->upd_intervals.size() / 3);
  *n_out = have;
  for (int32_t i = 0; i < have && i < max_launches; ++i)
    for (int q = 0; q < 3; ++q) out[3 * i + q] = s->upd_intervals[3 * (size_t)i + q];
  return GH_OK;
}
extern "C" int gh_chol_get_profile(const gh_chol* s, gh_chol_profile* out) {
  if (!s || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  *out = s->prof;
  return GH_OK;
}

static inline double* blk(double* A, int64_t ld, int64_t r, int64_t c) { return A + r * ld + c; }

// C = alpha A B^T + beta C on k-major operands
// (set by factor(): the K = 128 GEMMs of the chain hold 128-144 KiB of LDS per workgroup -- a whole CU.  Below
//  Np = 24576 the trailing SYRK leaves 32 CUs out and they run there; above it every CU carries two SYRK
//  workgroups and a chain workgroup that needs a CU to itself waits for one to drain while the dispatcher
//  holds it empty: N = 65536 went from 1.407 to 1.433 s.  There they keep the 32-KiB K-loop kernel.)
static thread_local bool t_gemm_small_lds = false;
// t_gemm_small_lds for a scope
struct SmallLdsGuard { bool prev; explicit SmallLdsGuard(bool v) : prev(t_gemm_small_lds) { t_gemm_small_lds = v; } ~SmallLdsGuard() { t_gemm_small_lds = prev; } };
int gh_gemm_nt(hipStream_t st, double* C, int64_t ldc, const double* A, int64_t lda, const double* B, int64_t ldb,
               int64_t M, int64_t N, int64_t K, double alpha, double beta, bool lower) {
  GhGemm g = gemm_desc(C, ldc, A, lda, true, B, ldb, true, M, N, K, alpha, beta);
  g.small_lds = t_gemm_small_lds;
  g.lower = lower;
  return gh_launch_gemm(g, st);
}

// gh_potf2.hip: MFMA-blocked 128x128 Cholesky + inverse (the default); GEORGE_AMD_POTF2=simple
// selects the first scalar version above for A/B validation
static bool use_simple_potf2() {
  static int v = -1;
  if (v < 0) { const char* e = getenv("GEORGE_AMD_POTF2"); v = (e && e[0] == 's') ? 1 : 0; }
  return v == 1;
}

// in-place lower Cholesky of the n x n block at A (n multiple of 128) + diagonal-block inverses
int gh_chol_potrf_block(hipStream_t st, double* A, int64_t ld, int64_t n, double* dinv, long long* d_info, long long base) {
  for (int64_t j0 = 0; j0 < n; j0 += T) {
    double* dj = dinv + (j0 / T) * T * T;
    if (use_simple_potf2()) {
      hipLaunchKernelGGL(potf2_inv_kernel, dim3(1), dim3(256), 0, st, blk(A, ld, j0, j0), (long)ld, dj, d_info, base + j0);
      GH_HIP(hipGetLastError());
    } else {
      GH_CHECK(gh_launch_potf2_mfma(blk(A, ld, j0, j0), ld, dj, d_info, base + j0, st));
    }
    const int64_t rem = n - (j0 + T);
    if (rem > 0) {
      double* P = blk(A, ld, j0 + T, j0);
      GH_CHECK(gh_gemm_nt(st, P, ld, P, ld, dj, T, rem, T, T, 1.0, 0.0, false));          // P <- P L_jj^-T (in place)
      GH_CHECK(gh_gemm_nt(st, blk(A, ld, j0 + T, j0 + T), ld, P, ld, P, ld, rem, rem, T, -1.0, 1.0, true));
    }
  }
  return GH_OK;
}
// A21 (m x n) <- A21 L11^-T, L11 n x n lower with diagonal-block inverses dinv
static int trsm_right(hipStream_t st, const double* L11, int64_t ld11, const double* dinv, double* A21, int64_t lda, int64_t m, int64_t n) {
  for (int64_t j0 = 0; j0 < n; j0 += T) {
    double* Xj = A21 + j0;
    if (j0 > 0)
      GH_CHECK(gh_gemm_nt(st, Xj, lda, A21, lda, L11 + j0 * ld11, ld11, m, T, j0, -1.0, 1.0, false));
    GH_CHECK(gh_gemm_nt(st, Xj, lda, Xj, lda, dinv + (j0 / T) * T * T, T, m, T, T, 1.0, 0.0, false));
  }
  return GH_OK;
}

extern "C" int gh_dev_potrf_block(double* a, int64_t lda, int64_t n, double* dinv, int64_t* info_dev, int64_t base_index, void* stream) {
  if (n % T) { gh_set_error("potrf_block: n must be a multiple of 128"); return GH_ERR_BAD_ARG; }
  // (tile operations of the multi-GPU driver run beside trailing updates that own every CU: small-LDS GEMMs, see t_gemm_small_lds)
  SmallLdsGuard guard(true);
  return gh_chol_potrf_block((hipStream_t)stream, a, lda, n, dinv, (long long*)info_dev, base_index);
}
extern "C" int gh_dev_trsm_right(const double* l11, int64_t ld11, const double* dinv, double* a21, int64_t lda, int64_t m, int64_t n, void* stream) {
  if (n % T || m % T) { gh_set_error("trsm_right: sizes must be multiples of 128"); return GH_ERR_BAD_ARG; }
  SmallLdsGuard guard(true);
  return trsm_right((hipStream_t)stream, l11, ld11, dinv, a21, lda, m, n);
}
extern "C" int gh_dev_trsv_lower(const double* l, int64_t ldl, const double* dinv, int64_t n,
                                 const double* w, double* z, void* scratch, void* stream) {
  if (n % T || n <= 0 || !scratch) { gh_set_error("trsv_lower: n must be a positive multiple of 128"); return GH_ERR_BAD_ARG; }
  const int64_t nt = n / T;
  if (w == z) { gh_set_error("trsv_lower: w and z must not be the same array"); return GH_ERR_BAD_ARG; }
  return gh_launch_trsv_fwd_chain(l, (long)ldl, dinv, nt, w, z, (unsigned*)scratch, (hipStream_t)stream);
}
extern "C" int gh_dev_trsv_lower_t(const double* l, int64_t ldl, const double* dinv, int64_t n,
                                   const double* w, double* x, void* scratch, void* stream) {
  if (n % T || n <= 0 || !scratch) { gh_set_error("trsv_lower_t: n must be a positive multiple of 128"); return GH_ERR_BAD_ARG; }
  const int64_t nt = n / T;
  if (w == x) { gh_set_error("trsv_lower_t: w and x must not be the same array"); return GH_ERR_BAD_ARG; }
  return gh_launch_trsv_bwd_chain(l, (long)ldl, dinv, nt, w, x, (unsigned*)scratch, (hipStream_t)stream);
}
extern "C" int gh_dev_logdet_accum(const double* a, int64_t lda, int64_t n, double* out_dev, void* stream) {
  return gh_launch_logdet_accum(a, (long)lda, (long)n, out_dev, (hipStream_t)stream);
}

// Outer panel width.  Wider panels raise the SYRK's arithmetic intensity and K-loop length and
// halve the number of look-ahead hand-overs, but put more work into the latency-bound panel chain.
// Measured (bench.py --nb, after the chain work of this round): 1024 wins from N = 16384 up
// (N = 16384: 36.5 vs 37.8 ms, N = 20480: 60.7 vs 63.3 ms, N = 65536: 1437 vs 1480 ms), 512 at
// N = 8192 (10.9 vs 11.2 ms), 1024 again at N <= 4096 (4.95 vs 5.03 ms at 4096, 1.16 vs 1.26 ms
// at 1024: the fewer hand-overs between the streams the better), 128 and 256 nowhere.
static int64_t panel_width(const gh_chol* s) {
  if (s->opts.nb > 0) return s->opts.nb;
  // (swept again after the second 128x128 kernel and the K = 128 GEMM, N = 2048 .. 20480, nb = 256 .. 2048:
  //  1024 wins or ties everywhere -- 512 used to win between 4096 and 12288, when a chain link cost twice as much)
  return 1024;
}
// Start columns of the outer panels, pc[0] = 0 < pc[1] < ... < pc[P] = Np.  With the width left to the solver (opts.nb == 0) the
// panels are 2048 columns wide while the trailing matrix behind them is larger than GH_WIDE_PANEL_MIN_TRAILING columns and 1024
// after (round 6; round 5 measured a uniform 2048 at -1.4 % for N = 65536 and +3.6 % for N = 32768: the K = 2048 update runs its
// tiles 2 % faster and halves the launches, but a 2048-column panel is sixteen chain links + a block-column update twice as
// deep, which only a trailing update of more than ~20 ms hides -- at 66 TFLOP/s that is a trailing matrix of ~25 000 columns).
#ifndef GH_WIDE_PANEL_MIN_TRAILING
#define GH_WIDE_PANEL_MIN_TRAILING 25600
#endif

static int g_build_on_chain = 1;
extern "C" int gh_debug_set_build_on_chain(int on) {
  const int prev = g_build_on_chain;
  g_build_on_chain = on ? 1 : 0;
  return prev;
}
static int g_adaptive_panels = 1;        // 0: off; 1: on (GH_WIDE_PANEL_MIN_TRAILING); > 1: on with this many trailing columns as the bound
extern "C" int gh_debug_set_adaptive_panels(int on) {
  const int prev = g_adaptive_panels;
  g_adaptive_panels = on < 0 ? 1 : on;
  return prev;
}
static std::vector<int64_t> panel_starts(const gh_chol* s) {
  const bool adaptive = s->opts.nb == 0 && g_adaptive_panels && !use_simple_potf2();
  const int64_t bound = g_adaptive_panels > 1 ? g_adaptive_panels : GH_WIDE_PANEL_MIN_TRAILING;
#ifdef GH_WIDE_PANEL_TIER2
  return gh_plan_panel_starts(s->np, panel_width(s), adaptive ? bound : 0, GH_WIDE_PANEL_TIER2);
#else
  return gh_plan_panel_starts(s->np, panel_width(s), adaptive ? bound : 0);
#endif
}

// One panel step: factor the nb x nb diagonal block at k0, TRSM the rows below it.
static int panel_step(gh_chol* s, hipStream_t st, int64_t k0, int64_t nb) {
  double* A = s->A.d();
  const int64_t np = s->np, ld = np;
  double* dinv = s->dinv.d() + (k0 / T) * T * T;
  const int64_t m = np - (k0 + nb);
  const bool on_panel_stream = (st == s->st2);
  // (Retired arms, all measured and slower, sources under scripts/dev/arms/: only row block j+1 on the chain and the
  //  other in-panel rows on a third stream; the chain on CUs of its own; only the potf2 launches on reserved CUs; the
  //  whole panel as two persistent flag-driven launches.  DESIGN.md section 4, "Where N < 24k stands".)
  if (!s->st3 || !on_panel_stream || m <= 0 || nb / T > 32 || use_simple_potf2()) {
    GH_CHECK(gh_chol_potrf_block(st, blk(A, ld, k0, k0), ld, nb, dinv, s->d_info, k0));
    if (m > 0) {
      GH_CHECK(trsm_right(st, blk(A, ld, k0, k0), ld, dinv, blk(A, ld, k0 + nb, k0), ld, m, nb));
    }
    return GH_OK;
  }
  // Look-ahead panels: the potf2 chain of the diagonal block stays on `st`; the TRSM of the rows
  // below runs on a second panel stream, column block j as soon as L_jj^-1 exists, so that only
  // the last block's TRSM is left when the chain ends (instead of all nb/128 of them).
  hipStream_t sa = s->st3;
  double* Ak = blk(A, ld, k0, k0);
  double* B = blk(A, ld, k0 + nb, k0);
  // (the rows-below stream's first operation waits for ev_diag[0], recorded on `st` behind everything this panel needs: no event of
  //  its own at the panel's start -- a record costs the recording stream ~6 us before its next kernel)
  for (int64_t j0 = 0; j0 < nb; j0 += T) {
    double* dj = dinv + (j0 / T) * T * T;
    GH_CHECK(gh_launch_potf2_mfma(blk(Ak, ld, j0, j0), ld, dj, s->d_info, k0 + j0, st));
    GH_HIP(hipEventRecord(s->ev_diag[j0 / T], st));
    GH_HIP(hipStreamWaitEvent(sa, s->ev_diag[j0 / T], 0));
    double* Xj = B + j0;
    if (j0 > 0) GH_CHECK(gh_gemm_nt(sa, Xj, ld, B, ld, Ak + j0 * ld, ld, m, T, j0, -1.0, 1.0, false));
    GH_CHECK(gh_gemm_nt(sa, Xj, ld, Xj, ld, dj, T, m, T, T, 1.0, 0.0, false));
    const int64_t rem = nb - (j0 + T);
    if (rem > 0) {
      double* P = blk(Ak, ld, j0 + T, j0);
      GH_CHECK(gh_gemm_nt(st, P, ld, P, ld, dj, T, rem, T, T, 1.0, 0.0, false));
      GH_CHECK(gh_gemm_nt(st, blk(Ak, ld, j0 + T, j0 + T), ld, P, ld, P, ld, rem, rem, T, -1.0, 1.0, true));
    }
  }
  GH_HIP(hipEventRecord(s->ev_aux, sa));
  GH_HIP(hipStreamWaitEvent(st, s->ev_aux, 0));
  return GH_OK;
}

// Right-looking factorisation with one-panel look-ahead on two HIP streams:
//   main stream  : trailing updates (the MFMA-bound >90 % of the work);
//   panel stream : (high priority) potf2/TRSM chain of the NEXT panel, which is latency-bound
//                  and would otherwise sit on the critical path between two trailing updates.
// Step k: the main stream first updates only block column k+1 (the next panel), signals the panel
// stream, then updates the rest of the trailing matrix while the panel stream factors panel k+1.
// The two touch disjoint regions: panel k+1 = columns [k1, k1+nb1), the remainder = rows and
// columns >= k1+nb1; both only READ panel k.
// Small matrices are bound by the panel chain (128 potf2 workgroups in a row at N = 16384), and
// that chain runs 4x slower when its workgroups share a CU with wavefronts of the trailing SYRK
// (in-kernel timers: potf2 114 us alone, 420-480 us beside SYRK -- LDS-queue contention, wavefront
// priority does not help).  For those sizes the trailing updates go to a stream whose CU mask
// leaves 32 CUs free for the panel stream.  The count is not arbitrary: the mask bits are dealt
// round-robin over the 8 XCDs and then over the 4 shader engines of each, and the workgroup
// dispatcher feeds shader engines evenly -- leaving out 8 CUs (one engine of every XCD one CU
// short) costs the SYRK 12 %, the same as leaving out 32 (every engine one short), so 32 it is:
// 12.5 % of the chip, about the panel's share of the flops at N = 16384 (9 %).  Larger matrices
// hide the chain behind the SYRK anyway and keep all 256 CUs.  The masked stream takes ~1 s to
// create (ROCm 7.2): once per process (gh_shared_masked_stream).  GEORGE_AMD_RESERVE_CUS=0 disables, =<n> forces n CUs.
static hipStream_t trailing_stream(gh_chol* s) {
  int want = s->np < 24576 ? 32 : 0;
  if (const char* e = getenv("GEORGE_AMD_RESERVE_CUS")) want = atoi(e);
  if (want <= 0 || want >= 128) return s->st;
  if (s->mask_reserved != want) {
    if (s->st_mask) { (void)hipStreamSynchronize(s->st_mask); if (!s->shared_streams) (void)hipStreamDestroy(s->st_mask); s->st_mask = nullptr; }
    s->mask_reserved = want;                                       // (a failed creation is not retried)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->opts.device) == hipSuccess && prop.multiProcessorCount > 2 * want) {
      const int ncu = prop.multiProcessorCount, words = (ncu + 31) / 32;
      std::vector<uint32_t> mask(words, 0u);
      for (int c = want; c < ncu; ++c) mask[c / 32] |= (1u << (c % 32));
      if (s->shared_streams) s->st_mask = gh_shared_masked_stream(s->opts.device, want);
      else if (hipExtStreamCreateWithCUMask(&s->st_mask, words, mask.data()) != hipSuccess) { s->st_mask = nullptr; (void)hipGetLastError(); }
    }
    if (s->st_mask && !s->ev_xfer && hipEventCreateWithFlags(&s->ev_xfer, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError(); if (!s->shared_streams) (void)hipStreamDestroy(s->st_mask); s->st_mask = nullptr;
    }
  }
  return s->st_mask ? s->st_mask : s->st;
}

// Look-ahead of depth d.  After panel j is factored, its trailing update is issued per block column
// for the d columns next to it and as ONE lower-triangular SYRK for the rest:
//   chain stream `sp` : panel(j) -> U(j, j+1) -> panel(j+1) -> ...            (the critical path)
//   near stream  `sn` : U(j, j+2), ..., U(j, j+d)                             (narrow GEMMs, high priority)
//   main stream  `sm` : W(j) = U(j, j+d+1 ...)                                (the wide SYRK)
// U(j, c): A[c0:, c0:c0+nb_c] -= L[c0:, j-panel] L[c0:c0+nb_c, j-panel]^T.  Every column receives its
// updates in panel order: U(j, c) follows U(j-1, c), which is the previous launch of the same
// stream except at the window's edges -- U(j, j+1) follows U(j-1, j+1) from the near stream (event
// ev_nf[j-1]), U(j, j+d) follows W(j-1) (event ev_w[j-1]) -- and everything of panel j follows
// ev_p[j].  With d = 1 the chain can start panel j+1 only when W(j-1) is over, so at sizes where the
// early SYRKs outlast a panel and the late ones do not (N ~ 8k-24k) the total is the SUM of the
// larger of the two per step; with d > 1 the chain runs up to d panels ahead during the SYRK-bound
// early steps and spends that lead in the chain-bound late ones.
static int factor_lookahead_deep(gh_chol* s, int depth) {
  // depth 1 (the default): the only work of the "near" stream is the rows below the diagonal block of
  // U(j, j+1), and the first thing that needs them is the rows-below TRSM of panel j+1 on st3 -- so it
  // goes to st3 itself: one hardware queue less.  (The process degrades by 20-40 % at N <= 16384 once
  // eight queues are in use -- null stream + this handle's + the application's; scripts/dev/queue_pattern.py.)
  hipStream_t sm = trailing_stream(s), sn = (depth == 1 && s->st3) ? s->st3 : s->st4;
  hipStream_t sp = s->st2;
  // Which stream a wide update W(j) runs on when `sm` is the CU-masked one (Np < 24576: 32 CUs kept free for the chain, worth
  // 12 % of the SYRK's rate): the reservation pays where the step is bound by the chain -- the late panels -- and costs where
  // it is bound by W(j) itself, the first panels, whose chain ends long before their update does.  W(j) longer than
  // GH_FULLCHIP_MS (estimated at 60 TFLOP/s) goes to the unmasked main stream; consecutive updates on different streams are
  // ordered through ev_w, and the chain's K = 128 GEMMs follow (t_gemm_small_lds below).  Measured (profiles/r04/schedule_ab.md):
  // N = 16384 29.08 -> 28.57 ms, 20480 51.9 -> 50.1, 24064 80.9 -> 76.8; a threshold of 1.2 ms loses 1.6 % at 12288 / 16384;
  // the same rule above Np = 24576 (late panels on the masked stream) is worth 1.3 % at 24576, nothing at 32768 and 65536 --
  // not the second it takes to make the masked stream.
#ifndef GH_FULLCHIP_MS
#define GH_FULLCHIP_MS 2.5
#endif
  const std::vector<int64_t> pc = panel_starts(s);
  auto wide_stream = [&](int j) -> hipStream_t {
    if (sm == s->st) return sm;
    const int cwj = j + depth + 1;
    if (j < 0 || cwj > (int)pc.size() - 2) return sm;
    const double m2 = (double)(s->np - pc[cwj]);
    const double ms = (m2 / T) * (m2 / T + 1.0) / 2.0 * 2.0 * T * T * (double)(pc[j + 1] - pc[j]) / 60e12 * 1e3;
    return ms > GH_FULLCHIP_MS ? s->st : sm;
  };
  hipStream_t sw_prev = nullptr;
  double* A = s->A.d();
  const int64_t np = s->np, ld = np;
  const int P = (int)pc.size() - 1;
  // (measured at N = 16384, depth 1: whole block column on the chain 34.8 ms; diagonal block on the chain + rows
  //  below on the near stream 35.6; the same with the chain on CUs of its own 48.5 -- retired, scripts/dev/arms/)
  const bool prof = s->opts.profile != 0;
  while ((int)s->ev_p.size() < P) {
    hipEvent_t e[3];
    for (auto& x : e) GH_HIP(hipEventCreateWithFlags(&x, hipEventDisableTiming));
    s->ev_p.push_back(e[0]); s->ev_w.push_back(e[1]); s->ev_nf.push_back(e[2]);
  }
  auto c0 = [&](int c) { return pc[c]; };
  auto nbc = [&](int c) { return pc[c + 1] - pc[c]; };
  auto narrow = [&](hipStream_t st, int j, int c) -> int {         // U(j, c)
    const double* Pj = blk(A, ld, c0(c), c0(j));
    const long eu = prof ? s->next_ev() : -1;
    if (eu >= 0) { GH_HIP(hipEventRecord(s->ev_pool[eu].a, st)); s->ev_update.push_back((size_t)eu); }
    GH_CHECK(gh_gemm_nt(st, blk(A, ld, c0(c), c0(c)), ld, Pj, ld, Pj, ld, np - c0(c), nbc(c), nbc(j), -1.0, 1.0, false));
    if (eu >= 0) GH_HIP(hipEventRecord(s->ev_pool[eu].b, st));
    // (algorithmic flops of the block column: its lower part only -- the strictly-upper tiles of the
    //  diagonal block are computed for convenience and never read)
    const double tr = (double)(np - c0(c)) / T, tc = (double)nbc(c) / T;
    const double fl = (tr * tc - tc * (tc - 1.0) / 2.0) * 2.0 * T * T * (double)nbc(j);
    s->prof.update_flops += fl;
    if (eu >= 0) s->ev_update_flops.push_back(fl);
    return GH_OK;
  };
  // everything queued so far (the build, on s->st) before any of the three streams starts
  if (!s->build_on_chain) {
    GH_HIP(hipEventRecord(s->ev_sync[0], s->st));
    GH_HIP(hipStreamWaitEvent(sp, s->ev_sync[0], 0));
    GH_HIP(hipStreamWaitEvent(sn, s->ev_sync[0], 0));
    if (sm != s->st) GH_HIP(hipStreamWaitEvent(sm, s->ev_sync[0], 0));
  }   // (else the build is the chain stream's own work: the rows-below stream follows ev_aux, the update streams ev_p[0])
  for (int j = 0; j < P; ++j) {
    // ---- chain: column j is complete once U(j-1, j) has run (issued at the end of the previous turn)
    {
      const long ep = prof ? s->next_ev() : -1;
      if (ep >= 0) { GH_HIP(hipEventRecord(s->ev_pool[ep].a, sp)); s->ev_panel.push_back((size_t)ep); }
      // (panel j runs beside W(j-1): where that update owns every CU, the chain's K = 128 GEMMs keep to 32 KiB of LDS -- t_gemm_small_lds)
      t_gemm_small_lds = wide_stream(j >= 1 ? j - 1 : 0) == s->st;
      GH_CHECK(panel_step(s, sp, c0(j), nbc(j)));
      if (ep >= 0) GH_HIP(hipEventRecord(s->ev_pool[ep].b, sp));
      GH_HIP(hipEventRecord(s->ev_p[j], sp));
    }
    if (j + 1 >= P) break;
    // ---- U(j, j+1): the whole block column on the chain stream (its diagonal block is what the potf2 chain of
    // panel j+1 needs, the rows below it what that panel's rows-below TRSM needs)
    const hipEvent_t prev = (j >= 1) ? (depth >= 2 ? s->ev_nf[j - 1] : s->ev_w[j - 1]) : nullptr;
    if (prev) GH_HIP(hipStreamWaitEvent(sp, prev, 0));
    GH_CHECK(narrow(sp, j, j + 1));
    // ---- U(j, j+2 .. j+d) on the near stream
    const int last_near = std::min(j + depth, P - 1);
    if (j + 2 <= last_near || (depth >= 2 && j + 2 <= P - 1)) GH_HIP(hipStreamWaitEvent(sn, s->ev_p[j], 0));
    for (int c = j + 2; c <= last_near; ++c) {
      if (c == j + depth && j >= 1) GH_HIP(hipStreamWaitEvent(sn, s->ev_w[j - 1], 0));      // column c was inside W(j-1)
      GH_CHECK(narrow(sn, j, c));
      if (c == j + 2) GH_HIP(hipEventRecord(s->ev_nf[j], sn));
    }
    if (depth >= 2 && j + 2 > last_near) GH_HIP(hipEventRecord(s->ev_nf[j], sn));        // (nothing to do: keep the event defined)
    // ---- W(j): the rest, one lower-triangular SYRK on the main stream
    const int cw = j + depth + 1;
    hipStream_t sw = wide_stream(j);
    if (sw_prev && sw_prev != sw && j >= 1) GH_HIP(hipStreamWaitEvent(sw, s->ev_w[j - 1], 0));      // W(j-1) ran on the other stream
    sw_prev = sw;
    GH_HIP(hipStreamWaitEvent(sw, s->ev_p[j], 0));
    if (cw <= P - 1) {
      const int64_t kw = c0(cw), m2 = np - kw;
      const long et = prof ? s->next_ev() : -1;
      if (et >= 0) {
        GH_HIP(hipEventRecord(s->ev_pool[et].a, sw)); s->ev_trailing.push_back((size_t)et); s->ev_update.push_back((size_t)et);
        s->ev_update_flops.push_back((double)(m2 / T) * (m2 / T + 1) / 2.0 * 2.0 * T * T * (double)nbc(j));
      }
      const double* P2 = blk(A, ld, kw, c0(j));
      GH_CHECK(gh_gemm_nt(sw, blk(A, ld, kw, kw), ld, P2, ld, P2, ld, m2, m2, nbc(j), -1.0, 1.0, true));
      if (et >= 0) GH_HIP(hipEventRecord(s->ev_pool[et].b, sw));
      const double tiles = (double)(m2 / T) * (m2 / T + 1) / 2.0;
      s->prof.trailing_flops += tiles * 2.0 * T * T * (double)nbc(j);
      s->prof.update_flops += tiles * 2.0 * T * T * (double)nbc(j);
      s->prof.n_trailing += 1;
    }
    GH_HIP(hipEventRecord(s->ev_w[j], sw));
  }
  // JOIN -- on the CHAIN stream, not on the main stream.  The host is far ahead of the device here, and a
  // hipStreamWaitEvent on the main stream issued now would sit at the head of that queue as a barrier packet for the whole
  // factorisation.  That is not free: whichever stream shares a DISPATCHER with the main stream (gh_debug_stream_dispatch;
  // which one does depends on how many queues the process made before) is served between polls of that barrier -- with the
  // chain or the rows-below stream there, N = 8192 took 11.0-12.8 instead of 7.2 ms per step (an application with five or
  // six streams of its own: profiles/r03/stream_placement_states.txt).  At the END of the chain's queue the same barriers
  // hold nothing up: the queue reaches them after its own last panel.  The caller continues on s->tail (log-det, copies).
  // (Waiting on the host for the last panel and joining on the main stream then works too, but costs 0.4 ms per step with a
  //  blocking wait and slows the device work by ~0.6 % when the host polls the event.)
  // In the placement a process gets that made no queues before, the main stream shares its dispatcher with the CU-masked
  // stream only, and there the join on the main stream is the faster one (N = 8192: 7.0 vs 7.3 ms, same box): the chain
  // join is used when the main stream was FOUND to share a dispatcher with a panel stream when the set was made
  // (gh_shared_main_crowded), and always with streams of the handle's own.
  const bool join_on_chain = !s->shared_streams || gh_shared_main_crowded(s->opts.device);
  if (sm != s->st && join_on_chain) {
    GH_HIP(hipEventRecord(s->ev_sync[2], sn));
    GH_HIP(hipStreamWaitEvent(sp, s->ev_sync[2], 0));
    GH_HIP(hipEventRecord(s->ev_xfer, sm));
    GH_HIP(hipStreamWaitEvent(sp, s->ev_xfer, 0));
    if (P >= 2) GH_HIP(hipStreamWaitEvent(sp, s->ev_w[P - 2], 0));          // (whichever stream the last wide update ran on)
    s->tail = sp;
    return GH_OK;
  }
  // (the trailing updates ran on the main stream itself -- large matrices -- or the old arm: the main stream joins)
  GH_HIP(hipEventRecord(s->ev_sync[1], sp));
  GH_HIP(hipStreamWaitEvent(s->st, s->ev_sync[1], 0));
  GH_HIP(hipEventRecord(s->ev_sync[2], sn));
  GH_HIP(hipStreamWaitEvent(s->st, s->ev_sync[2], 0));
  if (sm != s->st) {
    GH_HIP(hipEventRecord(s->ev_xfer, sm));
    GH_HIP(hipStreamWaitEvent(s->st, s->ev_xfer, 0));
  }
  return GH_OK;
}

// ---- the two-level driver: inner panels for the chain, groups of them for the trailing update (gh_chol_plan.h)
// The maximum number of inner panels per group; 1 = the one-level driver above, launch for launch.
#ifndef GH_UPDATE_GROUP_DEFAULT
#define GH_UPDATE_GROUP_DEFAULT 2
#endif
static int g_update_group = GH_UPDATE_GROUP_DEFAULT;
extern "C" int gh_debug_set_update_group(int gmax) {
  const int prev = g_update_group;
  g_update_group = gmax < 1 ? GH_UPDATE_GROUP_DEFAULT : gmax;
  return prev;
}
static double g_update_hide = GH_PLAN_HIDE;
extern "C" double gh_debug_set_update_hide(double hide) {
  const double prev = g_update_hide;
  g_update_hide = hide > 0.0 ? hide : GH_PLAN_HIDE;
  return prev;
}
extern "C" int gh_debug_chol_plan(int64_t np, int64_t nb, int64_t bound, int32_t gmax, double hide, int64_t* panel_starts_out, int32_t max_starts,
                                  int32_t* n_starts, int64_t* ops_out, int32_t max_ops, int32_t* n_ops, int32_t* n_events) {
  if (np <= 0 || nb <= 0 || np % T || nb % T || gmax < 1 || !n_starts || !n_ops || (max_starts > 0 && !panel_starts_out) || (max_ops > 0 && !ops_out)) {
    gh_set_error("chol_plan: Np and nb must be positive multiples of 128, the group maximum at least 1");
    return GH_ERR_BAD_ARG;
  }
  const GhCholPlan pl = gh_plan_build(np, gh_plan_panel_starts(np, nb, bound), gmax, hide);
  *n_starts = (int32_t)pl.pc.size();
  *n_ops = (int32_t)pl.ops.size();
  if (n_events) *n_events = pl.n_events;
  for (int32_t i = 0; i < *n_starts && i < max_starts; ++i) panel_starts_out[i] = pl.pc[i];
  for (int32_t i = 0; i < *n_ops && i < max_ops; ++i) {
    const GhPlanOp& o = pl.ops[i];
    const int64_t row[GH_PLAN_COLS] = {o.kind, o.stream, o.r0, o.r1, o.c0, o.c1, o.k0, o.k1, o.wait0, o.wait1, o.record, o.lower};
    memcpy(ops_out + (size_t)i * GH_PLAN_COLS, row, sizeof(row));
  }
  return GH_OK;
}
// Executes the list: nothing here decides an order.  Only where the trailing updates run on the unmasked main stream
// (Np >= 24576); the remarks in factor_lookahead_deep on where barrier packets may sit hold: the main stream's only waits
// are F(G)'s for the event of its group's last panel -- the kind W(j) has -- and the join at its end.
static int factor_two_level(gh_chol* s) {
  hipStream_t sm = s->st, sp = s->st2;
  const std::vector<int64_t> pc = panel_starts(s);
  if (s->plan.np != s->np || s->plan.gmax != g_update_group || s->plan.hide != g_update_hide || s->plan.pc != pc)
    s->plan = gh_plan_build(s->np, pc, g_update_group, g_update_hide);
  const GhCholPlan& pl = s->plan;
  while ((int)s->ev_plan.size() < pl.n_events) {
    hipEvent_t e;
    GH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    s->ev_plan.push_back(e);
  }
  double* A = s->A.d();
  const int64_t ld = s->np;
  const bool prof = s->opts.profile != 0;
  if (!s->build_on_chain) {                              // everything queued so far (the build, on s->st) before the chain starts
    GH_HIP(hipEventRecord(s->ev_sync[0], s->st));
    GH_HIP(hipStreamWaitEvent(sp, s->ev_sync[0], 0));
    GH_HIP(hipStreamWaitEvent(s->st3, s->ev_sync[0], 0));
  }
  for (const GhPlanOp& o : pl.ops) {
    hipStream_t st = o.stream == GH_PLAN_MAIN ? sm : sp;
    if (o.wait0 >= 0) GH_HIP(hipStreamWaitEvent(st, s->ev_plan[o.wait0], 0));
    if (o.wait1 >= 0) GH_HIP(hipStreamWaitEvent(st, s->ev_plan[o.wait1], 0));
    if (o.kind == GH_PLAN_PANEL) {
      const long ep = prof ? s->next_ev() : -1;
      if (ep >= 0) { GH_HIP(hipEventRecord(s->ev_pool[ep].a, st)); s->ev_panel.push_back((size_t)ep); }
      GH_CHECK(panel_step(s, st, o.c0, o.c1 - o.c0));
      if (ep >= 0) GH_HIP(hipEventRecord(s->ev_pool[ep].b, st));
    } else if (o.kind != GH_PLAN_JOIN) {
      const int64_t m = o.r1 - o.r0, n = o.c1 - o.c0, k = o.k1 - o.k0;
      // (algorithmic flops: the lower tiles only, with the K of this launch -- as the one-level driver counts its block columns)
      const double fl = gh_plan_trap_tiles(m, n) * 2.0 * T * T * (double)k;
      const long eu = prof ? s->next_ev() : -1;
      if (eu >= 0) {
        GH_HIP(hipEventRecord(s->ev_pool[eu].a, st));
        s->ev_update.push_back((size_t)eu); s->ev_update_flops.push_back(fl);
        if (o.kind == GH_PLAN_F) s->ev_trailing.push_back((size_t)eu);
      }
      GH_CHECK(gh_gemm_nt(st, blk(A, ld, o.r0, o.c0), ld, blk(A, ld, o.r0, o.k0), ld, blk(A, ld, o.c0, o.k0), ld, m, n, k, -1.0, 1.0, o.lower != 0));
      if (eu >= 0) GH_HIP(hipEventRecord(s->ev_pool[eu].b, st));
      s->prof.update_flops += fl;
      if (o.kind == GH_PLAN_F) { s->prof.trailing_flops += fl; s->prof.n_trailing += 1; }
    }
    if (o.record >= 0) GH_HIP(hipEventRecord(s->ev_plan[o.record], st));
  }
  return GH_OK;                                          // (the JOIN op left everything ordered on the main stream: s->tail stays s->st)
}

#ifndef GH_LOOKAHEAD_DEPTH
#define GH_LOOKAHEAD_DEPTH 1
#endif
static int lookahead_depth(const gh_chol* s) {
  // depth 1 in this formulation (block column j+1 updated on the chain stream itself, the wide SYRK
  // alone on the main stream) beats the older scheme (block column on the main stream, depth "0") by
  // 7-12 % from N = 4096 to 16384 and is level with it above; deeper windows lose (size sweep in
  // profiles/r02/lookahead_depth_sweep.md): the narrow GEMMs of the window compete with the potf2 chain.
  // (-DGH_LOOKAHEAD_DEPTH=<d> builds the deeper windows for an A/B; an environment switch until round 5)
  return GH_LOOKAHEAD_DEPTH;
}

static int factor(gh_chol* s) {
  SmallLdsGuard guard(s->opts.lookahead && s->st2 && trailing_stream(s) == s->st);       // no CUs kept free of the SYRK
  // (a matrix of ONE panel has nothing to look ahead to: on the main stream it saves the two cross-stream hand-overs,
  //  ~35 us each -- a tenth of the step at N = 1024)
  if (s->opts.lookahead && s->st2 && s->st3 && s->st4 && s->np > panel_width(s)) {      // (panel widths: panel_starts())
    if (g_update_group > 1 && lookahead_depth(s) == 1 && !use_simple_potf2() && trailing_stream(s) == s->st) return factor_two_level(s);
    return factor_lookahead_deep(s, lookahead_depth(s));
  }
  hipStream_t st = s->st;
  double* A = s->A.d();
  const int64_t np = s->np, ld = np;
  const bool prof = s->opts.profile != 0;
  const std::vector<int64_t> pc = panel_starts(s);             // (the same panel widths as the look-ahead schedule)
  for (size_t pj = 0; pj + 1 < pc.size(); ++pj) {
    const int64_t k0 = pc[pj], nb = pc[pj + 1] - pc[pj];
    const long ep = prof ? s->next_ev() : -1;
    if (ep >= 0) { GH_HIP(hipEventRecord(s->ev_pool[ep].a, st)); s->ev_panel.push_back((size_t)ep); }
    GH_CHECK(gh_chol_potrf_block(st, blk(A, ld, k0, k0), ld, nb, s->dinv.d() + (k0 / T) * T * T, s->d_info, k0));
    const int64_t m = np - (k0 + nb);
    if (m > 0)
      GH_CHECK(trsm_right(st, blk(A, ld, k0, k0), ld, s->dinv.d() + (k0 / T) * T * T, blk(A, ld, k0 + nb, k0), ld, m, nb));
    if (ep >= 0) GH_HIP(hipEventRecord(s->ev_pool[ep].b, st));
    if (m > 0) {
      const long et = prof ? s->next_ev() : -1;
      if (et >= 0) { GH_HIP(hipEventRecord(s->ev_pool[et].a, st)); s->ev_trailing.push_back((size_t)et); }
      const double* P = blk(A, ld, k0 + nb, k0);
      GH_CHECK(gh_gemm_nt(st, blk(A, ld, k0 + nb, k0 + nb), ld, P, ld, P, ld, m, m, nb, -1.0, 1.0, true));
      if (et >= 0) GH_HIP(hipEventRecord(s->ev_pool[et].b, st));
      const double tiles = (double)(m / T) * (m / T + 1) / 2.0;
      s->prof.trailing_flops += tiles * 2.0 * T * T * (double)nb;
      s->prof.n_trailing += 1;
    }
  }
  return GH_OK;
}

// x, yerr into the handle's copies and the failure word cleared, ONE launch (device-resident inputs: as two copies
// and a memset these were three runtime operations with 5-30 us between them -- a tenth of a step at N = 1024)
__global__ void prep_inputs_kernel(const double* xs, long nx, const double* es, long ne, double* xd, double* ed, long long* info) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  for (long e = i; e < nx; e += stride) xd[e] = xs[e];
  for (long e = i; e < ne; e += stride) ed[e] = es[e];
  if (i == 0) *info = 0;
}

// Everything of compute() up to and including the log-det launch, enqueued on s->st without a
// host synchronisation; gh_chol_compute_finish() takes the scalars read back.
int gh_chol_compute_enqueue(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr, ComputeCtx& c) {
  if (!s || !k || !x || !yerr || n <= 0) { gh_set_error("bad argument to compute"); return GH_ERR_BAD_ARG; }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  GH_CHECK(gh_chol_set_device(s));
  GH_CHECK(k->upload());
  s->computed = false;
  s->info = 0;
  const int64_t np = gh_round_up(n, T);
  s->n = n; s->np = np; s->ndim = ndim; s->have_yerr = true;
  GH_CHECK(s->A.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(s->dinv.ensure((size_t)(np / T) * T * T * sizeof(double)));
  GH_CHECK(s->x.ensure((size_t)n * ndim * sizeof(double)));
  GH_CHECK(s->yerr.ensure((size_t)n * sizeof(double)));
  GH_CHECK(s->scal.ensure(256 * sizeof(double)));      // [0] log-det, [1] quadratic form, [8..72) and [72..136) slice sums
  // With look-ahead the first thing that needs the matrix is the chain stream's first panel: inputs and kernel-matrix build go to
  // THAT stream (everything else waits for panel events that follow them in its order) instead of the main stream + a
  // cross-stream hand-over -- 19 us between the build and the first potf2 of every compute() (profiles/r06/: N = 2048 timeline).
  s->build_on_chain = g_build_on_chain && s->opts.lookahead && s->st2 && s->st3 && s->st4 && np > panel_width(s);
  hipStream_t st = s->build_on_chain ? s->st2 : s->st;
  memset(&s->prof, 0, sizeof(s->prof));
  s->ev_used = 0; s->ev_trailing.clear(); s->ev_panel.clear(); s->ev_update.clear(); s->ev_update_flops.clear();
  const bool prof = s->opts.profile != 0;
  c.e_all = prof ? s->next_ev() : -1;
  c.e_build = prof ? s->next_ev() : -1;
  if (c.e_all >= 0) GH_HIP(hipEventRecord(s->ev_pool[c.e_all].a, st));
  s->d_info = (long long*)(s->scal.d() + 2);            // beside log-det [0] and quadratic form [1]: ONE copy brings them back
  if (gh_is_device_ptr(x) && gh_is_device_ptr(yerr)) {
    const long tot = (long)n * ndim;
    hipLaunchKernelGGL(prep_inputs_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 1024)), dim3(256), 0, st,
                       x, tot, yerr, (long)n, s->x.d(), s->yerr.d(), s->d_info);
    GH_HIP(hipGetLastError());
  } else {
    GH_CHECK(gh_to_device(s->x.d(), x, (size_t)n * ndim, st));
    GH_CHECK(gh_to_device(s->yerr.d(), yerr, (size_t)n, st));
    GH_HIP(hipMemsetAsync(s->d_info, 0, sizeof(long long), st));
  }
  if (c.e_build >= 0) GH_HIP(hipEventRecord(s->ev_pool[c.e_build].a, st));
  GH_CHECK(gh_launch_kmat(k, s->x.d(), n, s->x.d(), n, s->yerr.d(), s->A.d(), np, np, np, 0, 0, true, true, st));
  if (c.e_build >= 0) GH_HIP(hipEventRecord(s->ev_pool[c.e_build].b, st));
  s->tail = s->st;
  GH_CHECK(factor(s));                                  // (may move s->tail to the chain stream)
  GH_CHECK(gh_launch_logdet(s->A.d(), np, np, s->scal.d(), s->scal.d() + 8, s->tail));
  if (c.e_all >= 0) GH_HIP(hipEventRecord(s->ev_pool[c.e_all].b, s->tail));
  return GH_OK;
}
// after the stream has been synchronised and logdet / info copied to the host
int gh_chol_compute_finish(gh_chol* s, const ComputeCtx& c, double ld_host, long long info_host, double* logdet_out) {
  if (s->opts.profile && c.e_all >= 0 && c.e_build >= 0) {
    float ms = 0;
    GH_HIP(hipEventElapsedTime(&ms, s->ev_pool[c.e_all].a, s->ev_pool[c.e_all].b)); s->prof.ms_total = ms;
    GH_HIP(hipEventElapsedTime(&ms, s->ev_pool[c.e_build].a, s->ev_pool[c.e_build].b)); s->prof.ms_build = ms;
    for (size_t i : s->ev_trailing) { GH_HIP(hipEventElapsedTime(&ms, s->ev_pool[i].a, s->ev_pool[i].b)); s->prof.ms_trailing += ms; }
    // time during which ANY trailing-update launch (wide SYRK on the main stream, block-column GEMM on the
    // chain stream) was running: union of their event intervals, measured from the start of compute()
    if (!s->ev_update.empty()) {
      std::vector<std::pair<float, float>> iv;
      s->upd_intervals.clear();
      for (size_t q = 0; q < s->ev_update.size(); ++q) {
        const size_t i = s->ev_update[q];
        float a = 0, b = 0;
        GH_HIP(hipEventElapsedTime(&a, s->ev_pool[c.e_all].a, s->ev_pool[i].a));
        GH_HIP(hipEventElapsedTime(&b, s->ev_pool[c.e_all].a, s->ev_pool[i].b));
        iv.emplace_back(a, b);
        s->upd_intervals.push_back(a); s->upd_intervals.push_back(b);
        s->upd_intervals.push_back(q < s->ev_update_flops.size() ? s->ev_update_flops[q] : 0.0);
      }
      std::sort(iv.begin(), iv.end());
      double tot = 0.0;
      float lo = iv[0].first, hi = iv[0].second;
      for (size_t q = 1; q < iv.size(); ++q) {
        if (iv[q].first > hi) { tot += hi - lo; lo = iv[q].first; hi = iv[q].second; }
        else if (iv[q].second > hi) hi = iv[q].second;
      }
      tot += hi - lo;
      s->prof.ms_update_union = tot;
    }
    for (size_t i : s->ev_panel) { GH_HIP(hipEventElapsedTime(&ms, s->ev_pool[i].a, s->ev_pool[i].b)); s->prof.ms_panel += ms; }
  }
  if (info_host != 0) {
    s->info = info_host;
    gh_set_error("%lld-th leading minor of the array is not positive definite", info_host);
    return GH_ERR_NOT_PD;
  }
  s->logdet = ld_host;
  s->computed = true;
  if (logdet_out) *logdet_out = ld_host;
  return GH_OK;
}

extern "C" int gh_chol_compute(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                               const double* yerr, double* logdet_out) {
  ComputeCtx c;
  GH_CHECK(gh_chol_compute_enqueue(s, k, x, n, ndim, yerr, c));
  hipStream_t st = s->tail;                             // (the stream the factorisation ended on: gh_chol_compute_enqueue)
  double back[3] = {0.0, 0.0, 0.0};                     // [0] log-det, [1] (quadratic form), [2] the failure word's bits
  GH_CHECK(read_scalars(s, back, 3, st));
  GH_HIP(hipStreamSynchronize(st));
  return gh_chol_compute_finish(s, c, back[0], info_from_bits(back[2]), logdet_out);
}

int gh_chol_need_computed(gh_chol* s) {
  if (!s) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!s->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  return gh_chol_set_device(s);
}

extern "C" void gh_chol_release_buffers(gh_chol* s) {
  // frees everything but the handle itself (streams, events); the next compute() re-allocates
  if (!s) return;
  (void)hipSetDevice(s->opts.device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  s->computed = false;
  for (GhBuf* b : {&s->A, &s->A_spare, &s->dinv, &s->x, &s->yerr, &s->v0, &s->v1, &s->v2, &s->rhs, &s->work, &s->work2, &s->scratch, &s->chain, &s->lv, &s->samp, &s->fish, &s->lgo}) b->release();
  gh_batch_free(s->batch);
  s->batch = nullptr;
}
extern "C" void gh_chol_trim(gh_chol* s) {
  // frees the transient N x N / N x M work buffers of predict / grad / get_inverse, keeps the factor
  if (!s) return;
  (void)hipSetDevice(s->opts.device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  for (GhBuf* b : {&s->rhs, &s->work, &s->work2, &s->scratch, &s->A_spare, &s->samp, &s->fish, &s->lgo}) b->release();
  gh_batch_free(s->batch);
  s->batch = nullptr;
}

