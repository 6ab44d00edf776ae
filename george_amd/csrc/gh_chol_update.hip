// gh_chol_update.hip -- the dense solver, moving and editing a computed factor: export / import, append / truncate / set_yerr,
// remove.  (gh_chol.hip makes the factor, gh_chol_solve.hip works on it; what they share is in gh_chol_impl.h.)
#include <math.h>
#include "gh_chol_impl.h"
#include "gh_gemm_tile.h"
#include "../../include/george_amd_debug.h"

// ============================================================ factor export / import
// The reference's BasicSolver survives pickling COMPUTED (tests/test_pickle.py:21-36: its factor is a
// NumPy array).  Here the factor lives in HBM, so it is packed on the device -- row i of the lower
// triangle at offset i (i + 1) / 2, N (N + 1) / 2 doubles -- and copied out, together with the
// inverses of the 128 x 128 diagonal blocks (Np / 128 x 128 x 128) that every solve multiplies by.
__global__ void pack_lower_kernel(const double* A, long ld, long n, double* out) {
  const long i = blockIdx.x;
  const double* row = A + i * ld;
  double* o = out + i * (i + 1) / 2;
  for (long j = threadIdx.x; j <= i; j += blockDim.x) o[j] = row[j];
}
__global__ void unpack_lower_kernel(const double* in, long n, double* A, long ld, long np) {
  const long i = blockIdx.x;                     // row of the padded matrix
  double* row = A + i * ld;
  if (i < n) {
    const double* src = in + i * (i + 1) / 2;
    for (long j = threadIdx.x; j < np; j += blockDim.x) row[j] = (j <= i) ? src[j] : 0.0;
  } else {
    for (long j = threadIdx.x; j < np; j += blockDim.x) row[j] = (j == i) ? 1.0 : 0.0;      // identity padding
  }
}
extern "C" int64_t gh_chol_factor_size(const gh_chol* s) { return s ? s->n * (s->n + 1) / 2 : 0; }
extern "C" int64_t gh_chol_dinv_size(const gh_chol* s) { return s ? (s->np / T) * T * T : 0; }
extern "C" int gh_chol_export_factor(gh_chol* s, double* packed_lower, double* dinv_out) {
  GH_CHECK(gh_chol_need_computed(s));
  if (!packed_lower || !dinv_out) { gh_set_error("null output"); return GH_ERR_BAD_ARG; }
  const int64_t n = s->n, np = s->np;
  const size_t cnt = (size_t)n * (n + 1) / 2;
  GH_CHECK(s->work.ensure(cnt * sizeof(double)));
  hipLaunchKernelGGL(pack_lower_kernel, dim3((unsigned)n), dim3(256), 0, s->st, s->A.d(), (long)np, (long)n, s->work.d());
  GH_HIP(hipGetLastError());
  GH_CHECK(gh_from_device(packed_lower, s->work.d(), cnt, s->st));
  GH_CHECK(gh_from_device(dinv_out, s->dinv.d(), (size_t)(np / T) * T * T, s->st));
  GH_HIP(hipStreamSynchronize(s->st));
  return GH_OK;
}
extern "C" int gh_chol_import_factor(gh_chol* s, int64_t n, int32_t ndim, const double* x, const double* packed_lower,
                                     const double* dinv_in, double logdet) {
  if (!s || n <= 0 || ndim <= 0 || !x || !packed_lower || !dinv_in) { gh_set_error("bad argument to import_factor"); return GH_ERR_BAD_ARG; }
  GH_CHECK(gh_chol_set_device(s));
  s->computed = false;
  const int64_t np = gh_round_up(n, T);
  s->n = n; s->np = np; s->ndim = ndim; s->info = 0; s->have_yerr = false;
  const size_t cnt = (size_t)n * (n + 1) / 2;
  GH_CHECK(s->A.ensure((size_t)np * np * sizeof(double)));
  GH_CHECK(s->dinv.ensure((size_t)(np / T) * T * T * sizeof(double)));
  GH_CHECK(s->x.ensure((size_t)n * ndim * sizeof(double)));
  GH_CHECK(s->scal.ensure(256 * sizeof(double)));
  GH_CHECK(s->work.ensure(cnt * sizeof(double)));
  GH_CHECK(gh_to_device(s->x.d(), x, (size_t)n * ndim, s->st));
  GH_CHECK(gh_to_device(s->work.d(), packed_lower, cnt, s->st));
  GH_CHECK(gh_to_device(s->dinv.d(), dinv_in, (size_t)(np / T) * T * T, s->st));
  hipLaunchKernelGGL(unpack_lower_kernel, dim3((unsigned)np), dim3(256), 0, s->st, s->work.d(), (long)n, s->A.d(), (long)np, (long)np);
  GH_HIP(hipGetLastError());
  GH_HIP(hipStreamSynchronize(s->st));
  s->logdet = logdet;
  s->computed = true;
  return GH_OK;
}

// ============================================================ append / truncate
// Sequential use: the data set gains (or loses) a few trailing points and the factor is kept.  With n = n0 + t, n0 = 128 * (n / 128):
//   * a Cholesky factor's leading rows do not depend on later rows: the n0 x n0 part of L and its diagonal-block inverses stay as they
//     are -- in place while the new points fit into the last partial tile, re-laid into buffers of the new Np (leading dimension = Np
//     throughout the solver) when the tile count grows;
//   * the new rows against the full tiles, X = K(x_new, x[:n0]) L00^-T: a row of X is the result of one forward sweep over L00 with
//     a row of the cross-covariance as its right-hand side -- contiguous, where the chained sweep kernels write it;
//   * the tail block, rows and columns [n0, n + m) padded to 128: S = K(tail, tail) + diag(yerr^2) - L_tail,0 L_tail,0^T, then
//     potrf_block.  The product has K = n0 and one or a few output tiles: split over K (tail_syrk_splitk_kernel), summed in a fixed
//     order.  The t old tail rows of the diagonal tile are formed again (last bits may differ from what compute() left there).
// DESIGN.md, "Appending points".
static int g_append_path = 0;
extern "C" int gh_debug_set_append_path(int path) {
  const int prev = g_append_path;
  g_append_path = (path >= 1 && path <= 3) ? path : 0;
  return prev;
}
// new rows up to which the chained sweeps (4 rows per pass over the factor) are taken; above, the blocked substitution, whose time does
// not depend on m up to 128.  Measured (profiles/append/append_paths.json) at n = 4032 / 16320: the substitution 0.75 / 3.3 ms; the
// sweeps 0.48 / 1.5 ms at m = 4 and 1.36 / 5.1 ms at m = 16, so about 0.77 / 2.7 ms at 8 and 1.07 / 3.9 ms at 12 (interpolated).
#define GH_APPEND_MULTI_MAX 8

static void swap_bufs(GhBuf& a, GhBuf& b) { std::swap(a.p, b.p); std::swap(a.bytes, b.bytes); std::swap(a.pooled, b.pooled); }

// Where a factor of np2 rows moves to.  Allocating it per call is what a move costs: hipMalloc + hipFree of 34 GB took 960 ms of a 971-ms
// append at N = 65536 (profiles/append/append_paths.json), the copy 6.5 ms.  So the handle keeps the buffer the factor left at its last
// move (A_spare) and the next move goes there; when that is too small the new one gets room for np2 / 32 (at least 1024) more rows, which
// the next 8 or more tile crossings find large enough.  A buffer of more rows holds a matrix of fewer: the leading dimension is Np.
static int take_factor_buffer(gh_chol* s, GhBuf& out, int64_t np2) {
  const size_t need = (size_t)np2 * np2 * sizeof(double);
  if (s->A_spare.p && s->A_spare.bytes >= need) { swap_bufs(out, s->A_spare); return GH_OK; }
  const int64_t cap = np2 + std::max<int64_t>(1024, gh_round_up(np2 / 32, T));
  if (out.ensure((size_t)cap * cap * sizeof(double)) == GH_OK) return GH_OK;
  return out.ensure(need);
}
// the lower 128-tiles of dst (nn x nn, nn a multiple of 128): src where row and column are below nvalid, identity elsewhere
__global__ __launch_bounds__(256) void relayout_lower_kernel(const double* src, long lds, long nvalid, double* dst, long ldd) {
  const long i = blockIdx.x, jend = (i / T + 1) * T;
  const double* sr = src + i * lds;
  double* dr = dst + i * ldd;
  if (i < nvalid) {
    for (long j = threadIdx.x; j < jend; j += 256) dr[j] = (j < nvalid) ? sr[j] : 0.0;
  } else {
    for (long j = threadIdx.x; j < jend; j += 256) dr[j] = (j == i) ? 1.0 : 0.0;
  }
}
// The last tile row of A (rows [t0, t0 + 128), one per workgroup) cut to n_keep points: rows from n_keep on become identity padding
// (columns up to the end of the diagonal tile), and the kept rows lose columns n_keep .. of the diagonal tile (zeros already, as
// potf2 leaves the strict upper triangle: written all the same, so that the tile is what compute() at n_keep builds).
__global__ __launch_bounds__(256) void pad_rows_kernel(double* A, long ld, long t0, long n_keep) {
  const long i = t0 + blockIdx.x, jend = t0 + T;
  double* r = A + i * ld;
  if (i >= n_keep) { for (long j = threadIdx.x; j < jend; j += 256) r[j] = (j == i) ? 1.0 : 0.0; }
  else { for (long j = n_keep + threadIdx.x; j < jend; j += 256) r[j] = 0.0; }
}
// a 128 x 128 diagonal-block inverse cut to its leading keep x keep part, identity behind it
__global__ __launch_bounds__(256) void dinv_clip_kernel(double* d, int keep) {
  for (int idx = threadIdx.x; idx < T * T; idx += 256) {
    const int i = idx >> 7, j = idx & 127;
    if (i >= keep || j >= keep) d[idx] = (i == j) ? 1.0 : 0.0;
  }
}
// Split-K stage 1 of Lt Lt^T (Lt: 128 * tiles rows, k contiguous, K = ktot): workgroup (p, sl) forms the 128 x 128 tile p of the
// lower triangle over the k-slice sl -- the dense solver's tile function -- into part[sl][p].  Stage 2 adds the slices in index order
// and subtracts the total from S: bitwise reproducible, like the log-det and the dot product.
__global__ __launch_bounds__(256, 2) void tail_syrk_splitk_kernel(const double* Lt, long ld, long kslice, long ktot, double* part) {
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  const long k0 = (long)blockIdx.y * kslice;
  const long K = kslice < ktot - k0 ? kslice : ktot - k0;
  double* C = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * T * T;
  gh_tile128_nt_sp<false>(sm, C, T, Lt + (long)ti * T * ld + k0, ld, Lt + (long)tj * T * ld + k0, ld, K);
}
__global__ __launch_bounds__(256) void tail_syrk_reduce_kernel(double* S, long ld, const double* part, int nslice) {
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  const long npairs = gridDim.x;
  for (int idx = blockIdx.y * 256 + threadIdx.x; idx < T * T; idx += gridDim.y * 256) {
    double acc = 0.0;
    for (int sl = 0; sl < nslice; ++sl) acc += part[((long)sl * npairs + blockIdx.x) * T * T + idx];
    S[((long)ti * T + (idx >> 7)) * ld + (long)tj * T + (idx & 127)] -= acc;
  }
}

// X (mr x n0, ld = ldx, mr a multiple of 128) <- X L00^-T, right-looking in row form on the matrix pipe: X_j <- X_j L_jj^-T with the
// stored inverse, then X[:, j+1:] -= X_j L[j+1:, j]^T -- inside super-blocks of 8 tiles, and ONE K = 1024 update of everything right
// of a super-block (as trsm_multi).  Every product has both operands k-major; the update is as wide as what is left of the row.
static int append_trsm_rows(hipStream_t st, const double* L, int64_t ld, const double* dinv, double* X, int64_t ldx, int64_t mr, int64_t nt0) {
  const int64_t SB = 8;
  for (int64_t J = 0; J < nt0; J += SB) {
    const int64_t Je = std::min<int64_t>(J + SB, nt0);
    for (int64_t j = J; j < Je; ++j) {
      double* Xj = X + j * T;
      GH_CHECK(gh_gemm_nt(st, Xj, ldx, Xj, ldx, dinv + j * T * T, T, mr, T, T, 1.0, 0.0, false));
      if (j + 1 < Je)
        GH_CHECK(gh_gemm_nt(st, X + (j + 1) * T, ldx, Xj, ldx, L + (j + 1) * T * ld + j * T, ld, mr, (Je - j - 1) * T, T, -1.0, 1.0, false));
    }
    if (Je < nt0)
      GH_CHECK(gh_gemm_nt(st, X + Je * T, ldx, X + J * T, ldx, L + Je * T * ld + J * T, ld, mr, (nt0 - Je) * T, (Je - J) * T, -1.0, 1.0, false));
  }
  return GH_OK;
}

extern "C" int gh_chol_append(gh_chol* s, gh_kernel* k, const double* x_new, int64_t m, const double* yerr_new, double* logdet_out) {
  if (!s || !k || !x_new || !yerr_new || m <= 0) { gh_set_error("bad argument to append"); return GH_ERR_BAD_ARG; }
  GH_CHECK(gh_chol_need_computed(s));
  if (k->ndim != s->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  // (the old rows of the last, partial tile are formed again from the kernel and the error bars)
  if (!s->have_yerr) { gh_set_error("append: the handle was rebuilt by import_factor and holds no error bars (gh_chol_set_yerr)"); return GH_ERR_BAD_ARG; }
  GH_CHECK(k->upload());
  const int64_t n = s->n, np = s->np, ndim = s->ndim, n2 = n + m, np2 = gh_round_up(n2, T);
  const int64_t n0 = (n / T) * T, nt0 = n0 / T, tailp = np2 - n0, tt = tailp / T;
  const bool grow = np2 > np;
  const int path = nt0 == 0 ? 0 : g_append_path ? g_append_path : (m <= GH_APPEND_MULTI_MAX ? 2 : 3);
  hipStream_t st = s->st;
  // ---- every allocation first: a failure up to here leaves the handle as it was
  GhBuf A2, dinv2, x2, yerr2;
  GhPooledBuf saved, part;
  if (grow) {
    GH_CHECK(take_factor_buffer(s, A2, np2));
    GH_CHECK(dinv2.ensure((size_t)(np2 / T) * T * T * sizeof(double)));
  } else {
    GH_CHECK(saved.ensure((size_t)2 * T * T * sizeof(double)));
  }
  const bool grow_x = s->x.bytes < (size_t)n2 * ndim * sizeof(double) || s->yerr.bytes < (size_t)n2 * sizeof(double);
  if (grow_x) {
    GH_CHECK(x2.ensure((size_t)np2 * ndim * sizeof(double)));
    GH_CHECK(yerr2.ensure((size_t)np2 * sizeof(double)));
  }
  const int64_t mr = path == 3 ? gh_round_up(m, T) : m;
  if (nt0 > 0) GH_CHECK(s->work.ensure((size_t)mr * n0 * sizeof(double)));
  const int64_t npairs = tt * (tt + 1) / 2;
  // k-slices in units of 128: as many workgroups as keep the chip busy, at most 256 slices
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(256, 2048 / npairs));
  const int64_t ktiles = nt0 > 0 ? (nt0 + want - 1) / want : 0, nslice = nt0 > 0 ? (nt0 + ktiles - 1) / ktiles : 0;
  if (nt0 > 0) GH_CHECK(part.ensure((size_t)nslice * npairs * T * T * sizeof(double)));
  GH_CHECK(chain_ensure(s, np2 / T));
  GH_CHECK(s->scal.ensure(256 * sizeof(double)));
  int* fail = append_fail(s);
  s->d_info = (long long*)(s->scal.d() + 2);
  // ---- inputs
  double* xd = grow_x ? x2.d() : s->x.d();
  double* yd = grow_x ? yerr2.d() : s->yerr.d();
  if (grow_x) {
    GH_HIP(hipMemcpyAsync(xd, s->x.d(), (size_t)n * ndim * sizeof(double), hipMemcpyDeviceToDevice, st));
    GH_HIP(hipMemcpyAsync(yd, s->yerr.d(), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  GH_CHECK(gh_to_device(xd + n * ndim, x_new, (size_t)m * ndim, st));
  GH_CHECK(gh_to_device(yd + n, yerr_new, (size_t)m, st));
  GH_HIP(hipMemsetAsync(s->d_info, 0, sizeof(long long), st));
  GH_HIP(hipMemsetAsync(fail, 0, sizeof(int), st));
  // ---- 1. grow (or save what is overwritten in place)
  double* Ad = grow ? A2.d() : s->A.d();
  double* dd = grow ? dinv2.d() : s->dinv.d();
  const int64_t ld = grow ? np2 : np;
  s->prof.ms_append_relayout = 0.0;
  // From here on the in-place case writes into the handle's own factor.  GH_ERR_NOT_PD and a sweep time-out put the old bits back; any
  // other error return (a failed HIP call) leaves the tail tile half written, and the handle NOT computed.
  struct Dirty { gh_chol* s; bool armed; ~Dirty() { if (armed) s->computed = false; } } dirty{s, false};
  long e_lay = -1;                                        // (profile: the relayout's share, gh_chol_profile.ms_append_relayout)
  if (grow && s->opts.profile) {                          // (events of its own: the pool belongs to the last compute()'s profile)
    for (auto& e : s->ev_lay) if (!e) GH_HIP(hipEventCreate(&e));
    e_lay = 0;
  }
  if (e_lay >= 0) GH_HIP(hipEventRecord(s->ev_lay[0], st));
  if (grow) {
    hipLaunchKernelGGL(relayout_lower_kernel, dim3((unsigned)np2), dim3(256), 0, st, s->A.d(), (long)np, (long)np, Ad, (long)ld);
    GH_HIP(hipGetLastError());
    GH_HIP(hipMemcpyAsync(dd, s->dinv.d(), (size_t)(np / T) * T * T * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (e_lay >= 0) GH_HIP(hipEventRecord(s->ev_lay[1], st));
  } else {
    dirty.armed = true;
    GH_HIP(hipMemcpy2DAsync(saved.d(), T * sizeof(double), Ad + n0 * ld + n0, ld * sizeof(double), T * sizeof(double), T, hipMemcpyDeviceToDevice, st));
    GH_HIP(hipMemcpyAsync(saved.d() + T * T, dd + nt0 * T * T, (size_t)T * T * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  // ---- 2. the new rows against the full tiles
  if (nt0 > 0) {
    double* Kc = s->work.d();
    GH_CHECK(gh_launch_kmat(k, xd + n * ndim, m, xd, n0, nullptr, Kc, n0, mr, n0, n, 0, true, false, st));
    if (path == 3) {
      GH_CHECK(append_trsm_rows(st, Ad, ld, dd, Kc, n0, mr, nt0));
      GH_HIP(hipMemcpy2DAsync(Ad + n * ld, ld * sizeof(double), Kc, n0 * sizeof(double), n0 * sizeof(double), m, hipMemcpyDeviceToDevice, st));
    } else {
      GH_HIP(hipMemset2DAsync(Ad + n * ld, ld * sizeof(double), 0xFF, n0 * sizeof(double), m, st));
      GH_CHECK(gh_launch_trsv_fwd_chain_rows(Ad, (long)ld, dd, nt0, Kc, (long)n0, Ad + n * ld, (long)ld, m, path == 2, fail, st));
    }
  }
  // ---- 3. the tail block
  double* S = Ad + n0 * ld + n0;
  GH_CHECK(gh_launch_kmat(k, xd + n0 * ndim, n2 - n0, xd + n0 * ndim, n2 - n0, yd + n0, S, ld, tailp, tailp, n0, n0, true, true, st));
  if (nt0 > 0) {
    hipLaunchKernelGGL(tail_syrk_splitk_kernel, dim3((unsigned)npairs, (unsigned)nslice), dim3(256), 0, st,
                       Ad + n0 * ld, (long)ld, (long)(ktiles * T), (long)n0, part.d());
    hipLaunchKernelGGL(tail_syrk_reduce_kernel, dim3((unsigned)npairs, 16), dim3(256), 0, st, S, (long)ld, part.d(), (int)nslice);
    GH_HIP(hipGetLastError());
  }
  GH_CHECK(gh_chol_potrf_block(st, S, ld, tailp, dd + nt0 * T * T, s->d_info, n0));
  // ---- 4. log-det over the whole diagonal; one synchronisation brings it back with the failure word and the sweeps' time-out flag
  GH_CHECK(gh_launch_logdet(Ad, (long)ld, (long)np2, s->scal.d(), s->scal.d() + 8, st));
  double back[3] = {0.0, 0.0, 0.0};
  int failed = 0;
  GH_CHECK(read_scalars(s, back, 3, st));
  GH_HIP(hipMemcpyAsync(&failed, fail, sizeof(int), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  const long long info_host = info_from_bits(back[2]);
  if (e_lay >= 0) { float ms = 0; GH_HIP(hipEventElapsedTime(&ms, s->ev_lay[0], s->ev_lay[1])); s->prof.ms_append_relayout = ms; }
  if (info_host != 0 || failed) {
    if (!grow) {                                          // put back what was overwritten in place: the old bits
      GH_HIP(hipMemcpy2DAsync(S, ld * sizeof(double), saved.d(), T * sizeof(double), T * sizeof(double), T, hipMemcpyDeviceToDevice, st));
      GH_HIP(hipMemcpyAsync(dd + nt0 * T * T, saved.d() + T * T, (size_t)T * T * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (nt0 > 0) GH_HIP(hipMemset2DAsync(Ad + n * ld, ld * sizeof(double), 0, n0 * sizeof(double), m, st));
    }
    GH_HIP(hipStreamSynchronize(st));                     // (the buffers of this call go back to the allocator on return)
    if (grow && !s->A_spare.p) swap_bufs(s->A_spare, A2);  // (... but not the large one)
    dirty.armed = false;
    GH_CHECK(gh_chain_timeout("append", failed != 0, false));
    s->info = info_host;
    gh_set_error("%lld-th leading minor of the array is not positive definite", info_host);
    return GH_ERR_NOT_PD;
  }
  dirty.armed = false;
  if (grow) { swap_bufs(s->A, A2); swap_bufs(s->A_spare, A2); swap_bufs(s->dinv, dinv2); }   // (the old factor buffer is the spare now)
  if (grow_x) { swap_bufs(s->x, x2); swap_bufs(s->yerr, yerr2); }
  s->n = n2; s->np = np2; s->info = 0;
  s->logdet = back[0];
  if (logdet_out) *logdet_out = back[0];
  return GH_OK;
}

extern "C" int gh_chol_set_yerr(gh_chol* s, const double* yerr) {
  if (!s || !yerr) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  GH_CHECK(gh_chol_need_computed(s));
  GH_CHECK(s->yerr.ensure((size_t)s->np * sizeof(double)));
  GH_CHECK(gh_to_device(s->yerr.d(), yerr, (size_t)s->n, s->st));
  GH_HIP(hipStreamSynchronize(s->st));
  s->have_yerr = true;
  return GH_OK;
}

extern "C" int gh_chol_truncate(gh_chol* s, int64_t n_keep, double* logdet_out) {
  if (!s) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  GH_CHECK(gh_chol_need_computed(s));
  if (n_keep <= 0 || n_keep > s->n) { gh_set_error("truncate: n_keep must be in 1 .. %lld", (long long)s->n); return GH_ERR_BAD_ARG; }
  if (n_keep == s->n) { if (logdet_out) *logdet_out = s->logdet; return GH_OK; }
  const int64_t np = s->np, np2 = gh_round_up(n_keep, T);
  hipStream_t st = s->st;
  GhBuf A2, dinv2, x2, yerr2;
  GH_CHECK(s->scal.ensure(256 * sizeof(double)));
  if (np2 < np) {
    // fewer tiles: the leading dimension is Np, so the lower tiles move into a buffer of the new size -- and dinv, x and yerr with
    // them: the handle holds what it holds after an append that ended at this size
    const int64_t ndim = s->ndim;
    GH_CHECK(take_factor_buffer(s, A2, np2));
    GH_CHECK(dinv2.ensure((size_t)(np2 / T) * T * T * sizeof(double)));
    GH_CHECK(x2.ensure((size_t)np2 * ndim * sizeof(double)));
    if (s->have_yerr) GH_CHECK(yerr2.ensure((size_t)np2 * sizeof(double)));
    GH_HIP(hipMemcpyAsync(dinv2.d(), s->dinv.d(), (size_t)(np2 / T) * T * T * sizeof(double), hipMemcpyDeviceToDevice, st));
    GH_HIP(hipMemcpyAsync(x2.d(), s->x.d(), (size_t)n_keep * ndim * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (s->have_yerr) GH_HIP(hipMemcpyAsync(yerr2.d(), s->yerr.d(), (size_t)n_keep * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(relayout_lower_kernel, dim3((unsigned)np2), dim3(256), 0, st, s->A.d(), (long)np, (long)n_keep, A2.d(), (long)np2);
  } else if (np2 > n_keep) {
    // dropped rows in the same tile row: a leading principal block of L is the factor of that block of K
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)T), dim3(256), 0, st, s->A.d(), (long)np, (long)(np2 - T), (long)n_keep);
  }
  GH_HIP(hipGetLastError());
  if (n_keep % T) {                                       // ... and of a diagonal block's inverse the inverse of that block
    hipLaunchKernelGGL(dinv_clip_kernel, dim3(1), dim3(256), 0, st, (np2 < np ? dinv2.d() : s->dinv.d()) + (np2 / T - 1) * T * T, (int)(n_keep % T));
    GH_HIP(hipGetLastError());
  }
  const double* Ad = np2 < np ? A2.d() : s->A.d();
  GH_CHECK(gh_launch_logdet(Ad, (long)np2, (long)np2, s->scal.d(), s->scal.d() + 8, st));
  double ldv = 0.0;
  GH_HIP(hipMemcpyAsync(&ldv, s->scal.d(), sizeof(double), hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  if (np2 < np) {
    swap_bufs(s->A, A2); swap_bufs(s->A_spare, A2); swap_bufs(s->dinv, dinv2); swap_bufs(s->x, x2);
    if (s->have_yerr) swap_bufs(s->yerr, yerr2);
  }
  s->n = n_keep; s->np = np2; s->info = 0;
  s->logdet = ldv;
  if (logdet_out) *logdet_out = ldv;
  return GH_OK;
}

// ============================================================ removing points
// K[keep, keep] = L[keep, :] L[keep, :]^T = Lk Lk^T + W W^T with Lk = L[keep, keep] (lower triangular, positive diagonal) and
// W = L[keep, rem] (zero where keep[p] < rem[j]): taking points out is a rank-m Cholesky UPDATE of the gathered factor -- it adds a
// positive semi-definite term, so it cannot lose positive definiteness -- and rows before the first removed index do not change.
// Per pass of at most 128 columns of W and per diagonal tile j from the first affected one, with Wj the tile's rows of W:
//   V = Ljj^-1 Wj;   L' = chol(Ljj Ljj^T + Wj Wj^T) and L'^-1;   C C^T = I + V^T V and C^-1   (Ri = C^-T)
//   Q = [[Ljj^T L'^-T, -V Ri], [Wj^T L'^-T, Ri]]   (orthogonal);   [Lij' | Wi'] = [Lij | Wi] Q for every tile row i below j.
// The gathered tile has no stored inverse (it is a principal submatrix of old tiles), so V comes from a substitution.  Everything is
// written into buffers the handle does not use yet; they are swapped in after the one synchronisation has reported success.
// DESIGN.md section 4, "Removing points".
static int g_remove_path = 0;
extern "C" int gh_debug_set_remove_path(int path) {
  const int prev = g_remove_path;
  g_remove_path = (path == 1 || path == 2) ? path : 0;
  return prev;
}
// the argument rule of gh_chol_remove for a factor of n points: host code, no handle and no device needed
extern "C" int gh_debug_check_remove_args(int64_t n, const int64_t* idx, int64_t m) {
  if (!idx) { gh_set_error("remove: null index array"); return GH_ERR_BAD_ARG; }
  if (m <= 0 || m >= n) { gh_set_error("remove: the number of removed points must be in 1 .. %lld", (long long)(n - 1)); return GH_ERR_BAD_ARG; }
  for (int64_t i = 0; i < m; ++i) {
    if (idx[i] < 0 || idx[i] >= n) { gh_set_error("remove: index %lld is out of range for %lld points", (long long)idx[i], (long long)n); return GH_ERR_BAD_ARG; }
    if (i > 0 && idx[i] <= idx[i - 1]) { gh_set_error("remove: indices must be strictly increasing"); return GH_ERR_BAD_ARG; }
  }
  return GH_OK;
}

// dst (np2 x np2, lower 128-tiles) = src[keep, keep] with identity padding; one row per workgroup.  keep is increasing, so a column
// at or left of the diagonal stays there; the rest of the diagonal tile is written as zero (what potf2 leaves there).
__global__ __launch_bounds__(256) void remove_gather_lower_kernel(const double* src, long lds, const int* keep, long n2, double* dst, long ldd) {
  const long p = blockIdx.x, qend = (p / T + 1) * T;
  double* dr = dst + p * ldd;
  if (p < n2) {
    const double* sr = src + (long)keep[p] * lds;
    for (long q = threadIdx.x; q < qend; q += 256) dr[q] = (q <= p) ? sr[keep[q]] : 0.0;
  } else {
    for (long q = threadIdx.x; q < qend; q += 256) dr[q] = (q == p) ? 1.0 : 0.0;
  }
}
// W (rows [row0, np2) x 128, ld 128): W[p, c] = src[keep[p], rem[c]] where c < kc and rem[c] < keep[p], else 0
__global__ __launch_bounds__(128) void remove_gather_w_kernel(const double* src, long lds, const int* keep, long n2, const int* rem, int kc,
                                                             double* W, long row0) {
  const long p = row0 + blockIdx.x;
  const int c = threadIdx.x;
  double v = 0.0;
  if (p < n2 && c < kc) {
    const long kp = keep[p], rc = rem[c];
    if (rc < kp) v = src[kp * lds + rc];
  }
  W[p * T + c] = v;
}
__global__ void remove_gather_vec_kernel(const double* x, const double* yerr, const int* keep, long n2, int ndim, double* x2, double* yerr2) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n2) return;
  const long kp = keep[p];
  for (int d = 0; d < ndim; ++d) x2[p * ndim + d] = x[kp * ndim + d];
  if (yerr2) yerr2[p] = yerr[kp];
}
// The small step's substitution, two workgroups (64 columns of Wj each, one column per lane of the first wavefront, its solution in
// LDS): V = Ljj^-1 Wj.  The other wavefronts save the tile (Lold = Ljj: the tile itself receives Ljj Ljj^T + Wj Wj^T next) and set
// G = I (it receives V^T V).  Columns from kc on are zero columns of Wj.
__global__ __launch_bounds__(256) void remove_tile_solve_kernel(const double* __restrict__ Ljj, long ld, const double* __restrict__ Wj, int kc,
                                                               double* __restrict__ V, double* __restrict__ Lold, double* __restrict__ G) {
  __shared__ double X[T * 64];
  const int tid = threadIdx.x, half = blockIdx.x;
  if (tid >= 64) {
    for (int idx = tid - 64; idx < 64 * T; idx += 192) {
      const int i = half * 64 + idx / T, j = idx % T;
      Lold[i * T + j] = Ljj[(long)i * ld + j];
      G[i * T + j] = (i == j) ? 1.0 : 0.0;
    }
    return;
  }
  const int c = half * 64 + tid;
  if (half * 64 >= kc) {
    for (int i = 0; i < T; ++i) V[i * T + c] = 0.0;
    return;
  }
  for (int i = 0; i < T; ++i) {
    const double* Li = Ljj + (long)i * ld;
    double a0 = Wj[i * T + c], a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int k = 0;
    for (; k + 4 <= i; k += 4) {
      a0 -= Li[k] * X[k * 64 + tid];
      a1 -= Li[k + 1] * X[(k + 1) * 64 + tid];
      a2 -= Li[k + 2] * X[(k + 2) * 64 + tid];
      a3 -= Li[k + 3] * X[(k + 3) * 64 + tid];
    }
    for (; k < i; ++k) a0 -= Li[k] * X[k * 64 + tid];
    const double x = ((a0 + a1) + (a2 + a3)) / Li[i];
    X[i * 64 + tid] = x;
    V[i * T + c] = x;
  }
}
// The hot path: [Lij' | Wi'] = [Lij | Wi] Q for the 128 rows of one tile row i below j per workgroup, on the fp64 matrix pipe.  The
// two halves of the slab live in two buffers (the factor, leading dimension ld; W, 128 wide); Q arrives as four k-major blocks,
//   B11 = (Ljj^T L'^-T)^T,  nB21 = -(Wj^T L'^-T)^T,  nB12 = (V Ri)^T,  B22 = Ri^T   (128 x 128 each, ld 128),
// streamed through LDS in 16-deep slabs by the tile function of gh_gemm_tile.h.  The workgroup owns its rows, and no product reads
// what the launch has written: W' goes to the OTHER W buffer (Wn), the accumulating products read their C through the thread that
// wrote it, and L' = L B11^T is written in place only after every slab of L has been read (gh_tile128_nt_sp's contract).  Only the
// first kc (a multiple of 32) columns of W are summed over; the columns of W' from kc on come out as zeros.
__global__ __launch_bounds__(256, 2) void remove_apply_q_kernel(double* A, long ld, long row0, long col0, const double* Wo, double* Wn,
                                                               const double* B11, const double* nB21, const double* nB12,
                                                               const double* B22, long kc) {
  __shared__ __attribute__((aligned(1024))) double sm[4 * BM * BK];
  const long r = row0 + (long)blockIdx.x * T;
  double* Lt = A + r * ld + col0;
  const double* wo = Wo + r * T;
  double* wn = Wn + r * T;
  // (one inlined copy of each form of the tile function, not four: the kernel must fit its registers -- check_kernels.py)
#pragma unroll 1
  for (int step = 0; step < 2; ++step) {
    double* const C = step ? Lt : wn;
    const long ldc = step ? ld : (long)T;
    const double* const A0 = step ? (const double*)Lt : wo;      // W' = W Ri               | L' = L Ljj^T L'^-T
    const double* const A1 = step ? wo : (const double*)Lt;      // W' -= L (V Ri)          | L' += W Wj^T L'^-T
    const long lda0 = step ? ld : (long)T, lda1 = step ? (long)T : ld;
    gh_tile128_nt_sp<false>(sm, C, ldc, A0, lda0, step ? B11 : B22, T, step ? (long)T : kc);
    gh_tile128_nt_sp<true>(sm, C, ldc, A1, lda1, step ? nB21 : nB12, T, step ? kc : (long)T);
  }
}

static int gemm_any(hipStream_t st, double* C, int64_t ldc, const double* A, int64_t lda, bool a_km, const double* B, int64_t ldb, bool b_km,
                    double alpha, double beta) {
  return gh_launch_gemm(gemm_desc(C, ldc, A, lda, a_km, B, ldb, b_km, T, T, T, alpha, beta), st);
}

extern "C" int gh_chol_remove(gh_chol* s, const int64_t* idx, int64_t m, double* logdet_out) {
  if (!s) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  GH_CHECK(gh_chol_need_computed(s));
  GH_CHECK(gh_debug_check_remove_args(s->n, idx, m));
  const int64_t n = s->n, np = s->np, ndim = s->ndim, n2 = n - m, np2 = gh_round_up(n2, T), nt2 = np2 / T;
  if (idx[0] == n - m) return gh_chol_truncate(s, n2, logdet_out);          // (strictly increasing below n: the trailing run)
  if (g_remove_path == 2) { gh_set_error("remove: compute afresh on the kept points"); return GH_REFACTORIZE; }
  if (n >= (1LL << 31)) { gh_set_error("remove: too many points"); return GH_ERR_BAD_ARG; }
  hipStream_t st = s->st;
  // ---- the index maps (host)
  std::vector<int> maps((size_t)(n2 + m));
  {
    int64_t r = 0, p = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (r < m && idx[r] == i) { maps[(size_t)(n2 + r)] = (int)i; ++r; }
      else maps[(size_t)p++] = (int)i;
    }
  }
  const int64_t j0t = idx[0] / T;                          // first affected tile: idx[0] points are kept in front of the first removed one
  // ---- every allocation first: a failure up to here leaves the handle as it was (and so does every failure after it)
  GhBuf A2, dinv2, x2, yerr2;
  GhPooledBuf wb, qs, ib;
  GH_CHECK(take_factor_buffer(s, A2, np2));
  GH_CHECK(dinv2.ensure((size_t)nt2 * T * T * sizeof(double)));
  GH_CHECK(x2.ensure((size_t)np2 * ndim * sizeof(double)));
  if (s->have_yerr) GH_CHECK(yerr2.ensure((size_t)np2 * sizeof(double)));
  GH_CHECK(wb.ensure((size_t)2 * np2 * T * sizeof(double)));
  GH_CHECK(qs.ensure((size_t)7 * T * T * sizeof(double)));
  GH_CHECK(ib.ensure(maps.size() * sizeof(int)));
  GH_CHECK(s->scal.ensure(256 * sizeof(double)));
  s->d_info = (long long*)(s->scal.d() + 2);
  // (on an early error return the factor buffer goes back to the handle as its spare, not to the allocator)
  struct Spare { gh_chol* s; GhBuf& b; bool armed; ~Spare() { if (armed && b.p && !s->A_spare.p) { (void)hipStreamSynchronize(s->st); swap_bufs(s->A_spare, b); } } }
      spare{s, A2, true};
  const int* keepd = (const int*)ib.p;
  const int* remd = keepd + n2;
  double* const Ad = A2.d();
  double* const W0 = wb.d();
  double* const W1 = W0 + np2 * T;
  double* const V = qs.d();
  double* const Lold = V + T * T, * const G = Lold + T * T, * const dG = G + T * T, * const B11 = dG + T * T, * const nB21 = B11 + T * T,
        * const nB12 = nB21 + T * T;
  GH_HIP(hipMemcpyAsync(ib.p, maps.data(), maps.size() * sizeof(int), hipMemcpyHostToDevice, st));
  GH_HIP(hipMemsetAsync(s->d_info, 0, sizeof(long long), st));
  // ---- 1. gather
  long e_lay = -1;
  if (s->opts.profile) {
    for (auto& e : s->ev_lay) if (!e) GH_HIP(hipEventCreate(&e));
    e_lay = 0;
    GH_HIP(hipEventRecord(s->ev_lay[0], st));
  }
  hipLaunchKernelGGL(remove_gather_lower_kernel, dim3((unsigned)np2), dim3(256), 0, st, s->A.d(), (long)np, keepd, (long)n2, Ad, (long)np2);
  hipLaunchKernelGGL(remove_gather_vec_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, s->x.d(),
                     s->have_yerr ? s->yerr.d() : (const double*)nullptr, keepd, (long)n2, (int)ndim, x2.d(), s->have_yerr ? yerr2.d() : (double*)nullptr);
  GH_HIP(hipGetLastError());
  if (j0t > 0) GH_HIP(hipMemcpyAsync(dinv2.d(), s->dinv.d(), (size_t)j0t * T * T * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (e_lay >= 0) GH_HIP(hipEventRecord(s->ev_lay[1], st));
  // ---- 2. the passes: at most 128 columns of W each, read from the OLD factor
  for (int64_t c0 = 0; c0 < m; c0 += T) {
    const int64_t kc = std::min<int64_t>(T, m - c0), kcp = gh_round_up(kc, 32);
    const int64_t pc0 = idx[c0] - c0;                      // kept points in front of this pass's first column: rows of W before it are zero
    if (pc0 >= n2) break;                                  // (the rest of rem lies behind every kept point)
    const int64_t jt0 = pc0 / T;
    hipLaunchKernelGGL(remove_gather_w_kernel, dim3((unsigned)(np2 - jt0 * T)), dim3(128), 0, st, s->A.d(), (long)np, keepd, (long)n2,
                       remd + c0, (int)kc, W0, (long)(jt0 * T));
    GH_HIP(hipGetLastError());
    double* cur = W0;
    double* oth = W1;
    for (int64_t j = jt0; j < nt2; ++j) {
      double* Ljj = Ad + j * T * np2 + j * T;
      double* Wj = cur + j * T * T;
      double* dS = dinv2.d() + j * T * T;
      hipLaunchKernelGGL(remove_tile_solve_kernel, dim3(2), dim3(256), 0, st, Ljj, (long)np2, Wj, (int)kc, V, Lold, G);
      GH_HIP(hipGetLastError());
      GH_CHECK(gemm_any(st, Ljj, np2, Lold, T, true, Lold, T, true, 1.0, 0.0));        // S = Ljj Ljj^T
      GH_CHECK(gemm_any(st, Ljj, np2, Wj, T, true, Wj, T, true, 1.0, 1.0));            //   + Wj Wj^T
      GH_CHECK(gh_launch_potf2_mfma(Ljj, np2, dS, s->d_info, j * T, st));              // L', L'^-1
      if (j + 1 == nt2) break;
      GH_CHECK(gemm_any(st, G, T, V, T, false, V, T, false, 1.0, 1.0));                // G = I + V^T V
      GH_CHECK(gh_launch_potf2_mfma(G, T, dG, s->d_info, j * T, st));                  // C, C^-1 = Ri^T
      GH_CHECK(gemm_any(st, B11, T, dS, T, true, Lold, T, false, 1.0, 0.0));           // L'^-1 Ljj
      GH_CHECK(gemm_any(st, nB21, T, dS, T, true, Wj, T, false, -1.0, 0.0));           // -L'^-1 Wj
      GH_CHECK(gemm_any(st, nB12, T, dG, T, true, V, T, true, 1.0, 0.0));              // Ri^T V^T
      hipLaunchKernelGGL(remove_apply_q_kernel, dim3((unsigned)(nt2 - j - 1)), dim3(256), 0, st, Ad, (long)np2, (long)((j + 1) * T), (long)(j * T),
                         cur, oth, B11, nB21, nB12, dG, (long)kcp);
      GH_HIP(hipGetLastError());
      std::swap(cur, oth);
    }
  }
  // ---- 3. log-det over the new diagonal; one synchronisation brings it back with the failure word
  GH_CHECK(gh_launch_logdet(Ad, (long)np2, (long)np2, s->scal.d(), s->scal.d() + 8, st));
  double back[3] = {0.0, 0.0, 0.0};
  GH_CHECK(read_scalars(s, back, 3, st));
  GH_HIP(hipStreamSynchronize(st));
  const long long info_host = info_from_bits(back[2]);
  if (e_lay >= 0) { float ms = 0; GH_HIP(hipEventElapsedTime(&ms, s->ev_lay[0], s->ev_lay[1])); s->prof.reserved[0] = ms; }
  if (info_host != 0 || !std::isfinite(back[0])) {
    gh_set_error("remove: the update met a pivot that is not positive and finite (tile row of index %lld); the factor is unchanged", info_host);
    return GH_ERR_NOT_PD;
  }
  spare.armed = false;
  swap_bufs(s->A, A2); swap_bufs(s->A_spare, A2);          // (the old factor buffer is the spare now)
  swap_bufs(s->dinv, dinv2); swap_bufs(s->x, x2);
  if (s->have_yerr) swap_bufs(s->yerr, yerr2);
  s->n = n2; s->np = np2; s->info = 0;
  s->logdet = back[0];
  if (logdet_out) *logdet_out = back[0];
  return GH_OK;
}
