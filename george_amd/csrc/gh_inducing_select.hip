// gh_inducing_select.hip -- greedy max-min selection of inducing points on the device: gh_inducing_select
// (include/george_amd.h has the definition; the host form is inducing_points in george_amd/solvers/inducing.py)
//
// The rule: idx[0] = first, dmin_i = +inf; for j = 1, 2, ...: dmin_i = min(dmin_i, d2(x_i, x_idx[j-1])), then idx[j] = the index
// of the largest dmin, ties going to the LOWER index.  One step kernel per pick, back to back on one stream: step j reads
// idx[j-1] from device memory, so the host never waits between steps, and no workgroup ever waits for another one.
//
// Step kernel: the points lie coordinate-major (one transposing pass per call), so that a wavefront reads 512 contiguous bytes
// per coordinate.  A thread walks its points grid-stride, four at a time, writes the new dmin and keeps its best key
// (dmin, index); the key order -- larger dmin first, then lower index -- is total, so the result does not depend on the grid or
// on the order of the reduction, and two calls give the same bits.  Reduction: shuffles across the wavefront, LDS across the
// workgroup, one partial key per workgroup in device memory.  The workgroup that finishes last -- a ticket from one atomicAdd
// behind __threadfence() -- reduces the partials, writes idx[j] and resets the ticket.  The partials cross workgroups inside a
// launch: they are written and read with agent-scope atomic stores and loads (which bypass the per-CU cache), the ticket is an
// agent-scope atomic, and the word is zeroed by a memset at the start of every call.  A grid of one workgroup skips all that.
//
// d2 = sum_k (x_ik - c_k)^2 from k = 0 on, one rounding per operation (no contraction into fused multiply-adds): for ndim <= 7
// that is the double NumPy's ((x - c)**2).sum(axis=1) gives, so the sequence equals the host routine's, ties and repeats past
// the number of distinct points included.  For more dimensions NumPy adds pairwise, and the result is the greedy sequence under
// THIS distance.  A d2 that is not a number never replaces a dmin, so every pick is a valid index whatever x holds.
#include <math.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"

#define IS_THREADS 256                  // threads of a workgroup
#define IS_UNROLL 4                     // points of one thread in flight
#define IS_WG_POINTS (IS_THREADS * IS_UNROLL)   // the grid has one workgroup per IS_WG_POINTS points: a small n launches few
#define IS_MAX_WG 1024                  // ... and at most this many (4 per CU); from there on a thread walks further

typedef unsigned long long is_u64;

__device__ __forceinline__ bool is_better(double d1, int i1, double d2, int i2) { return d1 > d2 || (d1 == d2 && i1 < i2); }

struct IsShared {
  double d[IS_THREADS / 64];
  int i[IS_THREADS / 64];
  int last;
};

// the best key of the workgroup, valid in thread 0
__device__ __forceinline__ void is_block_reduce(IsShared& sh, double& bd, int& bi) {
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_down(bd, off, 64);
    const int oi = __shfl_down(bi, off, 64);
    if (is_better(od, oi, bd, bi)) { bd = od; bi = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh.d[wave] = bd; sh.i[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < IS_THREADS / 64; ++w)
      if (is_better(sh.d[w], sh.i[w], bd, bi)) { bd = sh.d[w]; bi = sh.i[w]; }
}

// xt[k * ld + i] = x[i * nd + k]
__global__ __launch_bounds__(IS_THREADS) void inducing_select_transpose_kernel(const double* __restrict__ x, long n, int nd, long ld,
                                                                               double* __restrict__ xt) {
  const long e = (long)blockIdx.x * IS_THREADS + threadIdx.x;
  if (e >= n * nd) return;
  const long k = e / n, i = e - k * n;
  xt[k * ld + i] = x[i * nd + k];
}

// One step: dmin <- min(dmin, d2(., x_p)) with p = init ? first : *prev (init: dmin starts at +inf and is not read), and
// *pick = the index of the largest new dmin, the lower index among equals.  pd, pi: one partial key per workgroup.  ND: the
// number of coordinates when it is 1, 2 or 3 (their loads are then all in flight at once), 0: nd of them.
template <int ND>
__global__ __launch_bounds__(IS_THREADS) void inducing_select_step_kernel(const double* __restrict__ xt, long ld, int n, int nd, int init,
                                                                          int first, const int* __restrict__ prev,
                                                                          double* __restrict__ dmin, is_u64* pd, int* pi,
                                                                          unsigned* ticket, int* pick) {
#pragma clang fp contract(off)
  __shared__ IsShared sh;
  const int p = init ? first : prev[0];
  const int nk = ND ? ND : nd;
  const long gs = (long)gridDim.x * IS_THREADS;
  double bd = -1.0;                                         // below every dmin: 0 <= dmin <= +inf
  int bi = 0x7fffffff;
  for (long i0 = (long)blockIdx.x * IS_THREADS + threadIdx.x; i0 < n; i0 += IS_UNROLL * gs) {
    long il[IS_UNROLL];                                     // a point past the end reads point i0 again and is dropped below
    double s[IS_UNROLL], old[IS_UNROLL];
#pragma unroll
    for (int u = 0; u < IS_UNROLL; ++u) {
      const long i = i0 + u * gs;
      il[u] = i < n ? i : i0;
      s[u] = 0.0;
      old[u] = INFINITY;
    }
    if (!init) {
#pragma unroll
      for (int u = 0; u < IS_UNROLL; ++u) old[u] = dmin[il[u]];
    }
#pragma unroll
    for (int k = 0; k < nk; ++k) {
      const double* row = xt + k * ld;
      const double c = row[p];
#pragma unroll
      for (int u = 0; u < IS_UNROLL; ++u) {
        const double d = row[il[u]] - c;
        const double e = d * d;
        s[u] = s[u] + e;
      }
    }
#pragma unroll
    for (int u = 0; u < IS_UNROLL; ++u) {                   // (ascending in i)
      const long i = i0 + u * gs;
      if (i < n) {
        const double now = s[u] < old[u] ? s[u] : old[u];
        dmin[i] = now;
        if (is_better(now, (int)i, bd, bi)) { bd = now; bi = (int)i; }
      }
    }
  }
  is_block_reduce(sh, bd, bi);
  if (gridDim.x == 1) {
    if (threadIdx.x == 0) pick[0] = (bi >= 0 && bi < n) ? bi : 0;
    return;
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(pd + blockIdx.x, (is_u64)__double_as_longlong(bd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pi + blockIdx.x, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                        // the partial is out before the ticket is drawn
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == gridDim.x - 1;
    if (last) __threadfence();
    sh.last = last;
  }
  __syncthreads();
  if (!sh.last) return;                                     // (workgroup-uniform)
  bd = -1.0;
  bi = 0x7fffffff;
  for (unsigned b = threadIdx.x; b < gridDim.x; b += IS_THREADS) {
    const double od = __longlong_as_double((long long)__hip_atomic_load(pd + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const int oi = __hip_atomic_load(pi + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (is_better(od, oi, bd, bi)) { bd = od; bi = oi; }
  }
  is_block_reduce(sh, bd, bi);                              // (thread 0 read sh.d, sh.i of the first reduction before the barrier above)
  if (threadIdx.x == 0) {
    pick[0] = (bi >= 0 && bi < n) ? bi : 0;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // for the next step
  }
}

// ================================================================================ host side
extern "C" int gh_inducing_select(int32_t device, const double* x, int64_t n, int32_t ndim, int64_t first, int64_t m,
                                  int64_t* idx_out, double* dmin_out) {
  if (m < 1) { gh_set_error("the selection takes m >= 1, not %lld", (long long)m); return GH_ERR_BAD_ARG; }
  if (!idx_out || n < 0 || n > 0x7ffffff0L) { gh_set_error("bad argument to the selection of inducing points"); return GH_ERR_BAD_ARG; }
  if (ndim < 1 || ndim > GH_MAX_NDIM) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (n > 0 && !x) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (n > 0 && (first < 0 || first >= n)) { gh_set_error("the first point %lld is not one of the %lld points", (long long)first, (long long)n); return GH_ERR_BAD_ARG; }
  if (n == 0) return GH_OK;
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd selection of inducing points needs an MI355X"); return GH_ERR_HIP; }
  if (hipSetDevice(device) != hipSuccess) { gh_set_error("cannot initialise HIP device %d", (int)device); return GH_ERR_HIP; }
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;                                 // (the null stream where the shared ones could not be made)
  if (gh_shared_streams(device, shq) && shq[0]) st = shq[0];
  const int64_t k = std::min(m, n);
  const int64_t steps = dmin_out ? k : k - 1;               // step j makes pick j; the last one only completes dmin
  const int64_t ld = gh_round_up(n, 32);                    // (rows of xt start on a 256-byte boundary)
  const unsigned nwg = (unsigned)std::min<int64_t>((n + IS_WG_POINTS - 1) / IS_WG_POINTS, IS_MAX_WG);
  GhPooledBuf xa, xt, dm, pk, pd, pi, tk;
  const double* x_dev = x;
  if (!gh_is_device_ptr(x)) {
    GH_CHECK(xa.ensure((size_t)n * ndim * sizeof(double)));
    GH_CHECK(gh_to_device(xa.d(), x, (size_t)n * ndim, st));
    x_dev = xa.d();
  }
  GH_CHECK(xt.ensure((size_t)ld * ndim * sizeof(double)));
  GH_CHECK(dm.ensure((size_t)n * sizeof(double)));
  GH_CHECK(pk.ensure((size_t)(k + 1) * sizeof(int)));
  GH_CHECK(pd.ensure((size_t)nwg * sizeof(is_u64)));
  GH_CHECK(pi.ensure((size_t)nwg * sizeof(int)));
  GH_CHECK(tk.ensure(16));
  GH_HIP(hipMemsetAsync(tk.p, 0, 16, st));
  {
    const int64_t total = n * ndim;
    hipLaunchKernelGGL(inducing_select_transpose_kernel, dim3((unsigned)((total + IS_THREADS - 1) / IS_THREADS)), dim3(IS_THREADS), 0, st,
                       x_dev, (long)n, (int)ndim, (long)ld, xt.d());
    GH_HIP(hipGetLastError());
  }
  const auto step = ndim == 1 ? inducing_select_step_kernel<1> : ndim == 2 ? inducing_select_step_kernel<2>
                    : ndim == 3 ? inducing_select_step_kernel<3> : inducing_select_step_kernel<0>;
  int* picks = (int*)pk.p;                                  // picks[j] for 1 <= j <= steps; pick 0 is `first`
  for (int64_t j = 1; j <= steps; ++j) {
    step<<<dim3(nwg), dim3(IS_THREADS), 0, st>>>((const double*)xt.d(), (long)ld, (int)n, (int)ndim, j == 1 ? 1 : 0, (int)first,
                                                 (const int*)(picks + j - 1), dm.d(), (is_u64*)pd.p, (int*)pi.p, (unsigned*)tk.p, picks + j);
    GH_HIP(hipGetLastError());
  }
  std::vector<int> ph((size_t)k);
  if (k > 1) GH_HIP(hipMemcpyAsync(ph.data() + 1, picks + 1, (size_t)(k - 1) * sizeof(int), hipMemcpyDeviceToHost, st));
  if (dmin_out) GH_CHECK(gh_from_device(dmin_out, dm.d(), (size_t)n, st));
  GH_HIP(hipStreamSynchronize(st));
  idx_out[0] = first;
  for (int64_t j = 1; j < k; ++j) idx_out[j] = ph[(size_t)j];
  return GH_OK;
}
