// gh_vecchia_search.hip -- the exact nearest-neighbour search behind gh_vecchia_search and gh_vecchia_predict_local_search
// (include/george_amd.h has the definition; gh_vecchia_impl.h what the two Vecchia units share)
//
// Index: a uniform cell grid over the bounding box of the first g = min(ndim, 3) coordinates; the points are sorted by cell with
// a counting sort on the host (O(N), once per data set) and their coordinates kept in that order next to the original indices, so
// that a cell -- and a run of cells along the last grid axis -- is one contiguous read.  A distance in the projection on the
// gridded coordinates is a lower bound of the full distance: pruning is exact in any dimension and prunes less as ndim grows.
//
// Query kernel: one query per wavefront.  The 64 lanes hold the 64 best keys (d2, index) seen so far as a sorted list, lane s the
// s-th best; lane m - 1 is the worst key that still counts.  Cells are visited in rings of growing Chebyshev cell distance R
// around the query's cell (a query outside the box: the boundary cell).  64 candidates at a time: every lane computes one d2,
// a ballot marks the eligible ones below the worst key, and each marked one is put in its place with a shift by one lane.
// After ring R every unvisited point differs from the query by more than R h_min in a gridded coordinate; the walk ends when the
// list is full and its worst d2 is STRICTLY below (R h_min)^2 (1 - 2e-8) -- the margin covers the rounding of the cell numbers,
// DESIGN.md has the argument -- or when every cell has been visited.  The key order is total and every point is met once: the
// result does not depend on the visiting order, and two calls give the same bits.  No LDS, no scratch memory, no atomics.
//
// d2 = sum_k (x_k - q_k)^2 from k = 0 on, one rounding per operation (no contraction into fused multiply-adds): for ndim <= 7
// that is the double NumPy's ((x - q)**2).sum(axis=-1) gives, so the table equals the host search's, near-ties included.
#include <limits.h>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"
#include "gh_vecchia_impl.h"

#define VS_WAVES 4                      // queries (wavefronts) per workgroup; they share nothing
#define VS_MARGIN (1.0 - 2e-8)          // on the squared bound: (1 - 1e-8)^2

__device__ __forceinline__ double vs_lane_d(double v, int src_lane) {             // src_lane: wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ bool vs_less(double d1, int i1, double d2, int i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }
__device__ __forceinline__ double vs_d2(const double* __restrict__ p, const double* __restrict__ q, int nd) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int k = 0; k < nd; ++k) {
    const double d = p[k] - q[k];
    const double e = d * d;
    s = s + e;
  }
  return s;
}
__device__ __forceinline__ int vs_cell(double v, double lo, double inv_h, int nc) {
  if (nc <= 1) return 0;
  const double t = (v - lo) * inv_h;
  return t >= 0.0 ? (t < (double)nc ? (int)t : nc - 1) : 0;                      // (not a number: cell 0)
}

// the sorted points p0 <= p < p1 against the list: (kd, ki) this lane's key, (wd, wi) the key of lane m - 1
__device__ __forceinline__ void vs_scan(const GhVGridDev& G, const double* __restrict__ qc, long lim, int m, int lane, long p0, long p1,
                                        double& kd, int& ki, double& wd, int& wi) {
  for (long base = p0; base < p1; base += 64) {
    const long p = base + lane;
    double d = 0.0;
    int j = 0;
    bool take = false;
    if (p < p1) {
      j = G.idx[p];
      if ((long)j < lim) {
        d = vs_d2(G.xs + p * G.nd, qc, G.nd);
        take = vs_less(d, j, wd, wi);
      }
    }
    unsigned long long mask = __ballot(take);
    while (mask) {
      const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
      mask &= mask - 1;
      const double cd = vs_lane_d(d, b);
      const int cj = __builtin_amdgcn_readlane(j, b);
      if (!vs_less(cd, cj, wd, wi)) continue;               // (the worst key has moved since the ballot)
      const double pd = __shfl_up(kd, 1, 64);
      const int pi = __shfl_up(ki, 1, 64);
      if (vs_less(cd, cj, kd, ki)) {                        // this lane's key moves up one lane: it takes its neighbour's, or the candidate
        const bool shift = lane > 0 && vs_less(cd, cj, pd, pi);
        kd = shift ? pd : cd;
        ki = shift ? pi : cj;
      }
      wd = vs_lane_d(kd, m - 1);
      wi = __builtin_amdgcn_readlane(ki, m - 1);
    }
  }
}

__global__ __launch_bounds__(64 * VS_WAVES) void vecchia_search_kernel(GhVGridDev G, const double* __restrict__ q, long nq,
                                                                       const long long* __restrict__ limit, int m,
                                                                       int* __restrict__ table, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const long c = (long)blockIdx.x * VS_WAVES + (threadIdx.x >> 6);
  if (c >= nq) return;                                      // (wave-uniform; the waves of a workgroup never meet)
  const double* qc = q + c * G.nd;
  const long lim = limit ? (long)limit[c] : G.n;
  const int off = VG_AXES - G.g;
  const int n0 = G.nc[0], n1 = G.nc[1], n2 = G.nc[2];
  const int c0 = off <= 0 ? vs_cell(qc[0 - off], G.lo[0], G.inv_h[0], n0) : 0;
  const int c1 = off <= 1 ? vs_cell(qc[1 - off], G.lo[1], G.inv_h[1], n1) : 0;
  const int c2 = vs_cell(qc[2 - off], G.lo[2], G.inv_h[2], n2);
  const int rmax = max(max(max(c0, n0 - 1 - c0), max(c1, n1 - 1 - c1)), max(c2, n2 - 1 - c2));
  double kd = INFINITY, wd = INFINITY;
  int ki = INT_MAX, wi = INT_MAX;
  for (int R = 0;; ++R) {
    const int a0 = max(c0 - R, 0), a1 = min(c0 + R, n0 - 1);
    const int b0 = max(c1 - R, 0), b1 = min(c1 + R, n1 - 1);
    const int z0 = max(c2 - R, 0), z1 = min(c2 + R, n2 - 1);
    for (int i0 = a0; i0 <= a1; ++i0)
      for (int i1 = b0; i1 <= b1; ++i1) {
        const long row = ((long)i0 * n1 + i1) * n2;
        if (abs(i0 - c0) == R || abs(i1 - c1) == R) {       // on the ring in one of the slow axes: the whole run along the fast one
          vs_scan(G, qc, lim, m, lane, G.start[row + z0], G.start[row + z1 + 1], kd, ki, wd, wi);
        } else {                                            // (R >= 1) inside it: the run's two end cells
          if (c2 - R >= 0) vs_scan(G, qc, lim, m, lane, G.start[row + c2 - R], G.start[row + c2 - R + 1], kd, ki, wd, wi);
          if (c2 + R <= n2 - 1) vs_scan(G, qc, lim, m, lane, G.start[row + c2 + R], G.start[row + c2 + R + 1], kd, ki, wd, wi);
        }
      }
    if (R >= rmax) break;                                   // every cell visited
    const double reach = (double)R * G.h_min;
    if (wi != INT_MAX && wd < reach * reach * VS_MARGIN) break;
  }
  // the row ascending by index: a key's place is the number of keys below it
  const bool have = lane < m && ki != INT_MAX;
  int rank = 0;
  for (int t = 0; t < m; ++t) rank += __builtin_amdgcn_readlane(ki, t) < ki ? 1 : 0;
  const int count = __popcll(__ballot(have));
  if (have) table[c * m + rank] = ki;
  else if (lane < m) table[c * m + lane] = -1;              // (the lanes without a key are count .. m - 1)
  if (lane == 0) cnt[c] = count;
}

// ================================================================================ host side
int gh_vgrid_build(GhVGrid& G, const double* x, int64_t n, int nd, int occupancy, hipStream_t st) {
  G.valid = false;
  const int g = std::min(nd, VG_AXES), off = VG_AXES - g;
  GhVGridDev& D = G.dev;
  double ext[VG_AXES];
  for (int a = 0; a < VG_AXES; ++a) { D.nc[a] = 1; D.lo[a] = 0.0; D.inv_h[a] = 0.0; ext[a] = 0.0; }
  for (int k = 0; k < g; ++k) {
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t i = 0; i < n; ++i) {
      const double v = x[i * nd + k];
      if (v < mn) mn = v;
      if (v > mx) mx = v;
    }
    const double e = mx - mn;
    D.lo[off + k] = std::isfinite(mn) ? mn : 0.0;
    ext[off + k] = (e > 0.0 && std::isfinite(e)) ? e : 0.0;                       // (zero extent: one cell)
  }
  // cells per axis: cubes of edge h with `occ` points each on average, at most n cells in all
  const int64_t occ = occupancy > 0 ? occupancy : VG_OCCUPANCY;
  const int64_t target = std::max<int64_t>(1, n / occ);
  int active = 0;
  double logvol = 0.0;
  for (int a = 0; a < VG_AXES; ++a)
    if (ext[a] > 0.0) { ++active; logvol += log(ext[a]); }
  if (active > 0 && target > 1) {
    double h = exp((logvol - log((double)target)) / active);
    for (int it = 0; it < 4096; ++it) {
      double prod = 1.0;
      for (int a = 0; a < VG_AXES; ++a) {
        const double c = ext[a] > 0.0 ? floor(ext[a] / h) : 1.0;
        D.nc[a] = (int)std::min<double>(std::max<double>(c, 1.0), (double)VG_AXIS_CELLS);
        prod *= D.nc[a];
      }
      if (prod <= (double)target && std::isfinite(h)) break;
      h *= 1.0625;                                          // (a thin axis was rounded up to one cell: coarser cubes)
      if (it == 4095) D.nc[0] = D.nc[1] = D.nc[2] = 1;
    }
  }
  D.h_min = 0.0;
  int64_t ncells = 1;
  for (int a = 0; a < VG_AXES; ++a) {
    ncells *= D.nc[a];
    if (D.nc[a] > 1) {
      D.inv_h[a] = (double)D.nc[a] / ext[a];
      const double h = ext[a] / (double)D.nc[a];
      D.h_min = D.h_min > 0.0 ? std::min(D.h_min, h) : h;
    }
  }
  // counting sort by cell number (the last slot runs fastest); a point keeps its place among the points of its cell
  std::vector<int> cell((size_t)n), start((size_t)ncells + 1, 0), idx((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t id = 0;
    for (int a = 0; a < VG_AXES; ++a) {
      int ca = 0;
      if (D.nc[a] > 1) {
        const double t = (x[i * nd + (a - off)] - D.lo[a]) * D.inv_h[a];
        ca = t >= 0.0 ? (t < (double)D.nc[a] ? (int)t : D.nc[a] - 1) : 0;
      }
      id = id * D.nc[a] + ca;
    }
    cell[(size_t)i] = (int)id;
    ++start[(size_t)id + 1];
  }
  for (int64_t c = 0; c < ncells; ++c) start[(size_t)c + 1] += start[(size_t)c];
  std::vector<int> at(start.begin(), start.end() - 1);
  std::vector<double> xs((size_t)n * nd);
  for (int64_t i = 0; i < n; ++i) {
    const int p = at[(size_t)cell[(size_t)i]]++;
    idx[(size_t)p] = (int)i;
    memcpy(&xs[(size_t)p * nd], &x[i * nd], sizeof(double) * nd);
  }
  GH_CHECK(G.xs.ensure(std::max<size_t>(xs.size(), 1) * sizeof(double)));
  GH_CHECK(G.idx.ensure(std::max<size_t>(idx.size(), 1) * sizeof(int)));
  GH_CHECK(G.start.ensure(start.size() * sizeof(int)));
  if (n > 0) {
    GH_HIP(hipMemcpyAsync(G.xs.p, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice, st));
    GH_HIP(hipMemcpyAsync(G.idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, st));
  }
  GH_HIP(hipMemcpyAsync(G.start.p, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice, st));
  GH_HIP(hipStreamSynchronize(st));                         // (the host vectors end with this call)
  D.xs = G.xs.d(); D.idx = (const int*)G.idx.p; D.start = (const int*)G.start.p;
  D.n = (long)n; D.nd = nd; D.g = g;
  G.occupancy = occupancy;
  G.valid = true;
  return GH_OK;
}

int gh_vgrid_query(const GhVGrid& G, const double* q, int64_t nq, const int64_t* limit, int m, int* table, int* cnt, hipStream_t st) {
  if (!G.valid || m < 1 || m > VM_MAX || nq <= 0) { gh_set_error("bad argument to the neighbour search"); return GH_ERR_BAD_ARG; }
  const unsigned nwg = (unsigned)((nq + VS_WAVES - 1) / VS_WAVES);
  hipLaunchKernelGGL(vecchia_search_kernel, dim3(nwg), dim3(64 * VS_WAVES), 0, st, G.dev, q, (long)nq, (const long long*)limit, m, table, cnt);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

extern "C" int gh_vecchia_search(int32_t device, const double* x, int64_t n, int32_t ndim, const double* q, int64_t nq,
                                 const int64_t* limit, int32_t m, int32_t occupancy, int32_t* table_out) {
  if (m < 1 || m > VM_MAX) { gh_set_error("the neighbour search takes 1 <= m <= %d, not %d", VM_MAX, (int)m); return GH_ERR_BAD_ARG; }
  if (!table_out || n < 0 || nq < 0 || n > 0x7ffffff0L || nq > 0x3fffffffL || occupancy < 0) { gh_set_error("bad argument to the neighbour search"); return GH_ERR_BAD_ARG; }
  if (ndim < 1 || ndim > GH_MAX_NDIM) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if ((n > 0 && !x) || (nq > 0 && !q)) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (nq == 0) return GH_OK;
  if (n == 0) {
    std::fill(table_out, table_out + (size_t)nq * m, -1);
    return GH_OK;
  }
  if (gh_device_count() <= 0) { gh_set_error("no HIP device available: the george_amd neighbour search needs an MI355X"); return GH_ERR_HIP; }
  if (hipSetDevice(device) != hipSuccess) { gh_set_error("cannot initialise HIP device %d", (int)device); return GH_ERR_HIP; }
  hipStream_t shq[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t st = nullptr;                                 // (the null stream where the shared ones could not be made)
  if (gh_shared_streams(device, shq) && shq[0]) st = shq[0];
  std::vector<double> xh;
  if (gh_is_device_ptr(x)) {
    xh.resize((size_t)n * ndim);
    GH_HIP(hipMemcpy(xh.data(), x, xh.size() * sizeof(double), hipMemcpyDeviceToHost));
    x = xh.data();
  }
  GhVGrid G;
  GhPooledBuf qd, ld, tab, cnt;
  GH_CHECK(gh_vgrid_build(G, x, n, ndim, occupancy, st));
  const double* q_dev = q;
  if (!gh_is_device_ptr(q)) {
    GH_CHECK(qd.ensure((size_t)nq * ndim * sizeof(double)));
    GH_CHECK(gh_to_device(qd.d(), q, (size_t)nq * ndim, st));
    q_dev = qd.d();
  }
  const int64_t* l_dev = limit;
  if (limit && !gh_is_device_ptr(limit)) {
    GH_CHECK(ld.ensure((size_t)nq * sizeof(int64_t)));
    GH_HIP(hipMemcpyAsync(ld.p, limit, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, st));
    l_dev = (const int64_t*)ld.p;
  }
  GH_CHECK(tab.ensure((size_t)nq * m * sizeof(int)));
  GH_CHECK(cnt.ensure((size_t)nq * sizeof(int)));
  GH_CHECK(gh_vgrid_query(G, q_dev, nq, l_dev, m, (int*)tab.p, (int*)cnt.p, st));
  GH_HIP(hipMemcpyAsync(table_out, tab.p, (size_t)nq * m * sizeof(int), hipMemcpyDefault, st));
  GH_HIP(hipStreamSynchronize(st));
  return GH_OK;
}
