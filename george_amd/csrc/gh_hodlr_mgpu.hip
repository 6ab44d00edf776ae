// gh_hodlr_mgpu.hip -- the HODLR tree split over several devices (gh_hodlr_impl.h has the map of the units)
#include <atomic>
#include <thread>
#include "gh_hodlr_impl.h"
#include "gh_threads.h"

// ===================================================================== the tree split over several devices
// gh_hodlr_mgpu_* (include/george_amd.h): the top log2(P) levels of the tree are shared, sub-tree p is an ordinary
// gh_hodlr handle on devices[p] in sub-tree mode (HSub, gh_hodlr_impl.h).  One host thread per device; the threads meet at host
// barriers, and the only data they exchange after the ancestors' factors have been dealt out are the 2R x C sums of the
// top levels, through pinned host memory.
namespace {
std::mutex g_hm_dev_mu[16];          // one clustered (spin-waiting) ACA grid per PHYSICAL device at a time ("virtual devices")

struct gh_hodlr_mgpu_impl;
struct HmRank {
  int p = 0, dev = 0;
  gh_hodlr* h = nullptr;
  gh_kernel kern;
  GhBuf xg;                                   // all N points: only where the ACA of a top node runs
  std::vector<GhBuf*> stage;                  // [depth] local rows of the ancestors' factors, column-major n x R_l
  long row0 = 0, n = 0;
  double* pin = nullptr;                      // pinned: [0, cap) this device's partial sums, [cap, 2 cap) the completed sums
  size_t pin_cap = 0, pin_cnt = 0;
  std::unique_lock<std::mutex> dev_lock;
  int rc = GH_OK;
  std::string err;
  double ld = 0.0;
  gh_hodlr_mgpu_impl* owner = nullptr;
  std::vector<int> seed_off;
};
struct HmTop {                                // a node above the split
  int level = 0, q = 0, start = 0, half = 0, size = 0;
  int runner = 0;                             // the rank whose device runs its ACA
  int first = 0, span = 1;                    // the ranks below it: [first, first + span)
  int rank = 0;
  GhBuf Tcm, packed;                          // on the runner's device: ACA scratch; the same rows dealt into one contiguous chunk per rank
  std::vector<long> pack_off;
  HostBarrier bar;
};
struct gh_hodlr_mgpu_impl {
  gh_hodlr_mgpu_opts opts;
  int P = 1, depth = 0;
  std::vector<HmRank> ranks;
  std::vector<std::vector<HmTop*>> top;       // [level][q]
  HostBarrier world;
  std::atomic<int> abort{0};
  int64_t n = 0;
  int ndim = 0;
  bool computed = false;
  double logdet = 0.0;
  std::vector<int> all_ranks;
  int64_t top_n = -1;                         // the top nodes in `top` were laid out for this many points / this min_size
  int top_min = -1;
  void clear_top() { for (auto& lv : top) for (auto* t : lv) { if (t) { (void)hipSetDevice(ranks[t->runner].dev); delete t; } } top.clear(); }
};

// out[k * n_m + i] = Tcm[k * N + row0 + i]: the rows of one device out of a node's column-major factors
__global__ void hodlr_pack_rows_kernel(const double* Tcm, long N, long row0, long n_m, int r, double* out) {
  const long tot = n_m * r;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const long k = e / n_m, i = e % n_m;
    out[e] = Tcm[k * N + row0 + i];
  }
}

// hodlr.h:136-221 for ONE node above the split, on this handle's device against all N points (x_dev).  Same kernel,
// same cluster rule and same retry ladder as the levels of gh_hodlr_compute; nd.pad = the node's index in its level.
int aca_top_node(gh_hodlr* h, gh_kernel* k, const double* x_dev, long N, int ndim, int level, LvlNode nd, GhBuf& Tcm, int* rank_out) {
  hipStream_t st = h->st;
  GhPooledBuf d_node, d_rank, idx, sync, part;       // (all used on st only, and the call ends synchronised)
  GH_CHECK(d_node.ensure(sizeof(LvlNode)));
  GH_CHECK(d_rank.ensure(sizeof(int)));
  GH_HIP(hipMemcpyAsync(d_node.p, &nd, sizeof(LvlNode), hipMemcpyHostToDevice, st));
  int G = 1;
  {
    const int ept = 2;
    while (G * 2 <= 256 && (long)(G * 2) * ACA_THREADS * ept <= nd.half) G *= 2;
  }
  const int aca_fence = 0, aca_multi = 1;
  const int pstride = 8 + 2 * ACA_MAXR;
  const bool user_cap = h->opts.max_rank > 0;
  int rc = user_cap ? h->opts.max_rank : std::min(256, RANK_CAP);
  GH_CHECK(idx.ensure((size_t)N * sizeof(int)));
  GH_CHECK(sync.ensure(sizeof(unsigned) + sizeof(int) + 2 * sizeof(int)));
  GH_CHECK(part.ensure((size_t)G * pstride * sizeof(double)));
  for (;;) {
    GH_CHECK(Tcm.ensure((size_t)N * rc * sizeof(double)));
    GH_HIP(hipMemsetAsync(sync.p, 0, sizeof(unsigned) + sizeof(int) + 2 * sizeof(int), st));
    unsigned* d_bars = (unsigned*)sync.p;
    int* d_sel = (int*)(d_bars + 1);
    int* d_fail = d_sel + 1;
    AcaLaunch a{};
    a.x = x_dev; a.N = N; a.ndim = ndim;
    a.nodes = (const LvlNode*)d_node.p; a.Tcm = Tcm.d(); a.idx = (int*)idx.p; a.ranks = (int*)d_rank.p;
    a.bars = d_bars; a.part = part.d(); a.sel = d_sel; a.fail = d_fail; a.trunc = d_fail + 1;
    a.nwg = G; a.G = G; a.level = level; a.rc = rc; a.pstride = pstride; a.multi = aca_multi; a.fence = aca_fence; a.ones_only = G == 1;
    GH_CHECK(hodlr_launch_aca(h, k, a, st));
    int flags[2] = {0, 0};
    GH_HIP(hipMemcpyAsync(flags, d_fail, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GH_HIP(hipMemcpyAsync(rank_out, d_rank.p, sizeof(int), hipMemcpyDeviceToHost, st));
    GH_HIP(hipStreamSynchronize(st));
    if (flags[0]) { gh_set_error("HODLR: cluster barrier of the ACA kernel timed out at level %d", level); return GH_ERR_HIP; }
    if (!flags[1]) return GH_OK;
    if (user_cap || rc >= RANK_CAP) {
      gh_set_error("HODLR: an off-diagonal block of level %d needs a rank above %d to reach tol = %g (%s); the factorisation is not usable",
                   level, rc, h->opts.tol, user_cap ? "opts.max_rank" : "the solver's ceiling: loosen tol, raise min_size or use the dense solver");
      return user_cap ? GH_ERR_BAD_ARG : GH_ERR_RANK;
    }
    rc = std::min(2 * rc, RANK_CAP);
  }
}

// the 2R x C sums of a top level, completed over the ranks below the ancestor (HSub::allreduce)
int hm_allreduce(void* ctx, int level, double* dT, int rows, int cols, long pitch, hipStream_t st) {
  HmRank& r = *(HmRank*)ctx;
  gh_hodlr_mgpu_impl* H = r.owner;
  HmTop& t = *H->top[level][r.p >> (H->depth - level)];
  const size_t cnt = (size_t)rows * cols;
  if (cnt > r.pin_cap) {                      // (no other rank reads this one's buffer between two all-reduces; this rank's
    GH_HIP(hipStreamSynchronize(st));          //  own copy of the previous sums back to the device may still be in flight)
    if (r.pin) (void)hipHostFree(r.pin);
    r.pin = nullptr; r.pin_cap = 0;
    const size_t cap = std::max<size_t>(2 * cnt, 1 << 16);
    GH_HIP(hipHostMalloc((void**)&r.pin, 2 * cap * sizeof(double), hipHostMallocDefault));
    r.pin_cap = cap;
  }
  GH_HIP(hipMemcpy2DAsync(r.pin, cols * sizeof(double), dT, pitch * sizeof(double), cols * sizeof(double), rows, hipMemcpyDeviceToHost, st));
  GH_HIP(hipStreamSynchronize(st));
  r.pin_cnt = cnt;
  if (!t.bar.wait()) { gh_set_error("aborted: another device failed"); return GH_ERR_HIP; }
  double* sum = r.pin + r.pin_cap;
  for (int m = t.first; m < t.first + t.span; ++m) {            // fixed order: every rank adds up the same numbers the same way
    const HmRank& o = H->ranks[m];
    if (o.pin_cnt != cnt) { gh_set_error("HODLR split: ranks %d and %d disagree on the shape of a level-%d sum", r.p, m, level); H->abort.store(1); return GH_ERR_HIP; }
    if (m == t.first) memcpy(sum, o.pin, cnt * sizeof(double));
    else for (size_t e = 0; e < cnt; ++e) sum[e] += o.pin[e];
  }
  if (!t.bar.wait()) { gh_set_error("aborted: another device failed"); return GH_ERR_HIP; }
  GH_HIP(hipMemcpy2DAsync(dT, pitch * sizeof(double), sum, cols * sizeof(double), cols * sizeof(double), rows, hipMemcpyHostToDevice, st));
  return GH_OK;
}
int hm_local_done(void* ctx) {
  HmRank& r = *(HmRank*)ctx;
  if (r.dev_lock.owns_lock()) r.dev_lock.unlock();
  return GH_OK;
}

template <typename F>
int hm_run(gh_hodlr_mgpu_impl* H, F fn) {
  H->abort.store(0);
  H->world.reset();
  for (auto& lv : H->top) for (auto* t : lv) t->bar.reset();
  std::vector<std::thread> th;
  for (int i = 0; i < H->P; ++i) {
    th.emplace_back([H, i, &fn]() {
      HmRank& r = H->ranks[i];
      r.rc = GH_OK; r.err.clear();
      if (hipSetDevice(r.dev) != hipSuccess) { r.rc = GH_ERR_HIP; r.err = "hipSetDevice failed"; H->abort.store(1); return; }
      const int rc = fn(r);
      if (r.dev_lock.owns_lock()) r.dev_lock.unlock();
      if (rc != GH_OK) { r.rc = rc; r.err = gh_last_error(); H->abort.store(1); }
    });
  }
  for (auto& t : th) t.join();
  int first = GH_OK;
  for (auto& r : H->ranks) {
    if (r.rc == GH_OK) continue;
    if (first == GH_OK || r.err.find("aborted") == std::string::npos) {       // (prefer a real message to "saw the abort flag")
      first = r.rc;
      gh_set_error("sub-tree %d (device %d): %s", r.p, r.dev, r.err.c_str());
      if (r.err.find("aborted") == std::string::npos) break;
    }
  }
  return first;
}
}  // namespace

struct gh_hodlr_mgpu : gh_hodlr_mgpu_impl {};

extern "C" void gh_hodlr_mgpu_destroy(gh_hodlr_mgpu* H) {
  if (!H) return;
  H->clear_top();
  for (auto& r : H->ranks) {
    (void)hipSetDevice(r.dev);
    if (r.h) gh_hodlr_destroy(r.h);
    for (auto* b : r.stage) delete b;
    r.xg.release();
    if (r.kern.d_nodes) { (void)hipFree(r.kern.d_nodes); r.kern.d_nodes = nullptr; }
    if (r.pin) (void)hipHostFree(r.pin);
  }
  delete H;
}

extern "C" int gh_hodlr_mgpu_create(const gh_hodlr_mgpu_opts* opts, gh_hodlr_mgpu** out) {
  if (!opts || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  const int P = opts->n_dev;
  if (P < 1 || P > 16 || (P & (P - 1))) { gh_set_error("HODLR split: n_dev must be 1, 2, 4, 8 or 16 (got %d)", P); return GH_ERR_BAD_ARG; }
  const int ndev = gh_device_count();
  if (ndev <= 0) { gh_set_error("no HIP device available: the george_amd HODLR solver needs an MI355X"); return GH_ERR_HIP; }
  bool dup = false;
  for (int i = 0; i < P; ++i) {
    if (opts->devices[i] < 0 || opts->devices[i] >= ndev) { gh_set_error("HODLR split: device %d does not exist (%d visible)", opts->devices[i], ndev); return GH_ERR_BAD_ARG; }
    for (int j = 0; j < i; ++j) if (opts->devices[j] == opts->devices[i]) dup = true;
  }
  (void)dup;
  gh_hodlr_mgpu* H = new gh_hodlr_mgpu();
  H->opts = *opts;
  H->P = P;
  for (H->depth = 0; (1 << H->depth) < P; ++H->depth) {}
  H->ranks.resize(P);
  H->world.n = P;
  H->world.abort = &H->abort;
  for (int i = 0; i < P; ++i) {
    HmRank& r = H->ranks[i];
    r.p = i; r.dev = opts->devices[i]; r.owner = H;
    gh_hodlr_opts o;
    memset(&o, 0, sizeof(o));
    o.device = r.dev; o.min_size = opts->min_size; o.seed = opts->seed; o.max_rank = opts->max_rank; o.tol = opts->tol;
    const int rc = gh_hodlr_create(&o, &r.h);
    if (rc != GH_OK) { gh_hodlr_mgpu_destroy(H); return rc; }
    for (int l = 0; l < H->depth; ++l) r.stage.push_back(new GhBuf());
  }
  *out = H;
  return GH_OK;
}

// Host logic only (no device is touched): the rows of every sub-tree and, per level of the sub-trees, the index of each
// sub-tree's first internal node in the GLOBAL level (what keys a node's random stream) for a tree of n points split
// over n_dev devices.  seed_off: n_dev x max_levels, row-major, zero padded.  GH_ERR_BAD_ARG when a node above the split
// would be a leaf.  gh_hodlr_mgpu_compute lays its tree out through this function.
extern "C" int gh_hodlr_mgpu_layout(int64_t n, int32_t n_dev, int32_t min_size, int64_t* row0, int64_t* nrows,
                                    int32_t* seed_off, int32_t max_levels, int32_t* n_levels) {
  if (n <= 0 || n > 0x3fffffffL || n_dev < 1 || n_dev > 16 || (n_dev & (n_dev - 1)) || !row0 || !nrows) {
    gh_set_error("bad argument to layout"); return GH_ERR_BAD_ARG;
  }
  if (min_size < 1) min_size = 1;
  int depth = 0;
  while ((1 << depth) < n_dev) ++depth;
  struct Seg { int64_t start, size; };
  std::vector<Seg> cur(1, Seg{0, n});
  for (int l = 0; l < depth; ++l) {
    std::vector<Seg> next;
    for (const Seg& sg : cur) {
      const int64_t half = sg.size / 2;                      // hodlr.h:48: internal iff size / 2 >= min_size
      if (half < min_size) {
        gh_set_error("HODLR split: %lld points are too few for %d devices with min_size = %d (a node of level %d would be a leaf)",
                     (long long)n, n_dev, min_size, l);
        return GH_ERR_BAD_ARG;
      }
      next.push_back({sg.start, half});
      next.push_back({sg.start + half, sg.size - half});
    }
    cur.swap(next);
  }
  std::vector<std::vector<int>> cnt(n_dev);
  size_t maxl = 0;
  for (int p = 0; p < n_dev; ++p) {
    row0[p] = cur[p].start; nrows[p] = cur[p].size;
    std::vector<int64_t> sizes(1, cur[p].size);
    while (!sizes.empty()) {
      std::vector<int64_t> nx;
      int internal = 0;
      for (int64_t sz : sizes) if (sz / 2 >= min_size) { ++internal; nx.push_back(sz / 2); nx.push_back(sz - sz / 2); }
      if (internal == 0) break;
      cnt[p].push_back(internal);
      sizes.swap(nx);
    }
    maxl = std::max(maxl, cnt[p].size());
  }
  if (n_levels) *n_levels = (int32_t)maxl;
  if (seed_off) {
    for (int p = 0; p < n_dev; ++p)
      for (int l = 0; l < max_levels; ++l) {
        int v = 0;
        for (int o = 0; o < p; ++o) if ((size_t)l < cnt[o].size()) v += cnt[o][l];
        seed_off[(size_t)p * max_levels + l] = v;
      }
  }
  return GH_OK;
}

extern "C" int gh_hodlr_mgpu_compute(gh_hodlr_mgpu* H, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                                     const double* yerr, double* logdet_out) {
  if (!H || !k || !x || !yerr || n <= 0) { gh_set_error("bad argument to compute"); return GH_ERR_BAD_ARG; }
  if (ndim != k->ndim) { gh_set_error("dimension mismatch"); return GH_ERR_DIM; }
  if (n > 0x3fffffffL) { gh_set_error("HODLR: n too large"); return GH_ERR_BAD_ARG; }
  if (gh_is_device_ptr(x) || gh_is_device_ptr(yerr)) { gh_set_error("HODLR split: x and yerr must be host pointers"); return GH_ERR_BAD_ARG; }
  H->computed = false;
  H->n = n; H->ndim = ndim;
  const int P = H->P, depth = H->depth, min_size = std::max(1, H->opts.min_size);
  // ---- the tree above the split (hodlr.h:47-64) and the rows of every sub-tree
  // (kept from one compute() to the next while n is the same: a top node holds 8 N rcap bytes of ACA scratch)
  const bool keep_top = H->top_n == n && H->top_min == min_size && (int)H->top.size() == depth;
  H->top_n = -1;
  if (!keep_top) { H->clear_top(); H->top.resize(depth); }
  struct Seg { int start, size; };
  std::vector<Seg> cur(1, Seg{0, (int)n});
  for (int l = 0; l < depth; ++l) {
    std::vector<Seg> next;
    for (int q = 0; q < (int)cur.size(); ++q) {
      const int half = cur[q].size / 2;
      if (half < min_size) {
        gh_set_error("HODLR split: %lld points are too few for %d devices with min_size = %d (a node of level %d would be a leaf)",
                     (long long)n, P, min_size, l);
        H->clear_top();
        return GH_ERR_BAD_ARG;
      }
      if (!keep_top) {
        HmTop* t = new HmTop();
        t->level = l; t->q = q; t->start = cur[q].start; t->half = half; t->size = cur[q].size;
        t->span = P >> l; t->first = q * t->span; t->runner = t->first + (l % t->span);
        t->bar.n = t->span; t->bar.abort = &H->abort;
        H->top[l].push_back(t);
      }
      next.push_back({cur[q].start, half});
      next.push_back({cur[q].start + half, cur[q].size - half});
    }
    cur.swap(next);
  }
  // rows of every sub-tree, and where its nodes sit in the global levels (a node's random stream is keyed by that)
  {
    int64_t r0[16], nr[16];
    int32_t nl = 0;
    GH_CHECK(gh_hodlr_mgpu_layout(n, P, min_size, r0, nr, nullptr, 0, &nl));
    std::vector<int32_t> so((size_t)P * std::max(nl, 1), 0);
    GH_CHECK(gh_hodlr_mgpu_layout(n, P, min_size, r0, nr, so.data(), nl, &nl));
    for (int p = 0; p < P; ++p) {
      H->ranks[p].row0 = (long)r0[p]; H->ranks[p].n = (long)nr[p];
      H->ranks[p].seed_off.assign(so.begin() + (size_t)p * nl, so.begin() + (size_t)(p + 1) * nl);
    }
  }
#ifdef GH_HODLR_PHASE_MARKS
  const bool dbg = true;
#else
  const bool dbg = false;
#endif
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
  const int rc = hm_run(H, [&](HmRank& r) -> int {
    gh_hodlr* h = r.h;
    hipStream_t st = h->st;
    double tm[6] = {0, 0, 0, 0, 0, 0};
    struct Report { bool on; int p; double* tm; ~Report() { if (on) fprintf(stderr, "[hodlr split] rank %d: top ACA done %.2f, met %.2f, rows pulled %.2f, met %.2f, lock %.2f, compute returned %.2f ms\n", p, tm[0], tm[1], tm[2], tm[3], tm[4], tm[5]); } } report{dbg, r.p, tm};
    // a private copy of the kernel program on this device (a gh_kernel caches ONE device copy)
    if (r.kern.d_nodes) { (void)hipFree(r.kern.d_nodes); r.kern.d_nodes = nullptr; }
    r.kern.nodes = k->nodes; r.kern.ndim = k->ndim; r.kern.size = k->size; r.kern.fast = k->fast; r.kern.device = -1;
    GH_CHECK(r.kern.upload());
    // ---- the ACA of the top nodes this device runs
    std::vector<HmTop*> mine;
    for (auto& lv : H->top) for (auto* t : lv) if (t->runner == r.p) mine.push_back(t);
    if (!mine.empty()) {
      GH_CHECK(r.xg.ensure((size_t)n * ndim * sizeof(double)));
      GH_CHECK(gh_to_device(r.xg.d(), x, (size_t)n * ndim, st));
      std::lock_guard<std::mutex> lk(g_hm_dev_mu[r.dev & 15]);
      for (HmTop* t : mine) {
        GH_CHECK(aca_top_node(h, &r.kern, r.xg.d(), (long)n, ndim, t->level, LvlNode{t->start, t->half, t->size, t->q}, t->Tcm, &t->rank));
        t->pack_off.assign(t->span, 0);
        GH_CHECK(t->packed.ensure(std::max<size_t>((size_t)t->size * t->rank, 1) * sizeof(double)));
        long off = 0;
        for (int m = 0; m < t->span && t->rank > 0; ++m) {
          const HmRank& o = H->ranks[t->first + m];
          t->pack_off[m] = off;
          const long tot = o.n * t->rank;
          hipLaunchKernelGGL(hodlr_pack_rows_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 4096)), dim3(256), 0, st,
                             t->Tcm.d(), (long)n, o.row0, o.n, t->rank, t->packed.d() + off);
          off += tot;
        }
        GH_HIP(hipGetLastError());
      }
      GH_HIP(hipStreamSynchronize(st));
    }
    tm[0] = ms_since();
    if (!H->world.wait()) { gh_set_error("aborted: another device failed"); return GH_ERR_HIP; }
    tm[1] = ms_since();
    // ---- every device pulls its rows of each ancestor's factors
    HSub& sub = h->sub;
    sub.depth = depth;
    sub.half.assign(depth, 0); sub.R.assign(depth, 0); sub.T.assign(depth, nullptr);
    sub.seed_off = r.seed_off;
    sub.ctx = &r; sub.allreduce = hm_allreduce; sub.local_done = hm_local_done;
    for (int l = 0; l < depth; ++l) {
      int R = 0;
      for (auto* t : H->top[l]) R = std::max(R, t->rank);
      HmTop* t = H->top[l][r.p >> (depth - l)];
      sub.R[l] = R;
      sub.half[l] = (r.row0 >= t->start + t->half) ? 1 : 0;
      GhBuf* sg = r.stage[l];
      GH_CHECK(sg->ensure(std::max<size_t>((size_t)r.n * R, 1) * sizeof(double)));
      sub.T[l] = sg->d();
      if (R > t->rank) GH_HIP(hipMemsetAsync(sg->d() + (size_t)r.n * t->rank, 0, (size_t)r.n * (R - t->rank) * sizeof(double), st));
      if (t->rank > 0) {
        const double* src = t->packed.d() + t->pack_off[r.p - t->first];
        const size_t bytes = (size_t)r.n * t->rank * sizeof(double);
        const int sdev = H->ranks[t->runner].dev;
        if (sdev == r.dev) GH_HIP(hipMemcpyAsync(sg->p, src, bytes, hipMemcpyDeviceToDevice, st));
        else GH_HIP(hipMemcpyPeerAsync(sg->p, r.dev, src, sdev, bytes, st));
      }
    }
    GH_HIP(hipStreamSynchronize(st));
    tm[2] = ms_since();
    if (!H->world.wait()) { gh_set_error("aborted: another device failed"); return GH_ERR_HIP; }
    tm[3] = ms_since();
    // ---- the sub-tree: the single-device code (released for the next sub-tree of this device once its own part is done)
    r.dev_lock = std::unique_lock<std::mutex>(g_hm_dev_mu[r.dev & 15]);
    tm[4] = ms_since();
    const int rcc = gh_hodlr_compute(h, &r.kern, x + r.row0 * ndim, r.n, ndim, yerr + r.row0, &r.ld);
    tm[5] = ms_since();
    return rcc;
  });
  if (rc != GH_OK) return rc;
  // log|det|: the sub-trees' own blocks in tree order, then the ancestors' cores bottom-up (each from the first device below it)
  double logdet = 0.0;
  for (auto& r : H->ranks) logdet += r.ld;
  for (int l = depth - 1; l >= 0; --l)
    for (auto* t : H->top[l]) logdet += H->ranks[t->first].h->sub.ld_top[l];
  H->logdet = logdet;
  // ranks, level by level
  H->all_ranks.clear();
  for (int l = 0; l < depth; ++l) for (auto* t : H->top[l]) H->all_ranks.push_back(t->rank);
  for (size_t l = depth;; ++l) {
    bool any = false;
    for (auto& r : H->ranks)
      if (l < r.h->levels.size()) { any = true; for (int v : r.h->levels[l]->ranks) H->all_ranks.push_back(v); }
    if (!any) break;
  }
  H->computed = true;
  H->top_n = n; H->top_min = min_size;
  if (logdet_out) *logdet_out = logdet;
  return GH_OK;
}

extern "C" int gh_hodlr_mgpu_solve(gh_hodlr_mgpu* H, const double* b, int64_t nrhs, double* out) {
  if (!H) { gh_set_error("null solver"); return GH_ERR_BAD_ARG; }
  if (!H->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  if (!b || !out || nrhs <= 0) { gh_set_error("bad argument to solve"); return GH_ERR_BAD_ARG; }
  if (gh_is_device_ptr(b) || gh_is_device_ptr(out)) { gh_set_error("HODLR split: b and out must be host pointers"); return GH_ERR_BAD_ARG; }
  // (n, nrhs) row-major: the rows of a sub-tree are one contiguous slice
  return hm_run(H, [&](HmRank& r) -> int { return gh_hodlr_solve(r.h, b + r.row0 * nrhs, nrhs, out + r.row0 * nrhs); });
}
extern "C" int gh_hodlr_mgpu_dot_solve(gh_hodlr_mgpu* H, const double* y, double* out) {
  if (!H || !y || !out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  if (!H->computed) { gh_set_error("you must call 'compute' first"); return GH_ERR_NOT_COMPUTED; }
  std::vector<double> a((size_t)H->n);
  GH_CHECK(gh_hodlr_mgpu_solve(H, y, 1, a.data()));
  double v = 0.0;
  for (int64_t i = 0; i < H->n; ++i) v += y[i] * a[i];
  *out = v;
  return GH_OK;
}
extern "C" int gh_hodlr_mgpu_ranks(const gh_hodlr_mgpu* H, int32_t* ranks_out, int32_t max_out, int32_t* n_out) {
  if (!H || !n_out) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  int cnt = 0;
  for (int v : H->all_ranks) { if (ranks_out && cnt < max_out) ranks_out[cnt] = v; ++cnt; }
  *n_out = cnt < max_out ? cnt : max_out;
  return GH_OK;
}
extern "C" int gh_hodlr_mgpu_rows(const gh_hodlr_mgpu* H, int64_t* row0, int64_t* nrows) {
  if (!H || !row0 || !nrows) { gh_set_error("null argument"); return GH_ERR_BAD_ARG; }
  for (int p = 0; p < H->P; ++p) { row0[p] = H->ranks[p].row0; nrows[p] = H->ranks[p].n; }
  return GH_OK;
}
