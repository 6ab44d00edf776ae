// gh_hodlr_impl.h -- what the five units of the HODLR solver share (host side, private to them):
//   gh_hodlr.hip          the factorisation: handle, tree, leaf stage, Gauss-Jordan and core kernels, compaction, compute()
//   gh_hodlr_aca.hip      the ACA kernels (a workgroup or a cluster per node; a wavefront per node) and their launchers
//   gh_hodlr_apply.hip    applying a factor to right-hand sides: the small dense products, apply / solve, solve .. get_inverse
//   gh_hodlr_predict.hip  predict and the likelihood gradient on a computed factor, over column strips (predict's strip loop and
//                         column reduction are the ones all solvers share: gh_predict.hip, declared in gh_common.h)
//   gh_hodlr_mgpu.hip     the tree split over several devices (gh_hodlr_mgpu_*)
// A kernel is launched only from the unit that defines it; what another unit needs of it is a launcher declared here.
#pragma once
#include <string.h>
#include <algorithm>
#include <vector>
#include "gh_common.h"

#define HCH 128          // rows per reduce/update chunk
#define CPASS 256        // columns handled per pass of an apply
#define RANK_CAP 1024    // hard ceiling on a block's ACA rank (scratch n x rank, 2 rank x 2 rank cores)
#define ACA_THREADS 512        // workgroup size of hodlr_aca_kernel (the cluster rule counts columns per thread)
#define ACA_MAXR 2048          // coefficient slots in LDS: rank <= 2048 (one-workgroup nodes) / 1024 (clusters)
#define MV_C 8                 // the narrow kernels (hodlr_mv_*) take up to this many right-hand sides
#define SUM_NS 8               // hodlr_sum_kernel: slices of a node's chunks summed side by side (hodlr_core_kernel keeps its order)

// ------------------------------------------------------------------ device structs
struct LvlNode { int start, half, size, pad; };      // pad: added to the node's index where the ACA seeds its generator
struct Chunk { int node, half, row0, nrows; };
struct MMJob { long a_off; int b_row, o_row, m, kd; };
struct LeafDesc { int start, size; long off; };

// Several levels in ONE launch of hodlr_aca_kernel: workgroups [wg0, wg0 + nwg) work on the level described by a segment
// (the per-level arguments of the kernel are then taken from it).  The clustered levels of a tree
// are launched this way, 256 workgroups in all, so that every cluster is resident whatever the
// others do; launched one after the other they were 3 of the 9 ms of a C4 compute().
struct AcaSeg {
  const LvlNode* nodes; double* Tcm; int* idx; int* ranks; unsigned* bars; double* part; int* sel; int* fail; int* trunc;
  int level, G, wg0, nwg;
  // one-workgroup segments: dur[node] <- how long the node took (10-ns ticks); order != nullptr: workgroup q of the segment takes
  // node order[q] (the host's longest-first order from the previous compute() of the handle)
  int* dur; const int* order;
};
// (round 6) The factorisation's leaf product takes its input -- the un-factored U, which is V: the compaction writes the same values
// to both -- from the LEVEL-MAJOR copy VA (level l, row i, column k at VA[offv[l] + i R[l] + k]; a leaf's rows of a level are one
// contiguous piece) and writes the row-major U for the first time: the compaction no longer writes U (157 MB at C4) for this
// kernel to read back.  Same values in the same LDS image: the same bits.
struct LeafSrc { const double* VA; int nlev; int off[24], R[24]; long offv[24]; };

// ================================================================================ host side
struct HNode { int start, size, half, level, is_leaf; };
struct HLevel {
  int top_level = -1;
  bool top = false;                 // pseudo-level of a sub-tree handle (HSub below): one node, the ancestor cut down to the local rows
  std::vector<int> node_ids;
  int R = 0, off = 0, nchunks = 0;
  GhPooledBuf d_nodes, d_chunks, d_crange, d_red_jobs, d_upd_jobs, d_smul_jobs, d_ranks, sinv;   // (one stream: h->st)
  GhPooledBuf d_gj_offs, d_gj_sizes, d_gj_sc, d_updl_jobs;
  std::vector<int> ranks;
  // The job tables depend on the tree and on (R, off, Rtot) only: inside an optimiser loop neither
  // changes from one compute() to the next, and re-uploading them (~9 small copies per level, each a
  // host round trip) was ~1 ms of the 12 ms of a C4 compute.
  std::vector<int> chunk_geom;      // (row0, rows) of every chunk in order: two levels with the same list can share a pass over the rows
  bool nodes_up = false;
  std::vector<int> aca_dur;         // per node: ticks its one-workgroup ACA took in the last compute() (empty: unknown)
  GhPooledBuf d_order;              // the node order the next one-workgroup launch takes them in (longest first)
  int tab_R = -1, tab_off = -1, gj_R = -1;
  long tab_Rtot = -1;
};

// A handle can be ONE SUB-TREE of a tree that is split over several devices (gh_hodlr_mgpu.hip): its
// rows are rows [row0, row0 + n) of the whole problem, its tree is the sub-tree rooted at global level `depth`, and the
// `depth` levels above it appear here as PSEUDO-LEVELS of one node each -- the ancestor at that level, cut down to the
// local rows (which all lie in ONE of its halves).  Their low-rank factors are not computed here (the ACA of a top node
// runs on one device; T[l] holds the local rows of its result), and whenever such a level is applied, the 2R x C sums
// V^T X are completed over the devices below that ancestor (`allreduce`) between "sum" and "core product".  Everything
// else -- tables, kernels, the order of the sweep -- is the single-device code.
struct HSub {
  int depth = 0;                    // 0: an ordinary handle
  std::vector<int> half, R;         // [depth] the half of the level-l ancestor the local rows are in; the rank of global level l
  std::vector<const double*> T;     // [depth] column-major n x R[l]: local rows of the ancestor's ACA factors (this device)
  std::vector<int> seed_off;        // per local level: index of this sub-tree's first internal node in the global level
  void* ctx = nullptr;
  int (*allreduce)(void* ctx, int level, double* dT, int rows, int cols, long pitch, hipStream_t st) = nullptr;
  int (*local_done)(void* ctx) = nullptr;      // the part of compute() that needs no other device has been enqueued and has finished
  std::vector<double> ld_top;       // out: log|det| of the core of the level-l ancestor (every device below it computes the same)
  std::vector<int> sig() const { std::vector<int> v{depth}; v.insert(v.end(), half.begin(), half.end()); v.insert(v.end(), seed_off.begin(), seed_off.end()); return v; }
};

struct gh_hodlr {
  gh_hodlr_opts opts;
  HSub sub;
  std::vector<int> tree_sub;        // sub.sig() the tree was built for
  hipStream_t st = nullptr;
  GhBuf d_gather;                   // (fetch of every level's ranks / flags in one copy)
  int* h_gather = nullptr; size_t h_gather_cap = 0;      // pinned
  bool shared_streams = false;   // st, st_b, st_c belong to the process (gh_shared_streams, gh_common.h): not destroyed here
  hipStream_t st_b = nullptr;    // second stream: ACA of the one-workgroup-per-node levels beside the clustered ones
  hipEvent_t ev_b = nullptr;
  hipStream_t st_d = nullptr;    // fourth queue (the process-wide chain stream): one more independent ACA chain at a time
  hipEvent_t ev_d = nullptr;
  hipStream_t st_c = nullptr;    // third stream: the leaf stage, beside both ACA streams
  hipEvent_t ev_c = nullptr;
  std::vector<hipEvent_t> aca_ev;        // timing stamps of the side items of the last compute(), two per item
  size_t aca_ev_used = 0;
  std::vector<int> aca_items;            // level per item (-1: leaf stage), in stamp order
  hipEvent_t aca_fused_ev[2] = {nullptr, nullptr};
  bool aca_timed = false;
  std::vector<double> aca_ms;            // measured milliseconds: [0..nlev) levels, [nlev] fused launch, [nlev+1] leaf stage
  std::vector<char> wave_bad;            // per level: a block needed more columns than the wavefront-per-node ACA holds (hodlr_aca_wave_kernel): the workgroup kernel from then on
  int64_t n = 0;
  int ndim = 0;
  bool computed = false;
  double logdet = 0.0;
  std::vector<HNode> nodes;
  std::vector<HLevel*> levels;
  std::vector<LeafDesc> leaves;
  int Rtot = 0, max_leaf = 0, max_chunks = 0, maxR = 0;
  int leaf_pitch = 0;            // row pitch of the stored leaf inverses
  int cpass = CPASS;             // columns per apply pass = row pitch of P / Tsum / Tout / Y (>= the largest level rank)
  GhBuf x, yerr, UA, VA, leaf_inv, d_leaves, d_leaf_jobs, P, Tsum, Tout, Y, rhs, scal, work, dotp;
  GhBuf d_leaf_prod;
  GhBuf d_aca_segs, d_aca_segs1;
  double* pin = nullptr;         // pinned host block for the results compute() brings back (log|det| of every block, flags)
  size_t pin_doubles = 0;
  GhBuf UL, d_colbase, d_colld;  // level-major copy of the final U (wide solves: ensure_ul) and its column map
  bool ul_valid = false;
  long col_Rtot = -1;
  std::vector<int> col_sig;
  GhBuf ld_all, flags;           // log|det| of every factored block of a compute(); [0] Gauss-Jordan failure, [2..3] leaf info
  ~gh_hodlr() {
    for (auto* l : levels) delete l;
    if (h_gather) (void)hipHostFree(h_gather);
    if (ev_b) (void)hipEventDestroy(ev_b);
    if (st_b && !shared_streams) (void)hipStreamDestroy(st_b);
    if (ev_c) (void)hipEventDestroy(ev_c);
    if (ev_d) (void)hipEventDestroy(ev_d);
    if (st_c && !shared_streams) (void)hipStreamDestroy(st_c);
    for (auto& e : aca_ev) (void)hipEventDestroy(e);
    for (auto& e : aca_fused_ev) if (e) (void)hipEventDestroy(e);
    if (st && !shared_streams) (void)hipStreamDestroy(st);
  }
  int64_t tree_n = -1;
  int tree_min = -1;
  bool leaf_tab_up = false;
  void reset_tree() { for (auto* l : levels) delete l; levels.clear(); nodes.clear(); leaves.clear(); tree_n = -1; leaf_tab_up = false; col_Rtot = -1; col_sig.clear(); aca_ms.clear(); wave_bad.clear(); }
};

template <typename Tv>
static int upload(GhBuf& buf, const std::vector<Tv>& v, hipStream_t st) {
  GH_CHECK(buf.ensure(std::max<size_t>(v.size(), 1) * sizeof(Tv)));
  if (!v.empty()) GH_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(Tv), hipMemcpyHostToDevice, st));
  return GH_OK;
}

// ---- gh_potf2.hip: the batched 128x128 Cholesky + inverse of the factor (gh_launch_potf2_batched, gh_common.h) in its leaf form: block b -> K_b^-1 (full symmetric, in place) and logdet[b] = log|K_b|, nothing else written
int gh_launch_potf2_kinv_batched(double* A, int64_t lda, int64_t stride_a, double* logdet, long long* info, int nbatch, hipStream_t st);
int gh_launch_potf2_kinv_kernel_batched(double* A, int64_t lda, int64_t stride_a, double* logdet, long long* info, int nbatch,
                                        const GhFast& fast, const double* x, const double* yerr, int nd, const void* leaves, hipStream_t st);

// ---- gh_hodlr_aca.hip
// One launch of hodlr_aca_kernel: the nodes of ONE level (nodes .. trunc, level, G) or a table of segments (segs, nseg; the
// per-level fields null / 0 / G = 1), nwg workgroups in all.  ones_only: one workgroup per node throughout -- the instantiation
// without the cluster protocol, with the LDS mirrors.  tol, seed and the kernel program come from the handle and k.
struct AcaLaunch {
  const double* x; long N; int ndim;         // the points the blocks are evaluated on
  const LvlNode* nodes; double* Tcm; int* idx; int* ranks; unsigned* bars; double* part; int* sel; int* fail; int* trunc;
  const AcaSeg* segs; int nseg;
  int nwg, G, level, rc, pstride, multi, fence;
  bool ones_only;
};
int hodlr_launch_aca(const gh_hodlr* h, const gh_kernel* k, const AcaLaunch& a, hipStream_t st);
// the nn nodes of a level whose blocks have at most mr = 64 / 128 / 256 rows and columns through hodlr_aca_wave_kernel
int hodlr_launch_aca_wave(const gh_hodlr* h, const gh_kernel* k, int ndim, const LvlNode* nodes, int nn, int mr, double* Tcm, long N,
                          int rc, int* ranks, int level, int* trunc, hipStream_t st);

// ---- gh_hodlr_apply.hip
int hodlr_need(gh_hodlr* h);                                     // null handle, not computed, or the device cannot be set
int hodlr_passes();                                              // gh_debug_set_hodlr_passes' mask as it is now
// mtiles: 32-row tiles of a job handled by ONE workgroup
int hodlr_launch_mm(gh_hodlr* h, hipStream_t st, const MMJob* jobs, int njobs, int max_m, const double* A, long a_rs, long a_cs,
                    const double* B, long ldb, long b_col0, double* O, long ldo, long o_col0, int C, bool subtract, int mtiles = 1);
int hodlr_launch_red(gh_hodlr* h, const MMJob* jobs, int njobs, int R, const double* V, const double* B, long ldb, long b_col0,
                     double* O, long ldo, long o_col0, int C);
int hodlr_launch_upd(gh_hodlr* h, const MMJob* jobs, int njobs, int R, const double* A, long a_rs, const double* B, long ldb,
                     double* O, long ldo, int C);
bool hodlr_updred_possible(int passes, const HLevel* L, const HLevel* nx, int C, int cpass);
int hodlr_launch_updred(gh_hodlr* h, const HLevel* L, const HLevel* nx, const double* A, long a_rs, const double* B, long ldb,
                        double* O, long ldo, int C, const double* V2, double* P, long ldp);
// h->Tsum = the chunk partials in h->P added up per node and half, C columns, on h->st (hodlr_sum_kernel); S = the cores built from Tsum
int hodlr_launch_sum(gh_hodlr* h, const HLevel* L, int C);
int hodlr_launch_sbuild(const double* Tsum, long Cp, int R, double* S, int nb, hipStream_t st);
// columns [col0, col0 + cw) of the identity into the n x ld strip at p (the rest of the strip is the caller's)
int hodlr_launch_eye_strip(double* p, long ld, long col0, int cw, hipStream_t st);
int hodlr_apply_level(gh_hodlr* h, HLevel* L, double* X, long ldx, long xcol0, int C, const double* U, long ldu);
int hodlr_apply_leaves(gh_hodlr* h, int passes, double* X, long ldx, long xcol0, int C, const HLevel* red = nullptr, bool* red_done = nullptr,
                       const LeafSrc* src = nullptr);
int hodlr_solve_all(gh_hodlr* h, int passes, double* X, long ldx, int C);
