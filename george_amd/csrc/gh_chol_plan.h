// gh_chol_plan.h -- the launch list of the two-level dense Cholesky driver, as data (host C++ only: no device, no HIP).
//
// The inner panels (panel_starts(): 2048, later 1024 columns) stay the unit of the potf2/TRSM chain; the unit of the
// trailing update is a GROUP of consecutive inner panels, so that the far update runs with K = the group's width
// (the GEMM kernel's rate follows K: a tile has a fixed cost of 50-60 k-steps).  For a group G = [a, b) of panels and
// the next group G' = [b, b'), with c0(j) the first column of panel j:
//   chain stream, j = a .. b-1:
//     L(j)  (j > a)  block column j from its diagonal block down -= the in-group panels a .. j-1, ONE launch, K = c0(j) - c0(a)
//     PANEL(j)       panel_step(): diagonal block factored, rows below solved
//   chain stream:  T(G)  the lower trapezoid "rows >= c0(b), columns of G'" -= the whole group, K = c0(b) - c0(a)
//   main stream:   F(G)  the lower triangle from column c0(b') on         -= the whole group, same K; after PANEL(b-1)
// Who writes a column of group i, in order: F(G_0) ... F(G_i-2) (main stream order), T(G_i-1) (waits for F(G_i-2)'s event),
// L (chain order).  So every column receives every earlier panel's k-range exactly once, ascending: the factor has the
// same bits as with one launch per panel.  With every group one panel wide the list is the one-level schedule
// (T = U(j, j+1), F = W(j)).
//
// A wrong wait in such a driver does not fail, it flips low bits once in a while; so the driver executes THIS list and
// nothing else, and tests/test_chol_plan.py replays the list on a CPU (gh_debug_chol_plan).
#ifndef GH_CHOL_PLAN_H_
#define GH_CHOL_PLAN_H_
#include <stdint.h>
#include <algorithm>
#include <vector>

enum { GH_PLAN_PANEL = 0, GH_PLAN_L = 1, GH_PLAN_T = 2, GH_PLAN_F = 3, GH_PLAN_JOIN = 4 };
enum { GH_PLAN_MAIN = 0, GH_PLAN_CHAIN = 1 };
#define GH_PLAN_COLS 12        // int64 per op in gh_debug_chol_plan's output, in the order of the fields below

struct GhPlanOp {
  int64_t kind, stream;
  int64_t r0, r1, c0, c1;      // what the op writes: rows [r0, r1) x columns [c0, c1) of the lower triangle (r0 == c0)
  int64_t k0, k1;              // the columns of L it reads as the K range (PANEL: its own columns; JOIN: empty)
  int64_t wait0, wait1;        // events (indices) its stream waits for before it, -1: none
  int64_t record;              // event recorded on its stream after it, -1: none
  int64_t lower;               // update ops: 1 = launched as a lower trapezoid, 0 = as the full rectangle (tiles above the
                               // diagonal computed and never read; what one-panel block columns of <= 128 tiles always were)
};
struct GhCholPlan {
  int64_t np = 0;
  int gmax = 0;
  double hide = 0.0;
  std::vector<int64_t> pc;     // panel starts, pc[P] = np
  std::vector<int> gs;         // first panel of every group, gs.back() = P
  std::vector<GhPlanOp> ops;
  int n_events = 0;
};

// Start columns of the inner panels: `nb` columns, or 2 * nb while at least `bound` columns of trailing matrix lie
// behind such a panel (bound <= 0: nb throughout).
static inline std::vector<int64_t> gh_plan_panel_starts(int64_t np, int64_t nb, int64_t bound, int64_t tier2 = 0) {
  std::vector<int64_t> pc;
  for (int64_t k0 = 0; k0 < np;) {
    pc.push_back(k0);
    int64_t w = (bound > 0 && np - (k0 + 2 * nb) >= bound) ? 2 * nb : nb;
    if (tier2 > 0 && bound > 0 && np - (k0 + 4 * nb) >= tier2) w = 4 * nb;
    k0 += std::min<int64_t>(w, np - k0);
  }
  pc.push_back(np);
  return pc;
}

static inline double gh_plan_trap_tiles(int64_t m, int64_t n) {      // 128 x 128 tiles of an m x n lower trapezoid
  const double tm = (double)(m / 128), tn = (double)(n / 128);
  return tn * (tn + 1.0) / 2.0 + (tm - tn) * tn;
}

// The groups.  Group 0 is panel 0 alone (the main stream waits for no more than the first panel, as in the one-level
// schedule); after it the size doubles (2, 4, ...) up to gmax, and every group is cut back to what the far update running
// beside its chain hides: the chain of G' -- its panels, its L launches and T(G') -- runs while the main stream executes
// F(G).  Estimates in ms: the far update at GH_PLAN_FAR_TFLOPS, the chain's GEMMs, which share the chip with it, at
// GH_PLAN_CHAIN_TFLOPS (block-column updates beside a wide launch: 48-54 TFLOP/s early, ~40 late,
// profiles/r06/update_intervals_N65536.json), a 128-column link of a panel at GH_PLAN_LINK_MS (potf2 + its two K = 128
// GEMMs beside a wide launch).  A group is kept while chain <= hide * far (GH_PLAN_HIDE unless a test or a sweep says
// otherwise).  T's cost grows with the square of the group width, which is what ends the growth; as the trailing matrix
// shrinks (far ~ m^2, chain ~ m) the groups fall back to single panels, i.e. to the one-level schedule.  The rule only
// moves time: the bits do not depend on it.  Margin and maximum swept in profiles/two_level/ (DESIGN.md section 4).
#ifndef GH_PLAN_FAR_TFLOPS
#define GH_PLAN_FAR_TFLOPS 66.0
#endif
#ifndef GH_PLAN_CHAIN_TFLOPS
#define GH_PLAN_CHAIN_TFLOPS 45.0
#endif
#ifndef GH_PLAN_LINK_MS
#define GH_PLAN_LINK_MS 0.6
#endif
#ifndef GH_PLAN_HIDE
#define GH_PLAN_HIDE 1.2
#endif
static inline std::vector<int> gh_plan_groups(int64_t np, const std::vector<int64_t>& pc, int gmax, double hide) {
  const int P = (int)pc.size() - 1;
  std::vector<int> gs;
  if (gmax <= 1) {
    for (int j = 0; j <= P; ++j) gs.push_back(j);
    return gs;
  }
  const double tile_fl = 2.0 * 128.0 * 128.0;
  gs.push_back(0);
  int a = 0, b = 1, prev = 1;
  while (b < P) {
    int g = std::min(std::min(gmax, 2 * prev), P - b);
    for (; g > 1; --g) {
      const int e = b + g;                                         // G' = [b, e)
      const int64_t kg = pc[b] - pc[a];                            // K of F(G), G = [a, b)
      const double far_ms = gh_plan_trap_tiles(np - pc[e], np - pc[e]) * tile_fl * (double)kg / (GH_PLAN_FAR_TFLOPS * 1e9);
      double chain_fl = 0.0, links = 0.0;
      for (int j = b; j < e; ++j) {
        links += (double)((pc[j + 1] - pc[j] + 127) / 128);
        if (j > b) chain_fl += gh_plan_trap_tiles(np - pc[j], pc[j + 1] - pc[j]) * tile_fl * (double)(pc[j] - pc[b]);
      }
      const int64_t wnext = std::min<int64_t>(pc[e] - pc[b], np - pc[e]);    // (the group after G' is not chosen yet: as wide as G')
      chain_fl += gh_plan_trap_tiles(np - pc[e], wnext) * tile_fl * (double)(pc[e] - pc[b]);
      const double chain_ms = links * GH_PLAN_LINK_MS + chain_fl / (GH_PLAN_CHAIN_TFLOPS * 1e9);
      if (chain_ms <= hide * far_ms) break;
    }
    gs.push_back(b);
    a = b; b += g; prev = g;
  }
  gs.push_back(P);
  return gs;
}

static inline GhCholPlan gh_plan_build(int64_t np, const std::vector<int64_t>& pc, int gmax, double hide = GH_PLAN_HIDE) {
  GhCholPlan pl;
  if (!(hide > 0.0)) hide = GH_PLAN_HIDE;
  pl.np = np; pl.gmax = gmax; pl.hide = hide; pl.pc = pc;
  pl.gs = gh_plan_groups(np, pc, gmax, hide);
  const int G = (int)pl.gs.size() - 1;
  int nev = 0;
  int64_t ev_far_prev = -1;                                        // event of F(G_i-1)
  auto update = [&](int kind, int stream, int64_t c0, int64_t c1, int64_t k0, int64_t k1) {
    GhPlanOp o{};
    o.kind = kind; o.stream = stream; o.r0 = c0; o.r1 = np; o.c0 = c0; o.c1 = c1; o.k0 = k0; o.k1 = k1;
    o.wait0 = o.wait1 = o.record = -1;
    // (a launch of at most 128 lower tiles keeps the rectangular form the one-level driver gives it: gh_launch_gemm sends
    //  small rectangles and small trapezoids to different kernels)
    o.lower = gh_plan_trap_tiles(np - c0, c1 - c0) > 128.0 ? 1 : 0;
    return o;
  };
  for (int i = 0; i < G; ++i) {
    const int a = pl.gs[i], b = pl.gs[i + 1];
    int64_t ev_panel = -1;
    for (int j = a; j < b; ++j) {
      if (j > a) pl.ops.push_back(update(GH_PLAN_L, GH_PLAN_CHAIN, pc[j], pc[j + 1], pc[a], pc[j]));
      GhPlanOp p{};
      p.kind = GH_PLAN_PANEL; p.stream = GH_PLAN_CHAIN;
      p.r0 = pc[j]; p.r1 = np; p.c0 = pc[j]; p.c1 = pc[j + 1]; p.k0 = pc[j]; p.k1 = pc[j + 1];
      p.wait0 = p.wait1 = p.record = -1; p.lower = 1;
      if (j == b - 1) p.record = ev_panel = nev++;                 // what F(G) waits for; the last one of all: the join
      pl.ops.push_back(p);
    }
    if (i + 1 < G) {
      // (T(G) on the main stream in front of F(G) instead was measured and lost: profiles/two_level/sweep_65536.md)
      GhPlanOp t = update(GH_PLAN_T, GH_PLAN_CHAIN, pc[b], pc[pl.gs[i + 2]], pc[a], pc[b]);
      t.wait0 = ev_far_prev;                                       // F(G_i-1) wrote these columns (-1: there is none)
      pl.ops.push_back(t);
      if (i + 2 < G) {
        const int64_t cf = pc[pl.gs[i + 2]];
        GhPlanOp f = update(GH_PLAN_F, GH_PLAN_MAIN, cf, np, pc[a], pc[b]);
        f.lower = 1;
        f.wait0 = ev_panel;
        f.record = ev_far_prev = nev++;
        pl.ops.push_back(f);
      } else {
        ev_far_prev = -1;                                          // (the last T has been ordered behind the last F already)
      }
    } else {
      GhPlanOp jn{};                                               // the main stream joins the chain's end
      jn.kind = GH_PLAN_JOIN; jn.stream = GH_PLAN_MAIN;
      jn.r0 = jn.r1 = jn.c0 = jn.c1 = jn.k0 = jn.k1 = np;
      jn.wait0 = ev_panel; jn.wait1 = -1; jn.record = -1; jn.lower = 0;
      pl.ops.push_back(jn);
    }
  }
  pl.n_events = nev;
  return pl;
}
#endif  // GH_CHOL_PLAN_H_
