// gh_vecchia_impl.h -- what the Vecchia units share: the solver handle (gh_vecchia.hip) and the nearest-neighbour search on a
// cell grid (gh_vecchia_search.hip).  Private to the library.  predict through Q runs on the strip driver all solvers share
// (gh_predict.hip, declared in gh_common.h).
#pragma once
#include <vector>
#include "gh_common.h"

#define VM_MAX 64                       // lanes of a wavefront = the cap on m
#define VG_AXES 3                       // the grid covers the first min(ndim, 3) coordinates
#define VG_AXIS_CELLS (1 << 20)         // cells along one axis at most: keeps the rounding of a cell number under the bound's margin
#define VG_OCCUPANCY 16                 // points per cell aimed at when the caller passes 0 (profiles/vecchia/search_time.json)

// The grid of one data set: a uniform cell grid over the bounding box of the first g = min(ndim, 3) coordinates, the points
// sorted by cell.  Slot a of nc / lo / inv_h is grid axis a; the data's coordinate k sits in slot VG_AXES - g + k and the slots
// before it have one cell, so that the LAST slot runs fastest in the cell number and a run of cells along it is one contiguous
// run of sorted points.  An axis of zero (or not finite) extent has one cell.
struct GhVGridDev {
  const double* xs;                     // (n, nd) the coordinates in cell order
  const int* idx;                       // (n) the original index of a sorted point; ascending inside a cell
  const int* start;                     // (ncells + 1) the first sorted point of a cell
  long n;
  int nd, g;
  int nc[VG_AXES];
  double lo[VG_AXES], inv_h[VG_AXES];
  double h_min;                         // the smallest cell edge among the axes with more than one cell (0: one cell in all)
};
struct GhVGrid {
  GhPooledBuf xs, idx, start;
  GhVGridDev dev;
  bool valid = false;
  int occupancy = 0;                    // as requested (0: automatic)
  std::vector<double> x_seen;           // the host copy of the points the grid was built from
};
// Build the grid of the n points x (HOST memory, (n, nd) row-major) on the current device; the uploads are enqueued on st and the
// host arrays end with the call (it synchronises st).  occupancy: points per cell aimed at, 0 = VG_OCCUPANCY.
int gh_vgrid_build(GhVGrid& g, const double* x, int64_t n, int nd, int occupancy, hipStream_t st);
// table (nq, m) and cnt (nq), device memory: row c = the min(#eligible, m) points nearest to q[c] (device memory, (nq, nd)) by
// (squared distance, index), ascending by index, then -1; cnt[c] = how many.  Point j is eligible when j < limit[c]
// (device memory; nullptr: every point).  1 <= m <= VM_MAX.  Enqueued on st.
int gh_vgrid_query(const GhVGrid& g, const double* q, int64_t nq, const int64_t* limit, int m, int* table, int* cnt, hipStream_t st);

struct gh_vecchia {
  gh_vecchia_opts opts;
  hipStream_t st = nullptr;
  bool shared_stream = false;
  int64_t n = 0;
  int ndim = 0;
  bool computed = false;
  int64_t info = 0;
  double logdet = 0.0;
  // x, yerr, the compacted neighbour table (valid entries first) and its row counts, B (n, m), f, and the transposed index: the
  // entries (row, slot) of B in column j are tptr[j] .. tptr[j + 1], rows ascending.  One stream: st.
  GhPooledBuf x, yerr, nbr, cnt, B, f, tptr, trow, tslot, w1, scal;
  // the caller's table of the last compute(): the same table again (an optimiser moves the hyper-parameters, not the points) is
  // neither checked nor indexed nor uploaded a second time
  std::vector<int32_t> nbr_seen;
  // the search grid of x (gh_vecchia_predict_local_search): built at the first search after a compute() on other points
  GhVGrid grid;
};

struct VArgs {
  const double* x; const double* yerr; const int* nbr; const int* cnt;
  long n; int m, nd, n_nodes;
};
