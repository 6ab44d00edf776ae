// gh_fisher.hip -- the device pieces of gh_chol_fisher (gh_chol_solve.hip): F_ab = 1/2 tr(K^-1 D_a K^-1 D_b) in its symmetric form,
// W_a = L^-1 D_a L^-T (lower 128-tiles, by the GEMM family) and F_ab = sum_{i>j} W_a[i,j] W_b[i,j] + 1/2 sum_i W_a[i,i] W_b[i,i].
//   fisher_planes_kernel   D_a = dK/dtheta_a for the selected kernel parameters as dense np x np planes, plane-major
//   fisher_scale_kernel    L^-1 diag(d): what the first product of a DIAGONAL parameter would give, elementwise
//   fisher_pairs_kernel    up to 4 x 4 pairs of planes per launch: one 128 x 128 tile of every plane read once into registers,
//                          one partial row per workgroup; the fixed-order tree of gh_launch_kgrad_final follows
//   fisher_mirror_kernel   the pair sums into the (n_diag + size)^2 result, both halves from the same number
// No atomics anywhere: two calls give the same bits, and a pair's sum does not depend on which launch computed it (every
// accumulator sees the same elements in the same order whatever else the launch carries).  DESIGN.md section 4, "Information
// of the hyper-parameters".
#include "gh_common.h"
#include "gh_device_util.h"

namespace {
constexpr int FT = GH_TILE;                       // tile edge of the contraction = the tile of the GEMMs that wrote the planes

// One thread per element, consecutive lanes on consecutive columns: every plane is written in 512-byte runs per wavefront.
// The (n, n, P) interleaved layout of kgrad_kernel is what this avoids: a plane is a GEMM operand as it stands.
template <int PMAX>
__global__ __launch_bounds__(256) void fisher_planes_kernel(const GhNode* __restrict__ prog, int n_nodes, int nd, GhFisherSel sel,
                                                            const double* __restrict__ x, long n, long np, double* __restrict__ planes) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= np * np) return;
  const long i = idx / np, j = idx % np;
  const bool in = i < n && j < n;
  double g[PMAX];
  if (in) {
    // ordered arguments, as kgrad_kernel's symmetric form (kernel_interface.cpp:117-121)
    const double* p1 = x + i * nd;
    const double* p2 = x + j * nd;
    gh_eval_grad(prog, n_nodes, i > j ? p2 : p1, i > j ? p1 : p2, g);
  }
  for (int s = 0; s < sel.n; ++s) planes[(long)s * np * np + idx] = in ? g[sel.idx[s]] : 0.0;
}

// out[i][j] = linv[i][j] * d[j]   (d: np entries, zero from n on, so the padding columns come out zero)
__global__ __launch_bounds__(256) void fisher_scale_kernel(const double* __restrict__ linv, long np, const double* __restrict__ d,
                                                           double* __restrict__ out) {
  const long idx = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
  if (idx >= np * np) return;
  const long j = idx % np;                        // np is even: the pair never straddles a row
  const double2 v = *reinterpret_cast<const double2*>(linv + idx);
  const double2 w = *reinterpret_cast<const double2*>(d + j);
  *reinterpret_cast<double2*>(out + idx) = make_double2(v.x * w.x, v.y * w.y);
}

// One lower 128 x 128 tile (ti >= tj) per workgroup, 32 steps of 4 rows x 128 columns; a lane holds two adjacent columns
// (16-byte loads, a wavefront reads one whole 1 KiB tile row of a plane).  Per step a thread loads its two elements of each
// of the na + nb planes ONCE and feeds all na x nb accumulators from registers.  Weights: 1 below the diagonal, 1/2 on it, 0
// above (the diagonal tiles are full and only their lower half counts) -- powers of two, so scaling a factor is exact.
__global__ __launch_bounds__(256, 2) void fisher_pairs_kernel(GhFisherPairs q) {
  __shared__ double red[4][GH_FISHER_GROUP * GH_FISHER_GROUP];
  constexpr int G = GH_FISHER_GROUP;
  int ti, tj;
  tri_index(blockIdx.x, ti, tj);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long c = (long)tj * FT + lane * 2;
  const bool diag_tile = ti == tj;
  double acc[G][G];
#pragma unroll
  for (int a = 0; a < G; ++a)
#pragma unroll
    for (int b = 0; b < G; ++b) acc[a][b] = 0.0;
#pragma unroll 2
  for (int step = 0; step < FT / 4; ++step) {
    const long r = (long)ti * FT + step * 4 + wave;
    const long off = r * q.ld + c;
    double2 va[G], vb[G];
#pragma unroll
    for (int a = 0; a < G; ++a)
      va[a] = a < q.na ? *reinterpret_cast<const double2*>(q.a[a] + off) : make_double2(0.0, 0.0);
#pragma unroll
    for (int b = 0; b < G; ++b) {
      if (q.same) vb[b] = va[b];
      else vb[b] = b < q.nb ? *reinterpret_cast<const double2*>(q.b[b] + off) : make_double2(0.0, 0.0);
    }
    if (diag_tile) {
      const double w0 = c < r ? 1.0 : (c == r ? 0.5 : 0.0);
      const double w1 = c + 1 < r ? 1.0 : (c + 1 == r ? 0.5 : 0.0);
#pragma unroll
      for (int a = 0; a < G; ++a) { va[a].x *= w0; va[a].y *= w1; }      // (the a side only: vb was copied before)
    }
#pragma unroll
    for (int a = 0; a < G; ++a)
#pragma unroll
      for (int b = 0; b < G; ++b) {
        acc[a][b] = fma(va[a].x, vb[b].x, acc[a][b]);
        acc[a][b] = fma(va[a].y, vb[b].y, acc[a][b]);
      }
  }
#pragma unroll
  for (int a = 0; a < G; ++a)
#pragma unroll
    for (int b = 0; b < G; ++b) {
      const double v = wave_sum(acc[a][b]);
      if (lane == 0) red[wave][a * G + b] = v;
    }
  __syncthreads();
  if (threadIdx.x < G * G) {
    const int col = q.col[threadIdx.x];
    if (col >= 0) q.partial[(long)blockIdx.x * q.ncols + col] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// F[out[a]][out[b]] = F[out[b]][out[a]] = pairsum[pair(a, b)] for the Q active planes; everything else was zeroed before
__global__ void fisher_mirror_kernel(const double* __restrict__ pairsum, GhFisherMap m, double* __restrict__ F) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m.q * m.q) return;
  const int a = t / m.q, b = t % m.q;
  if (a > b) return;
  const double v = pairsum[gh_fisher_pair(a, b, m.q)];
  F[(long)m.out[a] * m.ptot + m.out[b]] = v;
  F[(long)m.out[b] * m.ptot + m.out[a]] = v;
}
}  // namespace

int gh_launch_fisher_planes(const gh_kernel* k, const GhFisherSel& sel, const double* x, int64_t n, int64_t np, double* planes,
                            hipStream_t st) {
  if (sel.n <= 0) return GH_OK;
  const long tot = (long)np * np;
  const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
  const int nn = (int)k->nodes.size();
  if (k->size <= 4)       hipLaunchKernelGGL(fisher_planes_kernel<4>, grid, block, 0, st, k->d_nodes, nn, k->ndim, sel, x, (long)n, (long)np, planes);
  else if (k->size <= 16) hipLaunchKernelGGL(fisher_planes_kernel<16>, grid, block, 0, st, k->d_nodes, nn, k->ndim, sel, x, (long)n, (long)np, planes);
  else                    hipLaunchKernelGGL(fisher_planes_kernel<GH_MAX_GRAD>, grid, block, 0, st, k->d_nodes, nn, k->ndim, sel, x, (long)n, (long)np, planes);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

int gh_launch_fisher_scale(const double* linv, int64_t np, const double* d, double* out, hipStream_t st) {
  const long half = (long)np * np / 2;
  hipLaunchKernelGGL(fisher_scale_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, st, linv, (long)np, d, out);
  GH_HIP(hipGetLastError());
  return GH_OK;
}

int gh_launch_fisher_pairs(const double* const* a, const int* a_idx, int na, const double* const* b, const int* b_idx, int nb,
                           int q_active, int64_t np, double* partial, hipStream_t st) {
  const bool same = b == nullptr;
  if (same) { b = a; b_idx = a_idx; nb = na; }
  const long tm = (long)(np / FT), nblk = tm * (tm + 1) / 2;
  constexpr int G = GH_FISHER_GROUP;
  for (int a0 = 0; a0 < na; a0 += G)
    for (int b0 = same ? a0 : 0; b0 < nb; b0 += G) {
      GhFisherPairs q{};
      q.na = std::min(G, na - a0); q.nb = std::min(G, nb - b0);
      q.same = same && a0 == b0;
      q.ld = (long)np; q.ncols = (long)q_active * (q_active + 1) / 2; q.partial = partial;
      for (int i = 0; i < G; ++i) {
        q.a[i] = i < q.na ? a[a0 + i] : nullptr;
        q.b[i] = i < q.nb ? b[b0 + i] : nullptr;
      }
      for (int i = 0; i < G; ++i)
        for (int j = 0; j < G; ++j) {
          int col = -1;
          if (i < q.na && j < q.nb && !(q.same && j < i)) {
            const int pa = a_idx[a0 + i], pb = b_idx[b0 + j];
            col = gh_fisher_pair(std::min(pa, pb), std::max(pa, pb), q_active);
          }
          q.col[i * G + j] = col;
        }
      hipLaunchKernelGGL(fisher_pairs_kernel, dim3((unsigned)nblk), dim3(256), 0, st, q);
      GH_HIP(hipGetLastError());
    }
  return GH_OK;
}

int gh_launch_fisher_mirror(const double* pairsum, const GhFisherMap& m, double* F, hipStream_t st) {
  if (m.q <= 0) return GH_OK;
  hipLaunchKernelGGL(fisher_mirror_kernel, dim3((unsigned)((m.q * m.q + 255) / 256)), dim3(256), 0, st, pairsum, m, F);
  GH_HIP(hipGetLastError());
  return GH_OK;
}
