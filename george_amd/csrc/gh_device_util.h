// gh_device_util.h -- small device helpers with ONE definition for the one-problem kernels (gh_kmat.hip, gh_chol_solve.hip) and
// their batched forms (gh_batch.hip), which claim the same bits; and (hw_*) for the HODLR units whose kernels reduce over a
// workgroup of any size: gh_hodlr.hip, gh_hodlr_aca.hip, gh_hodlr_apply.hip.  (The column reduction of predict needs none of
// them -- a thread per column -- and has its one definition in gh_predict.hip.)
#pragma once
#include <hip/hip_runtime.h>

// lower-triangular tile enumeration: b -> (ti, tj), tj <= ti
__device__ __forceinline__ void tri_index(long b, int& ti, int& tj) {
  long t = (long)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while (t * (t + 1) / 2 > b) --t;
  while ((t + 1) * (t + 2) / 2 <= b) ++t;
  ti = (int)t;
  tj = (int)(b - t * (t + 1) / 2);
}
// fixed-order sums over a wavefront (lane 0 has it) and over a 256-thread workgroup (every thread has it)
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double block_sum_256(double v, double* sh /* >= 4 */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- HODLR: the sum over a wavefront (lane 0 has it) and block-wide reductions for any workgroup size
__device__ __forceinline__ double hw_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// block-wide sum broadcast to all threads; `sh` needs blockDim/64 doubles
__device__ __forceinline__ double hw_block_sum(double v, double* sh) {
  v = hw_wave_sum(v);
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t += sh[w];
  return t;
}
// block-wide argmax of (val, idx): largest val, smallest idx on ties (Eigen maxCoeff order)
__device__ __forceinline__ void hw_block_argmax(double& val, int& idx, double* shv, int* shi) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(val, off, 64);
    const int oi = __shfl_down(idx, off, 64);
    if (ov > val || (ov == val && oi >= 0 && (idx < 0 || oi < idx))) { val = ov; idx = oi; }
  }
  const int nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = val; shi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  double bv = shv[0];
  int bi = shi[0];
  for (int w = 1; w < nw; ++w)
    if (shv[w] > bv || (shv[w] == bv && shi[w] >= 0 && (bi < 0 || shi[w] < bi))) { bv = shv[w]; bi = shi[w]; }
  val = bv; idx = bi;
}
