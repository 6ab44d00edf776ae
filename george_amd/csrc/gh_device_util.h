// gh_device_util.h -- small device helpers with ONE definition for the one-problem kernels (gh_kmat.hip, gh_chol_solve.hip) and
// their batched forms (gh_batch.hip), which claim the same bits
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
