// gh_kgrad_body.h -- the body of the fused gradient reduction (gh_kmat.hip), included once per kernel with GH_KGRAD_LOO set:
//   0: A_ij = alpha_i alpha_j - Kinv_ij, weights 1/2 on the diagonal and 1 below (1/2 sum_ij A_ij dK_ij: the likelihood gradient);
//   1: B_ij = 1/2 (alpha_i beta_j + beta_i alpha_j) - M_ij, weights 1 on the diagonal and 2 below (sum_ij B_ij dK_ij: the
//      leave-one-out gradient, gh_chol_loo); `kinv` holds M, `alpha` is TWO vectors `ld` apart -- alpha, then beta -- and diagA
//      receives diag(B).
// Text, not a function and not a template flag: the likelihood kernel stays token for token the kernel it was before there
// were two.  Both alternatives were built and compared in the device assembly: through a shared __forceinline__ function the
// likelihood instances came out with another register allocation and schedule (existing GPU tests pin their results, and the
// benchmark their time); a `bool LOO` template parameter kept the instructions but changed the mangled name that
// tests/test_hodlr_predict_grad_host.py looks the kernel's scratch size up by.
// The caller of the leave-one-out form (gh_chol_solve.hip, cv_contract) asserts that its two vectors are adjacent, ld = Np apart.
  __shared__ double xr[KT * GH_MAX_NDIM];
  __shared__ double xc[KT * GH_MAX_NDIM];
  __shared__ double red[4][PMAX];
  int ti, tj;
  tri_index(blockIdx.x, ti, tj);
  const long r0 = (long)ti * KT, c0 = (long)tj * KT;
  for (int t = threadIdx.x; t < KT * nd; t += 256) {
    const long r = r0 + t / nd;
    xr[t] = (r < n) ? x[r * nd + (t % nd)] : 0.0;
    const long c = c0 + t / nd;
    xc[t] = (c < n) ? x[c * nd + (t % nd)] : 0.0;
  }
  __syncthreads();
  double acc[PMAX];
#pragma unroll
  for (int p = 0; p < PMAX; ++p) acc[p] = 0.0;
  const int lc = threadIdx.x & 63;
  const int lr = threadIdx.x >> 6;
#pragma unroll 1
  for (int pass = 0; pass < KT / 4; ++pass) {
    const int rr = lr + pass * 4;
    const long r = r0 + rr, c = c0 + lc;
    if (r < n && c <= r) {
      double g[PMAX];
      // ordered arguments (x_min, x_max) = (x_c, x_r) since c <= r  (kernel_interface.cpp:117-121)
      gh_eval_grad(prog, n_nodes, &xc[lc * nd], &xr[rr * nd], g);
      const double kin = kinv[r * ld + c];
#if GH_KGRAD_LOO
      const double* beta = alpha + ld;
      const double aij = 0.5 * (alpha[r] * beta[c] + beta[r] * alpha[c]) - kin;
      const double w = (r == c) ? aij : 2.0 * aij;
#else
      const double aij = alpha[r] * alpha[c] - kin;
      const double w = (r == c) ? 0.5 * aij : aij;
#endif
      if (r == c && diagA) diagA[r] = aij;
#pragma unroll
      for (int p = 0; p < PMAX; ++p) if (p < P) acc[p] += w * g[p];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int p = 0; p < PMAX; ++p) {
    double v = acc[p];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][p] = v;
  }
  __syncthreads();
  if (threadIdx.x < PMAX && threadIdx.x < P) {
    const int p = threadIdx.x;
    partial[(long)blockIdx.x * P + p] = which[p] ? (red[0][p] + red[1][p]) + (red[2][p] + red[3][p]) : 0.0;
  }
