/*
 * george_amd.h -- C ABI of the MI355X-native GP solver backend for dfm/george.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point cites the reference interface it replaces (paths relative
 * to the dfm/george source tree).  The Python host layer (george_amd/ *.py)
 * binds these with ctypes; INTEGRATION.md shows the stub a george maintainer
 * would add.
 *
 * Conventions
 *   - all matrices are C-contiguous (row-major) fp64, exactly as the reference
 *     passes them through pybind11 / NumPy;
 *   - every function returns a status code (GH_OK == 0); gh_last_error() gives
 *     a thread-local message.  No exception crosses the boundary;
 *   - handles are opaque, owned by the library, freed by *_destroy, and not
 *     re-entrant (one call at a time per handle);
 *   - calls are synchronous: on return the result is complete.
 *
 * Pointer kinds (what tests/test_gpu_device_pointers.py passes, entry by entry)
 *   - DATA ARRAYS may be host memory or device (HBM) memory, each on its own: the
 *     points (x, x1, x2, xs, t, q, x_new), error bars and right-hand sides (yerr,
 *     yerr_new, y, r, b, z, diag_rows, params), packed factors, `limit` of the
 *     search, and every array result (out, mu, var, cov, dmu, dvar, grad, alpha,
 *     diagA, resid, lpd, v, diagB, fisher, draws, fac, logdet / quad / info of the
 *     batch calls).  `rank` of the sample calls too.  The library detects which
 *     (hipPointerGetAttributes), stages host arrays itself, reads device inputs
 *     where they lie or copies them, and writes a result into the memory space
 *     of its pointer;
 *   - these are always HOST memory, because the library reads or writes them on
 *     the host: the scalar results logdet_out, `out` of the *_dot_solve entries,
 *     logdet / quad of gh_chol_objective, logdet / lpd_sum of the cross-validation
 *     entries; the masks `which` (gh_chol_objective_grad_batch alone takes
 *     either); the index tables order, start, idx, nbr, qnbr;
 *     table_out of the two search entries; ranks_out and the like.  So is every
 *     pointer of the multi-device entries (gh_mgpu_*, gh_hodlr_mgpu_*), and
 *     every pointer of gh_dev_* is DEVICE memory, as said there;
 *   - a device array needs the alignment of its element type (8 bytes for
 *     doubles) and no more: no kernel reads or writes a caller's array with a
 *     wider access unless it has checked the address;
 *   - the caller guarantees that device inputs are complete when the call is
 *     made (the calls run on the library's own streams).  Inputs are never
 *     modified -- not even transiently -- unless the entry says that two
 *     arguments may alias;
 *   - every result, on the host or on the device, is complete when the call
 *     returns; two calls with the same arguments give the same bits whatever the
 *     memory spaces of the arguments.
 */
#ifndef GEORGE_AMD_H_
#define GEORGE_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GH_MAX_AXES    8           /* max active axes of one leaf kernel */
#define GH_MAX_NDIM    16          /* max input dimension */
#define GH_MAX_PARAMS  4
#define GH_MAX_METRIC  36          /* GH_MAX_AXES*(GH_MAX_AXES+1)/2 */
#define GH_MAX_NODES   64
#define GH_MAX_GRAD    64          /* max full_size of a kernel expression */
#define GH_MAX_STACK   8           /* max postfix evaluation depth */

/* status codes.  The Python layer maps NOT_PD -> numpy.linalg.LinAlgError,
 * BAD_ARG -> ValueError, DIM -> RuntimeError("dimension mismatch")
 * (reference include/george/exceptions.h:8-12), NOT_COMPUTED ->
 * RuntimeError("you must call 'compute' first") (exceptions.h:14-18). */
enum {
  GH_OK = 0,
  GH_ERR_NOT_PD = 1,
  GH_ERR_BAD_ARG = 2,
  GH_ERR_HIP = 3,
  GH_ERR_NOT_COMPUTED = 4,
  GH_ERR_DIM = 5,
  GH_ERR_NOMEM = 6,
  GH_ERR_RANK = 7,       /* HODLR: a block needs a rank above the solver's ceiling (1024) for the requested tol */
  GH_REFACTORIZE = 8     /* gh_chol_remove: nothing was done; the caller computes afresh on the kept points (not an error) */
};

/* node operators */
enum { GH_OP_LEAF = 0, GH_OP_SUM = 1, GH_OP_PRODUCT = 2 };

/* leaf kernel ids == the reference's `kernel_type` class attributes
 * (src/george/kernels.py:273,322,391,464,500,546,588,666,712,753,822,897,944) */
enum {
  GH_K_LINEAR = 0, GH_K_RATQUAD = 1, GH_K_EXP = 2, GH_K_LOCALGAUSS = 3,
  GH_K_EMPTY = 4, GH_K_COSINE = 5, GH_K_MATERN52 = 6, GH_K_EXPSINE2 = 7,
  GH_K_CONSTANT = 8, GH_K_EXPSQUARED = 9, GH_K_MATERN32 = 10,
  GH_K_POLYNOMIAL = 11, GH_K_DOTPRODUCT = 12
};

/*
 * One node of a kernel expression, flattened in POSTFIX order (children
 * before their operator).  This POD replaces the heap-allocated C++ object
 * tree that `george::parse_kernel_spec` builds from the Python spec
 * (include/george/parser.h:14-35 operators, :344-403 stationary leaves);
 * the fields are exactly the attributes that parser reads.
 */
typedef struct gh_knode {
  int32_t op;                       /* GH_OP_*                                        */
  int32_t kernel_type;              /* GH_K_* (leaf only)                              */
  int32_t metric_type;              /* 0 isotropic, 1 axis-aligned, 2 general; -1 = non-stationary leaf */
  int32_t ndim;                     /* input dimension                                 */
  int32_t naxes;                    /* number of active axes                           */
  int32_t blocked;                  /* stationary leaves: `blocked` flag               */
  int32_t n_params;                 /* own parameters (e.g. log_alpha)                 */
  int32_t n_metric;                 /* metric parameters                               */
  int32_t axes[GH_MAX_AXES];
  double  params[GH_MAX_PARAMS];    /* own parameters, in parameter_names order        */
  double  constant;                 /* `order` for Linear/Polynomial                   */
  double  metric[GH_MAX_METRIC];    /* metric.get_parameter_vector(include_frozen=True) */
  double  min_block[GH_MAX_AXES];
  double  max_block[GH_MAX_AXES];
} gh_knode;

typedef struct gh_kernel gh_kernel;
typedef struct gh_chol   gh_chol;
typedef struct gh_hodlr  gh_hodlr;

/* ------------------------------------------------------------------ misc */
int         gh_device_count(void);
const char* gh_last_error(void);
const char* gh_version(void);
/* Device memory the library keeps for re-use -- released transient blocks (up to 128 GB per device, gh_set_cache_limit) -- is really freed.  The
 * library does this itself before it reports GH_ERR_NOMEM; an application that needs the memory for its own allocations
 * calls it directly (solver handles keep what they hold: gh_chol_trim / gh_chol_release_buffers / *_destroy). */
void gh_release_caches(int32_t device);
/* upper bound, per device, on the released device blocks the library keeps parked for its next allocation (default 128 GB of
 * the 288; they are otherwise returned to the driver only when one of the library's OWN allocations fails).  A process that
 * shares a GPU with another allocator (torch, RCCL buffers) lowers it; 0 = park nothing.  Blocks above the new bound are
 * freed at once.  (No reference counterpart: NumPy's allocator, basic.py:58.) */
void gh_set_cache_limit(int64_t bytes);
/* ---------------------------------------------- kernel-function evaluator
 * Replaces the pybind11 class KernelInterface, src/george/kernel_interface.cpp:
 *   ctor + parse_kernel_spec  :12-14   -> gh_kernel_create
 *   value_general             :47-60   -> gh_kernel_value_general
 *   value_symmetric           :62-77   -> gh_kernel_value_symmetric
 *   value_diagonal            :79-90   -> gh_kernel_value_diagonal
 *   gradient_general          :92-107  -> gh_kernel_gradient_general
 *   gradient_symmetric        :109-125 -> gh_kernel_gradient_symmetric
 *   x1_gradient_general       :127-141 -> gh_kernel_x1_gradient_general
 *   x2_gradient_general       :143-157 -> gh_kernel_x2_gradient_general
 * `which` is the uint32 mask of kernels.py:120; masked-out slots (left
 * uninitialised by the reference, kernels.h:85-91) are written as 0. */
int  gh_kernel_create(const gh_knode* nodes, int n_nodes, gh_kernel** out);
void gh_kernel_destroy(gh_kernel* k);
int  gh_kernel_ndim(const gh_kernel* k);
int  gh_kernel_size(const gh_kernel* k);          /* full_size */
int  gh_kernel_value_general(gh_kernel* k, const double* x1, int64_t n1,
                             const double* x2, int64_t n2, double* out /* n1*n2 */);
int  gh_kernel_value_symmetric(gh_kernel* k, const double* x, int64_t n, double* out /* n*n */);
int  gh_kernel_value_diagonal(gh_kernel* k, const double* x1, const double* x2,
                              int64_t n, double* out /* n */);
int  gh_kernel_gradient_general(gh_kernel* k, const uint32_t* which,
                                const double* x1, int64_t n1, const double* x2, int64_t n2,
                                double* out /* n1*n2*size */);
int  gh_kernel_gradient_symmetric(gh_kernel* k, const uint32_t* which,
                                  const double* x, int64_t n, double* out /* n*n*size */);
int  gh_kernel_x1_gradient_general(gh_kernel* k, const double* x1, int64_t n1,
                                   const double* x2, int64_t n2, double* out /* n1*n2*ndim */);
int  gh_kernel_x2_gradient_general(gh_kernel* k, const double* x1, int64_t n1,
                                   const double* x2, int64_t n2, double* out /* n1*n2*ndim */);
/* Prior draws at t (m, ndim) (replaces GP.sample(t), src/george/gp.py -- get_matrix + TINY on the diagonal -- and utils.py:11-33):
 * K(t, t) + jitter * I is built and factored on the device (gh_dev_pstrf), draws (nz, m) = z[:, :rank] L[:, :rank]^T for the caller's
 * standard normals z (nz, m).  tol < 0: m * eps * max diag (K(t, t) + jitter I).  fac (m, m) or NULL; *rank int64 (host or device
 * memory).  The current device and its null stream, as gh_kernel_value_symmetric. */
int  gh_kernel_sample(gh_kernel* k, const double* t, int64_t m, double jitter, const double* z, int64_t nz, double tol,
                      double* draws /* nz*m */, double* fac /* m*m or NULL */, int64_t* rank);

/* ------------------------------------------------------- dense Cholesky solver
 * Replaces BasicSolver (src/george/solvers/basic.py) and the SciPy/LAPACK
 * dpotrf/dpotrs it calls:
 *   compute        :51-70   (K = kernel(x); K_ii += yerr_i^2; cholesky; log_det)
 *   apply_inverse  :72-87   (cho_solve)            -> gh_chol_solve
 *   dot_solve      :89-102  (y . cho_solve(y))     -> gh_chol_dot_solve
 *   apply_sqrt     :104-114 (r @ U)                -> gh_chol_apply_sqrt
 *   get_inverse    :116-121                        -> gh_chol_get_inverse
 * plus fused device-resident forms of the GP glue around it
 *   GP.predict            src/george/gp.py:482-545 -> gh_chol_predict
 *   GP.grad_log_likelihood (kernel part) gp.py:429-466 -> gh_chol_grad
 * K is built on the device from (kernel, x) and never visits the host.
 * Pointer kinds: "Pointer kinds" at the top of this file holds for every entry below; an entry repeats only which of its
 * pointers are host memory. */
typedef struct gh_chol_opts {
  int32_t device;        /* HIP device ordinal                                   */
  int32_t nb;            /* outer panel width (multiple of 128); 0 = default      */
  int32_t profile;       /* 1: record per-kernel-class hipEvent timings           */
  int32_t lookahead;     /* 1: overlap panel factorisation with trailing update   */
  int32_t reserved[4];
} gh_chol_opts;

int  gh_chol_create(const gh_chol_opts* opts, gh_chol** out);
void gh_chol_destroy(gh_chol* s);
/* yerr: (n,) standard deviations ALREADY including white noise (gp.py:330).  x and yerr: host or device memory, each on its own
 * (both on the device: one launch brings them in, no copy is enqueued); *logdet_out: host. */
int  gh_chol_compute(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                     const double* yerr, double* logdet_out);
/* Sequential use (no reference counterpart: gp.py:303-337 always rebuilds).
 * K' = [[K, k(x, xn)], [k(xn, x), k(xn, xn) + diag(yerr_new^2)]]: extend the computed factor by m rows.  The rows of the
 * full 128-row tiles of the factor and their diagonal-block inverses are not touched (bit for bit); the rows of the last,
 * partial tile are formed again.  The kernel must be the one (same parameters) the handle was computed with; that is the
 * caller's contract.  x_new (m, ndim), yerr_new (m).  On GH_OK the handle is computed at n + m and
 * *logdet_out = log|K'|.  On GH_ERR_NOT_PD, gh_chol_info() is the 1-based index in the extended matrix, and the handle is
 * left computed at the OLD n with the old factor bits; so it is after GH_ERR_NOMEM.  Any other error (a failed HIP call) while
 * the last tile is being rewritten in place leaves the handle NOT computed.  A handle rebuilt by gh_chol_import_factor needs
 * gh_chol_set_yerr first (GH_ERR_BAD_ARG otherwise): the old rows of the last, partial tile are formed again from the kernel
 * and the error bars.  When the tile count grows the factor moves into another buffer; the handle keeps the one it left as a
 * spare for the next move (counted by gh_chol_device_bytes, freed by gh_chol_trim). */
int  gh_chol_append(gh_chol* s, gh_kernel* k, const double* x_new, int64_t m, const double* yerr_new, double* logdet_out);
/* keep the first n_keep points (0 < n_keep <= n); *logdet_out = log|K[:n_keep, :n_keep]|.  Data movement and one reduction. */
int  gh_chol_truncate(gh_chol* s, int64_t n_keep, double* logdet_out);
/* Take the m points idx[0] < idx[1] < ... (host array, 0 <= idx[i] < n, 0 < m < n) out of the computed factor, anywhere in the data
 * set (no reference lines correspond: basic.py:51-70 always refactorises).  With keep / rem the kept / removed indices,
 * K[keep, keep] = L[keep, keep] L[keep, keep]^T + W W^T, W = L[keep, rem]: a rank-m Cholesky UPDATE of the gathered factor, in
 * passes of at most 128 columns of W -- no kernel evaluations and no error bars, so it works on an imported factor too.  Rows of
 * the 128-row tiles in front of the first removed index, and their diagonal-block inverses, keep their bits.  On GH_OK the handle
 * is computed at n - m and *logdet_out = log|K[keep, keep]|.  idx == n-m .. n-1 is gh_chol_truncate(n - m), bit for bit.  The new
 * factor is built in other buffers (the factor's spare, as append) and swapped in after one final synchronisation: on ANY failure
 * -- GH_ERR_BAD_ARG for a bad idx, GH_ERR_NOMEM, a failed HIP call, GH_ERR_NOT_PD for a pivot that is not finite and positive --
 * the handle keeps its factor, size, info and log-determinant bit for bit.  GH_REFACTORIZE: see gh_debug_set_remove_path. */
int  gh_chol_remove(gh_chol* s, const int64_t* idx, int64_t m, double* logdet_out);
/* the error bars (n, as given to compute / append; host or device memory) of a computed handle: what gh_chol_import_factor does
 * not bring */
int  gh_chol_set_yerr(gh_chol* s, const double* yerr);
int64_t gh_chol_info(const gh_chol* s);     /* 1-based index of the failing pivot after GH_ERR_NOT_PD, else 0 */
int64_t gh_chol_size(const gh_chol* s);
int64_t gh_chol_device_bytes(const gh_chol* s);  /* HBM bytes the handle holds right now (factor + work arrays) */
/* the protocol's four: b, y, r and the array results are host or device memory; *out of gh_chol_dot_solve is a host double.  A
 * device y is read where it lies when n is a multiple of 128, and is not modified. */
int  gh_chol_solve(gh_chol* s, const double* b, int64_t nrhs, double* out);   /* b, out: (n, nrhs) row-major; may alias */
int  gh_chol_dot_solve(gh_chol* s, const double* y, double* out);
int  gh_chol_apply_sqrt(gh_chol* s, const double* r, int64_t nrows, double* out); /* r, out: (nrows, n) */
int  gh_chol_get_inverse(gh_chol* s, double* out /* n*n */);
/* mu = K(xs,x) K^-1 r ; var = diag(K(xs,xs)) - diag(K(xs,x) K^-1 K(x,xs)) ;
 * cov = K(xs,xs) - K(xs,x) K^-1 K(x,xs).   var / cov may be NULL.  r, xs, mu, var, cov: host or device memory (device xs are
 * read where they lie). */
int  gh_chol_predict(gh_chol* s, gh_kernel* k, const double* r /* n: y - mean */,
                     const double* xs, int64_t m, double* mu /* m */,
                     double* var /* m or NULL */, double* cov /* m*m or NULL */);
/* Posterior draws on a computed handle, on the device (replaces GP.sample_conditional, src/george/gp.py, and the SVD of
 * utils.py:11-33 behind it).  mu and cov are formed exactly as gh_chol_predict forms them; cov stays on the device and is factored
 * there by the diagonally pivoted Cholesky with rank truncation of gh_dev_pstrf (a predictive covariance is numerically
 * semidefinite: a plain Cholesky fails on it); then, as one GEMM,
 *   draws (nz, m) = mu + z[:, :rank] L[:, :rank]^T        z (nz, m): standard normals supplied by the caller.
 * tol: the factor's absolute stop threshold; tol < 0 means the default m * eps * max diag K(xs, xs) -- the PRIOR's scale, because
 * the rounding error of cov scales with the prior, not with the possibly tiny posterior variances.  mu (m) or NULL (no mean model:
 * the caller adds it); fac (m, m) or NULL receives L (columns >= rank exactly zero; L L^T approximates cov within tol entrywise);
 * *rank (int64, host or device memory): the number of pivots taken.  The covariance never reaches the host; the
 * work buffers are counted by gh_chol_device_bytes and freed by gh_chol_trim. */
int  gh_chol_sample_conditional(gh_chol* s, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t m,
                                const double* z /* nz*m */, int64_t nz, double tol, double* mu /* m or NULL */,
                                double* draws /* nz*m */, double* fac /* m*m or NULL */, int64_t* rank);
/* Derivatives of the prediction with respect to the test points, on a computed handle (no lines of the reference correspond:
 * src/george/gp.py stops at predict; the two formulas below are the definition).  With alpha = K^-1 r, k_c = K(x, xs_c),
 * w_c = K^-1 k_c, G_cid = d k(xs_c, x_i) / d xs_cd (the evaluator's x1-gradient) and D_cd = [x1-gradient + x2-gradient]_d of k
 * at (xs_c, xs_c) -- zero for stationary kernels, taken from the evaluator for every kernel:
 *   dmu[c][d]  = sum_i G_cid alpha_i                      (no mean model: the caller adds its derivative)
 *   dvar[c][d] = D_cd - 2 sum_i G_cid w_ic
 * mu and var are gh_chol_predict's, bit for bit (the same launches).  G is evaluated and reduced in one kernel and never stored;
 * the sums run in a fixed order (no atomics: two calls give the same bits).  mu, var and dvar may be NULL, each on its own (dvar
 * without var is allowed); dmu may not.  The results leave in one batch of copies
 * followed by one synchronisation, after the one of predict's forward sweep.  With dmu alone (mu, var and dvar all NULL) neither
 * K(x, xs) nor a substitution with m right-hand sides is formed: two sweeps for alpha, the kernel, one synchronisation; dmu has
 * the same bits either way.  Memory is that of gh_chol_predict with var (W = K^-1 K(x, xs) overwrites V = L^-1 K(x, xs) in
 * place), counted by gh_chol_device_bytes and freed by gh_chol_trim. */
int  gh_chol_predict_grad(gh_chol* s, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t m,
                          double* mu /* m or NULL */, double* var /* m or NULL */,
                          double* dmu /* m*ndim */, double* dvar /* m*ndim or NULL */);
/* alpha = K^-1 r; A = alpha alpha^T - K^-1; grad[p] = 1/2 sum_ij A_ij dK_ij/dtheta_p
 * for the parameters selected by `which` (others 0); diagA (n) = diag(A).  which: host; r, grad, alpha, diagA: host or device. */
int  gh_chol_grad(gh_chol* s, gh_kernel* k, const uint32_t* which, const double* r,
                  double* grad /* size */, double* alpha /* n or NULL */, double* diagA /* n or NULL */);
/* Fused hyper-parameter objective: GP.nll + GP.grad_nll (src/george/gp.py:470-480, i.e. compute
 * gp.py:303-337 + log_likelihood :369-397 + the kernel part of grad_log_likelihood :429-466) as ONE
 * device-resident call with one synchronisation: build K, factor, *logdet = log|K|,
 * *quad = r^T K^-1 r, and -- when grad != NULL -- alpha = K^-1 r (from the same forward solve),
 * K^-1 and grad[p] = 1/2 sum_ij A_ij dK_ij/dtheta_p for the parameters selected by `which`.
 * grad / alpha / diagA may be NULL; the handle is left computed (solve / predict may follow).  *logdet, *quad and which: host;
 * x, yerr, r, grad, alpha, diagA: host or device memory. */
int  gh_chol_objective(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                       const double* yerr, const double* r /* n: y - mean */, const uint32_t* which,
                       double* logdet, double* quad, double* grad /* size or NULL */,
                       double* alpha /* n or NULL */, double* diagA /* n or NULL */);
/* Leave-one-out cross-validation on a computed handle (no reference counterpart: src/george/gp.py has none; GPML section 5.4.2).
 * With alpha = K^-1 r and c_i = (K^-1)_ii:
 *   resid[i] = alpha_i / c_i = y_i - mu_i   (mu_i: the prediction of y_i from all other points)
 *   var[i]   = 1 / c_i
 *   lpd[i]   = 1/2 log c_i - 1/2 alpha_i^2 / c_i - 1/2 log 2 pi;      *lpd_sum = sum_i lpd[i]   (GPML eq. 5.11)
 * and, with u = resid, w_i = 1/2 (1 + alpha_i^2 / c_i) / c_i, v = K^-1 u, B = 1/2 (v alpha^T + alpha v^T) - K^-1 diag(w) K^-1:
 *   grad[p]  = sum_ij B_ij dK_ij/dtheta_p  for the parameters selected by `which` (others exactly 0)
 *   v (n)    : d lpd_sum / d mean_i;      diagB (n) = diag(B): d lpd_sum / d K_ii.
 * grad, v and diagB all NULL: K^-1 is not formed (c from L^-1; one N x N work buffer); otherwise two, as gh_chol_grad.
 * which == NULL: no gradient (grad must be NULL too).  *lpd_sum and which are host memory.  Two calls give the same bits. */
int  gh_chol_loo(gh_chol* s, gh_kernel* k, const uint32_t* which /* NULL: no gradient */, const double* r,
                 double* lpd_sum, double* resid /* n: alpha_i / c_i = y_i - mu_i */, double* var /* n */,
                 double* lpd /* n or NULL */, double* grad /* size, or NULL */, double* v /* n or NULL */,
                 double* diagB /* n or NULL */);
/* Fused leave-one-out objective: gh_chol_compute + gh_chol_loo as ONE device-resident call with one synchronisation (what
 * gh_chol_objective is to compute + dot_solve + grad), bit for bit the results of the two calls; *logdet = log|K|.  The handle
 * is left computed; on GH_ERR_NOT_PD gh_chol_info() is set and it is not.  *logdet, *lpd_sum and which: host. */
int  gh_chol_loo_objective(gh_chol* s, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                           const double* r, const uint32_t* which, double* logdet, double* lpd_sum,
                           double* resid, double* var, double* grad, double* v, double* diagB);
/* Leave-group-out cross-validation on a computed handle (no reference lines correspond: src/george/gp.py has no cross-validation).
 * The groups I_1 .. I_G partition the points: order (n) lists the point indices sorted by group, start (ngroups + 1) the groups'
 * offsets into it; both are HOST arrays.  With C = K^-1, alpha = C r and C_gg the block of C on group g (m_g points):
 *   resid_g = C_gg^-1 alpha_g = y_g - mu_g   (mu_g: the joint prediction of the group from all other points)
 *   cov_g   = C_gg^-1,  var = its diagonal
 *   lpd[g]  = 1/2 log|C_gg| - 1/2 alpha_g^T C_gg^-1 alpha_g - m_g/2 log 2 pi;      *lpd_sum = sum_g lpd[g]
 * and, with u = resid, v = C u, W = blockdiag_g 1/2 (C_gg^-1 + u_g u_g^T), B = 1/2 (v alpha^T + alpha v^T) - C W C:
 *   grad[p]  = sum_ij B_ij dK_ij/dtheta_p  for the parameters selected by `which` (others exactly 0)
 *   v (n)    : d lpd_sum / d mean_i;      diagB (n) = diag(B): d lpd_sum / d K_ii.
 * Groups of one point each give gh_chol_loo.  resid, var, v, diagB are in the caller's point order; cov holds the G blocks one after
 * the other, each m_g x m_g row-major with its rows in the order of `order`.  A group has at most 128 points.  GH_ERR_BAD_ARG, before
 * any device work, when order is not a permutation of 0 .. n-1, start does not rise from 0 to n, a group is empty or has more than
 * 128 points, or grad is given without which.  grad, v and diagB all NULL: K^-1 is not formed (one N x N work buffer); otherwise two,
 * as gh_chol_grad.  The slot buffers are counted by gh_chol_device_bytes and freed by gh_chol_trim.  *lpd_sum and which are host
 * memory, like order and start.  Two calls give the same bits. */
int  gh_chol_lgo(gh_chol* s, gh_kernel* k, const uint32_t* which /* NULL: no gradient */, const double* r,
                 const int64_t* order /* n, host */, const int64_t* start /* ngroups+1, host */, int64_t ngroups,
                 double* lpd_sum, double* resid /* n, caller's point order */, double* var /* n */,
                 double* lpd /* ngroups or NULL */, double* cov /* sum m_g^2, group-major, row-major blocks, or NULL */,
                 double* grad /* size or NULL */, double* v /* n or NULL */, double* diagB /* n or NULL */);
/* Expected (Fisher) information of the hyper-parameters on a computed handle (no reference lines correspond: src/george/gp.py
 * stops at the gradient; GPML eq. 5.9 differentiated once more and averaged over y ~ N(0, K)):
 *   fisher[a][b] = 1/2 tr(K^-1 D_a K^-1 D_b),    (n_diag + size)^2 doubles, row-major, symmetric bit for bit.
 * The "parameters" are, in this order, the n_diag DIAGONAL derivative matrices D_p = diag(diag_rows[p]) -- how a white-noise
 * model enters: dK/dtheta_p = diag(exp(wn(x)) dwn_p(x)) -- and the kernel's `size` parameters, D = dK/dtheta from the evaluator;
 * those masked out by `which` have rows and columns of exactly 0.  It does not depend on y.  n_diag <= 64.
 * Formed as W_a = L^-1 D_a L^-T (two triangular GEMMs per kernel parameter, one per diagonal one; K^-1 is not formed) and
 * fisher[a][b] = 1/2 sum_ij W_a[i][j] W_b[i][j] over dense planes of 8 Np^2 bytes (Np = n rounded up to 128), contracted in
 * fixed-order sums (no atomics: two calls give the same bits).
 * Memory: L^-1, one intermediate and the planes.  max_bytes > 0 bounds these (2 + planes) * 8 Np^2 bytes; <= 0: no limit of
 * its own.  When every active plane fits (the budget, and what the device can allocate) they are resident at once; otherwise
 * the call works in blocks -- (planes that fit) - 1 resident, every later plane formed again into the remaining one for every
 * block -- and the result has the same bits for every max_bytes the call accepts.  When not even two planes fit: GH_ERR_NOMEM.
 * The factor is not modified and on any failure the handle keeps its factor, size, info and log-determinant.  which is host
 * memory.  Everything runs on the handle's main stream with one synchronisation at the end; the buffers are
 * counted by gh_chol_device_bytes and freed by gh_chol_trim.  For a general (full-matrix) metric the evaluator's
 * parameter-gradient entries are the reference's, and the information inherits them. */
int  gh_chol_fisher(gh_chol* s, gh_kernel* k, const uint32_t* which /* size */,
                    const double* diag_rows /* (n_diag, n) or NULL */, int32_t n_diag,
                    int64_t max_bytes /* <= 0: no limit of its own */,
                    double* fisher /* (n_diag + size)^2, row-major */);
/* B independent problems that share the points x (n, ndim) and the kernel's STRUCTURE, each with its own parameters, error bars
 * and residual (B rounds of compute gp.py:303-337 + log_likelihood :369-397, one device call):
 *   K_b = k(params_b)(x, x) + diag(yerr_b^2);  logdet[b] = log|K_b|;  quad[b] = r_b^T K_b^-1 r_b;
 *   info[b] = 0, or the 1-based index of the failing pivot of K_b (the gh_chol_info of the one-problem call).
 * params: (B, gh_kernel_size(k)) row-major, each row a FULL parameter vector of k (frozen entries included, k's order);
 * k supplies the structure only.  yerr, r: (B, n) row-major.  A member that is not positive definite does not fail the call:
 * GH_OK is returned whenever every member was evaluated, and failures are reported in info (logdet / quad of such a member
 * are NaN).  Any pointer may be host or device memory.  The handle is left NOT computed. */
int  gh_chol_objective_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                             const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                             double* logdet, double* quad, int64_t* info);
/* B posterior predictions of one kernel STRUCTURE at B parameter vectors (B rounds of compute gp.py:303-337 + predict
 * :482-545, one device call).  params, x, yerr, r, info: as gh_chol_objective_batch.  xs: (m, ndim).
 *   mu[b]  (m)    = K_b(xs, x) K_b^-1 r_b                          (no mean model: the caller adds it, as for gh_chol_predict)
 *   var[b] (m)    = diag K_b(xs, xs) - diag K_b(xs, x) K_b^-1 K_b(x, xs)     or NULL
 *   cov[b] (m, m) = K_b(xs, xs) - K_b(xs, x) K_b^-1 K_b(x, xs)               or NULL   (not both var and cov)
 *   logdet[b], quad[b]: as gh_chol_objective_batch, or NULL.
 * A failed member's rows are NaN; GH_OK whenever every member was evaluated.  Any pointer may be host or device memory.
 * The handle is left NOT computed. */
int  gh_chol_predict_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                           const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                           const double* xs, int64_t m, double* mu, double* var, double* cov,
                           double* logdet, double* quad, int64_t* info);
/* B rounds of compute + gh_chol_sample_conditional at B parameter vectors, one device call (replaces the loop of
 * set_parameter_vector + GP.sample_conditional, gp.py, with utils.py:11-33 behind each round).  params, x, yerr, r, xs, info: as
 * gh_chol_predict_batch, whose launches form mu[b] and cov[b]; the covariances stay on the device in their (B, m, m) layout and
 * are factored there by ONE batched gh_dev_pstrf; then one GEMM per member:
 *   draws[b] (nz, m) = mu[b] + z[b][:, :rank[b]] L_b[:, :rank[b]]^T        z (B, nz, m): standard normals supplied by the caller.
 * tol < 0: member b's default m * eps * max diag K_b(xs, xs).  mu (B, m) or NULL; fac (B, m, m) or NULL; rank (B) int64.  A failed
 * member (info[b] != 0) has NaN draws (and mu, fac) and rank[b] = -1; GH_OK whenever every member was evaluated.  Any pointer may
 * be host or device memory.  The handle is left NOT computed. */
int  gh_chol_sample_conditional_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                      const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                      const double* xs, int64_t m, const double* z, int64_t nz, double tol,
                                      double* mu, double* draws, double* fac, int64_t* rank, int64_t* info);
/* B rounds of compute gp.py:303-337 + log_likelihood :369-397 + the kernel part of grad_log_likelihood :429-466, one device
 * call.  params, x, yerr, r, info: as gh_chol_objective_batch.  which: (gh_kernel_size(k)) mask shared by all members.
 *   logdet[b], quad[b]      as gh_chol_objective_batch (logdet bit-identical to it)
 *   grad[b] (P)             1/2 sum_ij A_ij dK_ij/dtheta_p, A = alpha alpha^T - K_b^-1; masked entries exactly 0
 *   alpha[b] (n)            K_b^-1 r_b                                     (or NULL)
 *   diagA[b] (n)            diag(A)                                        (or NULL)
 * A failed member has info[b] != 0 and NaN in every output row; GH_OK whenever every member was evaluated.  Any pointer
 * may be host or device memory.  The handle is left NOT computed. */
int  gh_chol_objective_grad_batch(gh_chol* s, gh_kernel* k, const double* params, int32_t nbatch,
                                  const double* x, int64_t n, int32_t ndim, const double* yerr, const double* r,
                                  const uint32_t* which, double* logdet, double* quad, double* grad,
                                  double* alpha, double* diagA, int64_t* info);
/* Checkpointing of the device factor (the reference's BasicSolver pickles COMPUTED,
 * tests/test_pickle.py:21-36, because its factor is a NumPy array, basic.py:68): the lower
 * triangle of L packed by rows (gh_chol_factor_size() = n (n + 1) / 2 doubles) and the inverses of
 * its 128 x 128 diagonal blocks (gh_chol_dinv_size() doubles).  import_factor() rebuilds a computed
 * handle from them plus the inputs x (n, ndim) that predict / grad evaluate kernels against.  packed_lower, dinv_out / dinv_in
 * and x: host or device memory. */
int64_t gh_chol_factor_size(const gh_chol* s);
int64_t gh_chol_dinv_size(const gh_chol* s);
int  gh_chol_export_factor(gh_chol* s, double* packed_lower, double* dinv_out);
int  gh_chol_import_factor(gh_chol* s, int64_t n, int32_t ndim, const double* x,
                           const double* packed_lower, const double* dinv_in, double logdet);
/* memory management of a long-lived handle: trim() frees the transient work buffers of predict /
 * grad / get_inverse (up to 3 x 8 N^2 bytes) and the buffers of objective_batch / predict_batch / objective_grad_batch / sample_conditional(_batch), and keeps the factor;
 * release_buffers() frees everything but the handle (streams, events) -- the next compute() re-allocates. */
void gh_chol_trim(gh_chol* s);
void gh_chol_release_buffers(gh_chol* s);
/* profile counters of the last compute(): see george_amd/csrc/gh_chol.hip */
typedef struct gh_chol_profile {
  double ms_total;          /* build + factor, device time                     */
  double ms_build;          /* kernel-matrix build                             */
  double ms_panel;          /* potf2 + trsm + inner updates                    */
  double ms_trailing;       /* sum of trailing-update (SYRK) launches: the wide lower-triangular ones on the main stream
                             * (one per inner panel, or one per group of panels -- the two-level driver's far launches) */
  double trailing_flops;    /* algorithmic flops of those launches             */
  int64_t n_trailing;       /* number of trailing-update launches              */
  double ms_solve;          /* last dot_solve / solve                          */
  double ms_update_union;   /* time during which ANY trailing-update launch ran (wide SYRKs on the main
                             * stream + block-column / in-group / next-group GEMMs on the chain stream): union of their intervals */
  double update_flops;      /* algorithmic flops of all those launches          */
  double ms_append_relayout; /* last gh_chol_append(): moving the factor into buffers of the new Np (0: it stayed in place) */
  double reserved[1];       /* [0]: last gh_chol_remove() of a profiled handle: gathering the kept rows and columns into the new buffers, ms */
} gh_chol_profile;
int  gh_chol_get_profile(const gh_chol* s, gh_chol_profile* out);
/* per trailing-update launch of the last profiled compute(): (start ms, end ms, algorithmic flops), times from the
 * start of compute() by HIP events on the stream each launch went to; *n_out = number of launches recorded.  The
 * union of these intervals is gh_chol_profile.ms_update_union (bench.py's roofline: reproducible from them). */
int  gh_chol_get_update_intervals(const gh_chol* s, double* out /* 3 * max_launches */, int32_t max_launches, int32_t* n_out);

/* ------------------------------------------------------------ HODLR solver
 * Replaces HODLRSolver (src/george/solvers/hodlr.py:13-76), the pybind11
 * `Solver` (src/george/solvers/_hodlr.cpp:38-110) and hodlr::Node
 * (include/george/hodlr.h:13-258).  x, yerr, b, y, r, xs and the array results are host or device memory ("Pointer kinds" at
 * the top of this file; a device y of gh_hodlr_dot_solve is read where it lies); *logdet_out, *out of gh_hodlr_dot_solve, which
 * and ranks_out / n_out are host memory. */
typedef struct gh_hodlr_opts {
  int32_t device;
  int32_t min_size;      /* hodlr.py:43 default 100 */
  int32_t seed;          /* hodlr.py:43 default 42  */
  int32_t max_rank;      /* cap on the ACA rank per block; 0 = default (256) */
  double  tol;           /* hodlr.py:43 default 0.1 */
  int32_t reserved[4];
} gh_hodlr_opts;

int  gh_hodlr_create(const gh_hodlr_opts* opts, gh_hodlr** out);
void gh_hodlr_destroy(gh_hodlr* h);
int  gh_hodlr_compute(gh_hodlr* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                      const double* yerr, double* logdet_out);
int  gh_hodlr_solve(gh_hodlr* h, const double* b, int64_t nrhs, double* out);  /* (n, nrhs) row-major */
int  gh_hodlr_dot_solve(gh_hodlr* h, const double* y, double* out);
int  gh_hodlr_get_inverse(gh_hodlr* h, double* out /* n*n */);
int  gh_hodlr_ranks(const gh_hodlr* h, int32_t* ranks_out, int32_t max_out, int32_t* n_out);
/* Fused device-resident forms of the GP glue on a computed handle, the HODLR counterparts of gh_chol_predict / gh_chol_grad.
 * Both work over column strips of n x Ct doubles (Ct a multiple of 64 chosen from a byte budget, gh_hodlr_predict.hip), leave the factor,
 * log|K| and the computed state untouched, synchronise once at the end, and refuse a sub-tree handle of the multi-device split. */
/* mu = K(xs,x) K^-1 r ; var = diag K(xs,xs) - diag(K(xs,x) K^-1 K(x,xs)) ; cov = K(xs,xs) - K(xs,x) K^-1 K(x,xs)
 * (gp.py:482-545 with apply_inverse = hodlr.h:107-114).  k may differ from the kernel of compute() (GP.predict(kernel=...)).
 * var / cov may be NULL (not both non-NULL).  cov keeps K(x,xs) and K^-1 K(x,xs) whole on
 * the device (2 * 8 * n * m bytes): GH_ERR_NOMEM when they do not fit. */
int  gh_hodlr_predict(gh_hodlr* h, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t m,
                      double* mu /* m */, double* var /* m or NULL */, double* cov /* m*m or NULL */);
/* alpha = K^-1 r; A = alpha alpha^T - K^-1 (the solver's K^-1: solve against the identity, _hodlr.cpp get_inverse);
 * grad[p] = 1/2 sum_ij A_ij dK_ij/dtheta_p over ALL (i, j) for the parameters selected by `which` (others exactly 0);
 * diagA = diag(A).  (gp.py:429-466).  K^-1 is never formed as a whole; two calls give the same bits. */
int  gh_hodlr_grad(gh_hodlr* h, gh_kernel* k, const uint32_t* which, const double* r,
                   double* grad /* size */, double* alpha /* n or NULL */, double* diagA /* n or NULL */);

/* ------------------------------------------------------------ Vecchia solver
 * The nearest-neighbour (Vecchia) approximation p(y) ~ prod_i p(y_i | y_c(i)): c(i) holds at most m points among the
 * predecessors of i in the order the points are given in.  With b_i = K_cc^-1 k_ci and f_i = k_ii - k_ci^T b_i the precision is
 * Q = (I - B)^T F^-1 (I - B), B strictly lower triangular with the b_i as rows, F = diag(f).  Every predecessor in c(i)
 * (m >= n - 1) gives the dense answers up to rounding.  O(n m^3) flops, O(n m) memory; no reference counterpart.  Fixed-order
 * sums throughout: two calls give the same bits.  (george_amd/csrc/gh_vecchia.hip)
 * x, yerr, b, y, r, xs, diag_rows and the array results mu, var, cov, out, grad, alpha, diagA are host or device memory ("Pointer kinds" at
 * the top of this file); *logdet_out, *out of gh_vecchia_dot_solve, which, nbr, qnbr and table_out are host memory.  A compute()
 * on device x always drops a kept search grid (the points cannot be compared on the host). */
typedef struct gh_vecchia gh_vecchia;
typedef struct gh_vecchia_opts {
  int32_t device;
  int32_t m;             /* neighbours per point, 1 .. 64 */
  int32_t reserved[2];
} gh_vecchia_opts;
/* GH_ERR_BAD_ARG for m < 1 or m > 64 (host check, before any device is touched) */
int  gh_vecchia_create(const gh_vecchia_opts* opts, gh_vecchia** out);
void gh_vecchia_destroy(gh_vecchia* h);
/* nbr: host array, row i = the neighbours of point i, each -1 (padding, anywhere in the row) or in [0, i), no duplicates in a
 * row, any order; checked on the host before any launch (GH_ERR_BAD_ARG).  *logdet_out = sum_i log f_i.  A pivot of a K_cc or
 * an f_i that is not positive and finite: GH_ERR_NOT_PD, gh_vecchia_info() = the lowest such point, and the handle is not
 * computed. */
int  gh_vecchia_compute(gh_vecchia* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                        const int32_t* nbr /* n*m */, double* logdet_out);
int64_t gh_vecchia_info(const gh_vecchia* h);     /* 1-based index of the failing (test) point after GH_ERR_NOT_PD, else 0 */
int  gh_vecchia_solve(gh_vecchia* h, const double* b, int64_t nrhs, double* out);   /* out = Q b; (n, nrhs) row-major */
int  gh_vecchia_dot_solve(gh_vecchia* h, const double* y, double* out);             /* y^T Q y = sum_i e_i^2 / f_i */
/* grad[p] = sum_i sum_jk W(i)_jk dk(x_j, x_k)/dtheta_p over the blocks c(i) + {i}, with W(i) the derivative of
 * log p(y_i | y_c(i)) with respect to the block (parameters not selected by `which`: exactly 0); alpha = Q r;
 * diagA_j = 2 sum over the blocks that hold j of W_jj.  The layout of gh_chol_grad, and its values when m >= n - 1. */
int  gh_vecchia_grad(gh_vecchia* h, gh_kernel* k, const uint32_t* which, const double* r,
                     double* grad /* size */, double* alpha /* n or NULL */, double* diagA /* n or NULL */);
/* Leave-one-out cross-validation of the Vecchia density, the Gaussian with precision Q = sum_i u_i u_i^T / f_i (u_i = [-b_i; 1] on
 * the block c(i) + {i}); exact for that density.  With c_j = Q_jj = 1/f_j + sum over column j of B of b^2 / f_row and alpha = Q r:
 *   resid[j] = alpha_j / c_j = y_j - mu_j,   var[j] = 1 / c_j,
 *   lpd[j]   = 1/2 log c_j - 1/2 alpha_j^2 / c_j - 1/2 log 2 pi;      *lpd_sum = sum_j lpd[j]
 * and, with w = 1/2 (1 + alpha^2 / c) / c, a = alpha / c and M = diag(w) - 1/2 (a r^T + r a^T):  d lpd_sum = sum_i d[u^T M u / f],
 * one closed form per block: g = M u, h = A^-1 g, W(i) = (u.g / f^2) u u^T - (1/f) (h u^T + u h^T), and
 *   grad[p]  = sum_i sum_jk W(i)_jk dk(x_j, x_k)/dtheta_p  for the parameters selected by `which` (others exactly 0)
 *   v (n)    = Q a: d lpd_sum / d mean_j;      diagB_j = sum over the blocks that hold j of W_jj: d lpd_sum / d K_jj.
 * The layout of gh_chol_loo, and its values when m >= n - 1; for smaller m this is the leave-one-out of the approximate density,
 * as far from the dense one as Q is from K^-1.  which == NULL: values only (grad, v and diagB must be NULL; O(n m), no block is
 * rebuilt); otherwise about the cost of gh_vecchia_grad.  Nothing of size n x n.  *lpd_sum and which are host memory, the
 * vectors host or device memory.  A block that is not positive definite (only with another kernel than compute()'s) adds nothing
 * to grad and diagB.  Two calls give the same bits. */
int  gh_vecchia_loo(gh_vecchia* h, gh_kernel* k, const uint32_t* which /* NULL: values only */, const double* r,
                    double* lpd_sum, double* resid /* n */, double* var /* n */, double* lpd /* n or NULL */,
                    double* grad /* size, or NULL */, double* v /* n or NULL */, double* diagB /* n or NULL */);
/* The expected (Fisher) information of the Vecchia likelihood (Guinness 2021), a sum of one closed form per block: with
 * u = [-b_i; 1], L the factor of K_cc and D_a a derivative matrix restricted to the block c(i) + {i},
 *   v_a = D_a u,  df_a = u^T v_a,  w_a = L^-1 (v_a)[:c],   F_ab = sum_i 1/2 df_a df_b / f_i^2 + (w_a . w_b) / f_i.
 * D_a: first the n_diag diagonal matrices diag(diag_rows[a]) (how a white-noise model enters; (n_diag, n) row-major in the order
 * of compute()'s points, host or device memory, NULL with n_diag == 0), then dK/dtheta of every kernel parameter (the lower index
 * is the first argument).  out: (n_diag + size)^2 row-major, host or device memory, exactly symmetric; a kernel parameter not
 * selected by `which` (host, size entries) has a row and a column of exactly 0.  At m >= n - 1 this is the dense
 * 1/2 tr(K^-1 D_a K^-1 D_b) of gh_chol_fisher up to rounding; for smaller m it is the information of the approximate likelihood
 * with each conditioning set's covariance taken as K_cc, a different quantity.  One pass over the blocks, about the cost of
 * gh_vecchia_grad; nothing of size n x n.  At most 64 planes in one call -- n_diag plus the selected kernel parameters -- else
 * GH_ERR_BAD_ARG.  A block that is not positive definite (only with another kernel than compute()'s) adds nothing.  Two calls
 * give the same bits. */
int  gh_vecchia_fisher(gh_vecchia* h, gh_kernel* k, const uint32_t* which, const double* diag_rows /* n_diag*n or NULL */,
                       int32_t n_diag, double* out /* (n_diag + size)^2 */);
/* mu = K(xs,x) Q r; var = diag K(xs,xs) - colsumsq(V), cov = K(xs,xs) - V^T V with V = F^-1/2 (I - B) K(x,xs).  var / cov may be
 * NULL (not both non-NULL); k may differ from the kernel of compute().  Strips of test points sized to a byte budget; cov keeps
 * K(x,xs), V and the m x m result on the device: GH_ERR_NOMEM when the budget does not hold them. */
int  gh_vecchia_predict(gh_vecchia* h, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t m,
                        double* mu /* m */, double* var /* m or NULL */, double* cov /* m*m or NULL */);
/* Local (nearest-neighbour) prediction: test point c is conditioned on the data points of row c of qnbr alone,
 *   mu = k_c^T (K_cc + yerr^2)^-1 r_c,   var = k** - k_c^T (K_cc + yerr^2)^-1 k_c,
 * a proper conditional variance; one Cholesky of at most 64 x 64 per test point, O(M mq^3) whatever n, no n-sized work space.
 * x and yerr are the handle's copies from compute().  qnbr: host array, each entry -1 (padding, anywhere in the row) or in
 * [0, n), no duplicates in a row, any order; checked on the host before any launch (GH_ERR_BAD_ARG).  1 <= mq <= 64,
 * independent of the handle's m.  A row without a valid entry gives mu = 0, var = k**.  k_data builds K_cc (the lower data
 * index is the first argument), k_cross builds k_c = k(x_j, t) and k** = k(t, t); they may be the same object; a dimension
 * mismatch on either is GH_ERR_DIM.  A pivot that is not positive and finite or a variance that is not finite: GH_ERR_NOT_PD,
 * gh_vecchia_info() = the lowest such test point, the handle stays computed and no output is defined.  A variance that rounds
 * to a tiny negative value is returned as computed.  A test point's result does not depend on the other test points. */
int  gh_vecchia_predict_local(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r /* n: y - mean */,
                              const double* xs, int64_t M, const int32_t* qnbr /* M*mq */, int32_t mq,
                              double* mu /* M */, double* var /* M or NULL */);
/* The exact nearest-neighbour search on the device (george_amd/csrc/gh_vecchia_search.hip); it needs no solver handle.  Row c of
 * table_out (host, (nq, m) int32) = the min(#eligible, m) points of x nearest to q[c] by squared Euclidean distance, ties going
 * to the lower index, ascending by index, then -1.  Point j is eligible for query c when j < limit[c]; limit == NULL: every
 * point (limit[c] = c with q = x gives the default table of gh_vecchia_compute).  d2 = sum_k (x_k - q_k)^2 from k = 0 on without
 * fused multiply-adds: for ndim <= 7 the double NumPy's ((x - q)**2).sum(-1) gives; for more dimensions NumPy adds in another
 * order and the rows are a nearest set under THIS distance.  A cell grid over the first min(ndim, 3) coordinates aimed at
 * `occupancy` points per cell (0: automatic; >= n: one cell, a brute-force search) prunes exactly.  x, q and limit may be host
 * or device memory.  Host checks before any device call: GH_ERR_BAD_ARG for m outside 1 .. 64, a null pointer, a negative size
 * or occupancy; GH_ERR_DIM for ndim outside 1 .. GH_MAX_NDIM; nq == 0 or n == 0 gives a table of -1 and touches no device.  Two
 * calls give the same bits. */
int  gh_vecchia_search(int32_t device, const double* x, int64_t n, int32_t ndim, const double* q, int64_t nq,
                       const int64_t* limit /* nq or NULL */, int32_t m, int32_t occupancy, int32_t* table_out /* nq*m */);
/* gh_vecchia_predict_local with the table made by that search over the handle's own x: the grid is kept in the handle and built
 * again at the first search after a compute() on other points (n (8 ndim + 4) bytes and 4 bytes per cell on the device, the
 * points once more on the host); the table and its row counts stay on the device.  table_out (host, M*mq, or NULL) receives the
 * table, in the handle's point numbering.  Errors and gh_vecchia_info() as gh_vecchia_predict_local. */
int  gh_vecchia_predict_local_search(gh_vecchia* h, gh_kernel* k_data, gh_kernel* k_cross, const double* r /* n: y - mean */,
                                     const double* xs, int64_t M, int32_t mq, int32_t occupancy,
                                     double* mu /* M */, double* var /* M or NULL */, int32_t* table_out /* M*mq or NULL */);

/* ------------------------------------------------------------ inducing-point solver
 * The low-rank approximations DTC and FITC, and Titsias' variational bound (VFE), through m inducing inputs u, the complement of the Vecchia solver: near-exact for
 * smooth kernels, mediocre for rough ones.  With s_i = yerr_i^2, K_uu the symmetric build over u (the lower index is the first
 * argument) and K_fu = K(x, u) (the data point is the first argument):
 *   K_uu + jitter I = L_u L_u^T,   V = L_u^-1 K_uf (m x n),   q_i = |V[:, i]|^2,
 *   lambda_i = s_i + phi max(k(x_i, x_i) - q_i, 0)      (phi = 0: DTC, 1: FITC),
 *   C = V^T V + diag(lambda)  -- the model covariance --,   A = I + V Lambda^-1 V^T = L_A L_A^T,   H = L_A^-1 V,
 *   log|C| = sum_i log lambda_i + 2 sum_j log (L_A)_jj,   t(b) = H Lambda^-1 b,
 *   C^-1 b = Lambda^-1 b - Lambda^-1 H^T t(b),   b^T C^-1 b = sum_i b_i^2 / lambda_i - |t(b)|^2.
 * O(n m^2) flops in GEMM shapes; nothing of size n x m is kept: the data points pass in strips, and the handle holds about five
 * m x m matrices (m padded to a multiple of 128; 2.7 GB at the cap m = 8192).  No reference counterpart.  Sums have a fixed
 * order (strips ascending on one stream): two calls give the same bits.  (george_amd/csrc/gh_inducing.hip)
 * The variational bound (variational = 1; lambda_i = s_i as DTC):
 *   F = log N(r | 0, C) - 1/2 tau,   tau = sum_i max(k(x_i, x_i) - q_i, 0) / s_i >= 0,
 * F <= the dense log-likelihood, and F does not decrease when an inducing input is added.  solve, dot_solve and predict are DTC's.
 * x, yerr, u, b, y, r, xs and the array results out, grad, alpha, diagA, mu, var, cov are host or device memory ("Pointer kinds"
 * at the top of this file), and so is ugrad; *logdet_out, *out of gh_inducing_dot_solve and of gh_inducing_trace_term and which
 * are host memory. */
typedef struct gh_inducing gh_inducing;
typedef struct gh_inducing_opts {
  int32_t device;
  int32_t method;        /* 0: DTC, 1: FITC */
  int32_t strip_points;  /* data points per strip: 0 = from a byte budget, else rounded up to a multiple of 128 */
  int32_t variational;   /* 0, or 1: the variational bound; with method 0 only */
} gh_inducing_opts;
/* GH_ERR_BAD_ARG for a method other than 0 / 1, a negative strip_points, a variational other than 0 / 1 or variational = 1 with
 * method = 1 (host checks, before any device is touched) */
int  gh_inducing_create(const gh_inducing_opts* opts, gh_inducing** out);
void gh_inducing_destroy(gh_inducing* h);
/* After GH_ERR_NOT_PD: +p when pivot p (1-based) of K_uu + jitter I failed, -p when pivot p of A failed; else 0. */
int64_t gh_inducing_info(const gh_inducing* h);
/* *out = tau of the last compute(), 0 when the bound is off (*logdet_out of compute() stays log|C| either way) */
int  gh_inducing_trace_term(const gh_inducing* h, double* out);
/* u: (m, ndim), 1 <= m <= 8192 (GH_ERR_BAD_ARG otherwise, a host check); jitter >= 0 is absolute.  A pivot of K_uu + jitter I or
 * of A that is not positive: GH_ERR_NOT_PD, gh_inducing_info() says which, and the handle is not computed. */
int  gh_inducing_compute(gh_inducing* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                         const double* u, int64_t m, double jitter, double* logdet_out);
int  gh_inducing_solve(gh_inducing* h, const double* b, int64_t nrhs, double* out);   /* out = C^-1 b; (n, nrhs) row-major */
int  gh_inducing_dot_solve(gh_inducing* h, const double* y, double* out);             /* y^T C^-1 y */
/* The likelihood gradient in the layout of gh_chol_grad: alpha = C^-1 r, diagA_i = alpha_i^2 - (C^-1)_ii, and with
 * P = K_uu^-1 K_uf (K_uu with its jitter), T = (P alpha) alpha^T - P C^-1 and one weight vector omega for the three objectives,
 * omega_i = 0 (DTC), diagA_i (FITC), -1 / s_i (the bound):  Z = T - P diag(omega), W = -1/2 Z P^T,
 *   grad[p] = sum_ij Z_ji dk(x_i, u_j)/dtheta_p + sum_jj' W_jj' dk(u_j, u_j')/dtheta_p + 1/2 sum_i omega_i dk(x_i, x_i)/dtheta_p
 * (parameters not selected by `which`: exactly 0; the clamp counts as inactive).  Under the bound this is the gradient of F, and
 * diagA_i = alpha_i^2 - (C^-1)_ii + max(k(x_i, x_i) - q_i, 0) / s_i^2, so that 1/2 diagA_i is dF / ds_i.  k: the kernel of compute(). */
int  gh_inducing_grad(gh_inducing* h, gh_kernel* k, const uint32_t* which, const double* r,
                      double* grad /* size */, double* alpha /* n or NULL */, double* diagA /* n or NULL */);
/* The same, and the gradient of the objective with respect to the inducing inputs, for all three objectives (d1: the derivative
 * in the first argument, d2: in the second; the absolute jitter is a constant, as in grad):
 *   ugrad[j, :] = sum_i Z_ji d2 k(x_i, u_j) + sum_b (W_jb + W_bj) d1 k(u_j, u_b)          (b = j included)
 * d2 k(x_i, u_j) is taken as the evaluator's d1 k(u_j, x_i): kernels are symmetric.  which == NULL: no kernel gradient (grad may
 * then be NULL too).  grad, alpha and diagA have the bits gh_inducing_grad gives.  ugrad takes Z and W from P itself -- a pass
 * over the strips for H Lambda^-1 P^T and P alpha, then Z_J^T = alpha_J (P alpha)^T - Lambda_J^-1 (P_J^T - H_J^T (H Lambda^-1 P^T))
 * - diag(omega_J) P_J^T and Z P^T = sum_J Z_J P_J^T -- since grad's own Z, a product with explicit inverse factors, is exact only
 * in sums over j.  Beside grad's work: one more pass of n m input-gradient evaluations, seven more strip GEMMs and two m x m ones
 * (counts); two more strips, one m x m matrix, an (m, ndim) buffer and the partial sums of the reduction on the device.  Host checks come before any device call:
 * GH_ERR_BAD_ARG for a null h, k, r or ugrad, or which without grad; GH_ERR_NOT_COMPUTED; GH_ERR_DIM. */
int  gh_inducing_grad_u(gh_inducing* h, gh_kernel* k, const uint32_t* which /* or NULL */, const double* r,
                        double* grad /* size, or NULL */, double* alpha /* n or NULL */, double* diagA /* n or NULL */,
                        double* ugrad /* m*ndim */);
/* Leave-one-out cross-validation of the DTC / FITC density N(r | 0, C), exact for it, from the low-rank form
 * C^-1 = D - R^T R (D = Lambda^-1, R = H D, m x n); the layout of gh_chol_loo and gh_vecchia_loo, and the dense values when u = x
 * without jitter:
 *   c_i = (C^-1)_ii = 1/lambda_i - |H[:, i]|^2 / lambda_i^2,   alpha = C^-1 r,
 *   resid[i] = alpha_i / c_i = y_i - mu_i,   var[i] = 1 / c_i,
 *   lpd[i]   = 1/2 log c_i - 1/2 alpha_i resid_i - 1/2 log 2 pi;      *lpd_sum = sum_i lpd[i]   (fixed order)
 * and, with w = 1/2 (1 + alpha resid) / c:  v = C^-1 resid (d lpd_sum / d mean_i), and with S = R diag(w) R^T, G1 = R P^T and
 * G3 = R diag(w D) P^T (three m x m sums over the strips)
 *   diagB_i = alpha_i v_i - (w_i D_i^2 - 2 w_i D_i |R[:, i]|^2 + R[:, i]^T S R[:, i])          (d lpd_sum / d C_ii)
 *   Z_J^T   = alpha_J (P v)^T + v_J (P alpha)^T - 2 (diag(w D^2)_J P_J^T - diag(w D)_J R_J^T G1 + R_J^T (S G1 - G3))
 *             - 2 phi diag(diagB)_J P_J^T,        W = -1/2 Z P^T
 *   grad[p] = sum_ij Z_ji dk(x_i, u_j)/dtheta_p + sum_jj' W_jj' dk(u_j, u_j')/dtheta_p + phi sum_i diagB_i dk(x_i, x_i)/dtheta_p:
 * gh_inducing_grad's reduction with 2 B, B = 1/2 (v alpha^T + alpha v^T) - C^-1 diag(w) C^-1, in the place of alpha alpha^T - C^-1
 * (parameters not selected by `which`: exactly 0; the clamp counts as inactive, the absolute jitter as a constant).  Under the
 * bound (variational = 1) this is the leave-one-out of the DTC density, with the bits of a method 0 handle: tau does not enter.
 * which == NULL: values only (grad, v and diagB must be NULL): one apply and one pass of one strip GEMM and one row kernel, about
 * one gh_inducing_dot_solve more.  Otherwise a second apply and a second pass: thirteen strip GEMMs and three m x m ones in all,
 * five strips and three m x m matrices beside the handle's on the device (counts, not measurements).  Nothing of size n x m or
 * n x n is kept.  *lpd_sum and which are host memory, the vectors host or device memory.  Host checks as gh_inducing_grad:
 * GH_ERR_BAD_ARG for a null h, k, r, lpd_sum, resid or var, which without grad, or grad, v or diagB without which, or more than
 * GH_MAX_GRAD parameters with which; GH_ERR_NOT_COMPUTED; GH_ERR_DIM.  k: the kernel of compute().  Two calls give the same bits,
 * and gh_inducing_grad and gh_inducing_grad_u return what they did before. */
int  gh_inducing_loo(gh_inducing* h, gh_kernel* k, const uint32_t* which /* NULL: values only */, const double* r,
                     double* lpd_sum, double* resid /* n */, double* var /* n */, double* lpd /* n or NULL */,
                     double* grad /* size, or NULL */, double* v /* n or NULL */, double* diagB /* n or NULL */);
/* The same for DTC, FITC and the bound: with V* = L_u^-1 K(u, xs), H* = L_A^-1 V*:  mu = H*^T t(r),
 * var = diag K(xs,xs) - colsumsq(V*) + colsumsq(H*),  cov = K(xs,xs) - V*^T V* + H*^T H*.  O(M m^2) whatever n, in strips of
 * test points; var / cov may be NULL (not both non-NULL); cov keeps its operands whole: GH_ERR_NOMEM over the strip budget.  k
 * may differ from the kernel of compute(). */
int  gh_inducing_predict(gh_inducing* h, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t M,
                         double* mu /* M */, double* var /* M or NULL */, double* cov /* M*M or NULL */);
/* The greedy max-min selection of inducing points on the device (george_amd/csrc/gh_inducing_select.hip); it needs no solver
 * handle.  idx[0] = first and dmin_i = +inf; for j = 1, 2, ..., min(m, n) - 1: dmin_i = min(dmin_i, d2(x_i, x_idx[j-1])), then
 * idx[j] = the index of the largest dmin, ties going to the LOWER index; data with fewer distinct points than picks is no special
 * case (every dmin is 0 and index 0 wins).  After the last pick dmin is updated once more: dmin_out (n doubles, host or device
 * memory, or NULL) is every point's squared distance to the chosen set and its maximum the squared fill distance.  That is the
 * rule of inducing_points() in george_amd/solvers/inducing.py, whose choice of `first` (the point nearest the centroid) stays
 * with the caller.  d2 = sum_k (x_ik - c_k)^2 from k = 0 on without fused multiply-adds: for ndim <= 7 the double NumPy's
 * ((x - c)**2).sum(-1) gives, so the sequence is the host routine's; for more dimensions NumPy adds in another order and the
 * result is the greedy sequence under THIS distance.  A d2 that is not a number never lowers a dmin.  m is not capped: m >= n
 * gives a max-min ordering of all n points.  One kernel launch per pick on one stream, no host synchronisation between them;
 * O(n m) work, n (8 ndim + 8) bytes on the device beside x.  x may be host or device memory; idx_out (min(m, n) int64) is host
 * memory.  Host checks before any device call: GH_ERR_BAD_ARG for m < 1, n < 0, n > 0x7ffffff0, a null idx_out, a null x with
 * n > 0, or first outside [0, n) when n > 0; GH_ERR_DIM for ndim outside 1 .. GH_MAX_NDIM; n == 0 writes nothing and touches no
 * device.  Two calls give the same bits. */
int  gh_inducing_select(int32_t device, const double* x, int64_t n, int32_t ndim, int64_t first, int64_t m,
                        int64_t* idx_out /* min(m, n) */, double* dmin_out /* n or NULL */);

/* --------------------------------------------------- dense solver on several GPUs
 * The BasicSolver protocol of /root/reference/src/george/solvers/basic.py:51-102 (compute, log-determinant,
 * dot_solve, apply_inverse) for ONE process that owns several MI355X: 2-D block-cyclic tiles (tile (I, J)
 * on rank (I mod pr) * pc + (J mod pc)), one host thread and one stream per device, panels moved with RCCL
 * over xGMI (grouped ncclSend / ncclRecv on the communicator of ncclCommInitAll; librccl is dlopen'ed at the
 * first create).  The reference has nothing here: it is single-process, single-host (gp.py:327).  The
 * multi-PROCESS form of the same algorithm (one rank per GPU under torch.distributed; what bench.py
 * --gpus N runs) is george_amd/distributed.py.  Default grid: pr = n_dev, pc = 1 -- whole tile rows per rank in
 * "snake" order (0 1 .. P-1 P-1 .. 1 0: equal shares of the lower triangle) -- because on the xGMI full mesh
 * the critical chain potrf(k) -> TRSM -> block column k+1 -> potrf(k+1) then moves only two nb x nb tiles per
 * step, over all links at once (george_amd/csrc/gh_mgpu.hip; profiles/r04/scale_model.md).  The whole solver
 * protocol is offered: the O(N^2 R) operations are left-looking tile sweeps on the sharded factor. */
typedef struct gh_mgpu gh_mgpu;
enum {
  GH_MGPU_RCCL = 0,      /* RCCL point-to-point over xGMI; one rank per physical device                      */
  GH_MGPU_COPY = 1       /* peer copies behind events; the same device may be listed several times ("virtual
                            devices": exercises the n_dev-rank ownership and ordering logic on one GPU)     */
};
enum {
  GH_MGPU_PLAIN_CYCLIC = 1,  /* pc == 1: tile row I on rank I mod pr instead of the snake order                    */
  /* (2 and 4 are the timing aids GH_MGPU_CHAIN_ONLY / GH_MGPU_TRACE: include/george_amd_debug.h -- a chain-only compute()
   *  returns GH_OK with numbers that mean nothing, which has no place among the drop-in's flags)                          */
  GH_MGPU_ONE_COMM     = 8   /* GH_MGPU_RCCL: the bulk gather on the chain's stream and communicator (one communicator in
                                flight at a time) -- chosen by itself when the two streams of a rank do not dispatch
                                independently (gh_mgpu_comm_mode tells which)                                         */
};
typedef struct gh_mgpu_opts {
  int32_t n_dev;             /* 1..16 */
  int32_t devices[16];       /* HIP device ordinals, rank i runs on devices[i] */
  int32_t pr, pc;            /* process grid, pr * pc == n_dev; 0, 0: n_dev x 1 (whole tile rows per rank) */
  int32_t nb;                /* tile edge, multiple of 128; 0: 1024 from N = 24576 up, else 512 */
  int32_t transport;         /* GH_MGPU_RCCL | GH_MGPU_COPY */
  int32_t flags;             /* GH_MGPU_PLAIN_CYCLIC | GH_MGPU_ONE_COMM (| the timing aids of george_amd_debug.h) */
  int32_t reserved[3];
} gh_mgpu_opts;
int  gh_mgpu_create(const gh_mgpu_opts* opts, gh_mgpu** out);      /* communicators + an all-reduce self-check */
void gh_mgpu_destroy(gh_mgpu* h);
/* basic.py:51-70 on the grid: every rank builds its own tiles from (kernel, x, yerr) -- host pointers --
 * and the factor stays sharded; GH_ERR_NOT_PD + gh_mgpu_info() as gh_chol_compute */
int  gh_mgpu_compute(gh_mgpu* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                     const double* yerr, double* logdet_out);
int64_t gh_mgpu_info(const gh_mgpu* h);
int  gh_mgpu_grid(const gh_mgpu* h, int32_t* pr, int32_t* pc, int32_t* nb);
int  gh_mgpu_comm_mode(const gh_mgpu* h);   /* 2: chain and bulk gather on their own communicators; 1: GH_MGPU_ONE_COMM; 0: GH_MGPU_COPY */
int  gh_mgpu_owner(const gh_mgpu* h, int64_t tile_row, int64_t tile_col);              /* rank that holds tile (I, J); -1 on bad arguments */
/* all of the following take HOST pointers; every right-hand side of a call is swept together (chunks of 2048 columns) */
int  gh_mgpu_dot_solve(gh_mgpu* h, const double* y, double* out);                     /* basic.py:89-102 */
int  gh_mgpu_solve(gh_mgpu* h, const double* b, int64_t nrhs, double* out);           /* basic.py:72-87; (n, nrhs) row-major, may alias */
int  gh_mgpu_apply_sqrt(gh_mgpu* h, const double* r, int64_t nrows, double* out);     /* basic.py:104-114; r, out: (nrows, n) */
int  gh_mgpu_get_inverse(gh_mgpu* h, double* out /* n*n */);                          /* basic.py:116-121 */
/* gp.py:482-545 on the sharded factor (forward sweep only: K* K^-1 K*^T = V^T V with V = L^-1 K(x, xs));
 * var / cov may be NULL; cov is offered for m <= 2048 */
int  gh_mgpu_predict(gh_mgpu* h, gh_kernel* k, const double* r /* n: y - mean */, const double* xs, int64_t m,
                     double* mu /* m */, double* var /* m or NULL */, double* cov /* m*m or NULL */);
/* --------------------------------------------------- HODLR solver, tree split over several GPUs
 * hodlr::Node (include/george/hodlr.h:29-254) with the top log2(n_dev) levels of the tree shared and the
 * n_dev sub-trees below them -- independent of each other (hodlr.h:75-103: a node's factorisation touches
 * its own rows only) -- one per device.  ONE process, a host thread per device.  Per compute():
 *   - the ACA of each of the n_dev - 1 top nodes runs on one device against the whole point set, and every
 *     device pulls the rows it owns of each ancestor's factors (peer copies, N x r doubles per node in all);
 *   - every device builds and factors its sub-tree (the single-GPU code on rows [row0, row0 + n_p)), carrying
 *     the ancestors' U rows along as extra right-hand-side columns;
 *   - a top node's 2r x 2r core needs V^T U summed over the devices below it: 2r x C doubles exchanged
 *     through pinned host memory per level -- the only data-path exchange, also in every solve.
 * Same node-by-node random streams as the single-GPU solver (a node's generator is keyed by its position
 * in the global tree), so ranks and results agree with gh_hodlr_* to rounding.  n_dev must be a power of
 * two and every top node internal (N / n_dev >= 2 min_size); x, yerr, b, y are HOST pointers.  The same
 * device may be listed several times ("virtual devices": the split is then exercised on one GPU).
 * The reference has nothing here (single process, single thread). */
typedef struct gh_hodlr_mgpu gh_hodlr_mgpu;
typedef struct gh_hodlr_mgpu_opts {
  int32_t n_dev;             /* 1, 2, 4, 8 or 16 */
  int32_t devices[16];       /* HIP device ordinals; sub-tree p (rows in tree order) lives on devices[p] */
  int32_t min_size;          /* as gh_hodlr_opts */
  int32_t seed;
  int32_t max_rank;
  double  tol;
  int32_t reserved[4];
} gh_hodlr_mgpu_opts;
int  gh_hodlr_mgpu_create(const gh_hodlr_mgpu_opts* opts, gh_hodlr_mgpu** out);
void gh_hodlr_mgpu_destroy(gh_hodlr_mgpu* h);
int  gh_hodlr_mgpu_compute(gh_hodlr_mgpu* h, gh_kernel* k, const double* x, int64_t n, int32_t ndim,
                           const double* yerr, double* logdet_out);                          /* hodlr.h:75-103 */
int  gh_hodlr_mgpu_solve(gh_hodlr_mgpu* h, const double* b, int64_t nrhs, double* out);      /* hodlr.h:107-114; (n, nrhs) row-major */
int  gh_hodlr_mgpu_dot_solve(gh_hodlr_mgpu* h, const double* y, double* out);                /* hodlr.h:116-120 */
/* ranks of all internal nodes, level by level, left to right (the order gh_hodlr_ranks uses) */
int  gh_hodlr_mgpu_ranks(const gh_hodlr_mgpu* h, int32_t* ranks_out, int32_t max_out, int32_t* n_out);
/* host logic only, no device needed: the rows of every sub-tree of an n-point tree split over n_dev devices (hodlr.h:47-64
 * applied log2(n_dev) times) and, per sub-tree level, the index of each sub-tree's first internal node in the global
 * level (seed_off: n_dev x max_levels, may be NULL); *n_levels = levels of the deepest sub-tree */
int  gh_hodlr_mgpu_layout(int64_t n, int32_t n_dev, int32_t min_size, int64_t* row0, int64_t* nrows,
                          int32_t* seed_off, int32_t max_levels, int32_t* n_levels);
/* rows [row0[p], row0[p] + nrows[p]) live on devices[p]; arrays of n_dev entries (after compute()) */
int  gh_hodlr_mgpu_rows(const gh_hodlr_mgpu* h, int64_t* row0, int64_t* nrows);

/* ------------------------------------------- device-level tile operations
 * Building blocks of the blocked factorisation on DEVICE pointers and an
 * explicit hipStream_t (passed as void*; NULL = default stream).  Used by the
 * multi-GPU 2-D block-cyclic driver (george_amd/distributed.py), which moves
 * panels between ranks with torch.distributed (RCCL) in between.  Leading
 * dimensions are in elements; all sizes must be multiples of 128. */
/* out[r, c] = k(x[row0+r], x[col0+c]) (+ yerr[row0+r]^2 where row0+r == col0+c); x / yerr are the
 * full n-point device arrays, rows / columns past n are identity padding */
int gh_dev_kmat_block(gh_kernel* k, const double* x, int64_t n, int32_t ndim, const double* yerr,
                      int64_t row0, int64_t nrows, int64_t col0, int64_t ncols,
                      double* out, int64_t ldo, void* stream);
/* y = beta*y + alpha * A x (trans == 0; A is m x n row-major) or alpha * A^T x (trans != 0) */
int gh_dev_gemv(const double* a, int64_t lda, int64_t m, int64_t n, int32_t trans,
                const double* x, double* y, double alpha, double beta, void* stream);
/* z = L^-1 w for the n x n lower-triangular block `l` factored by gh_dev_potrf_block (`dinv` = its
 * diagonal-block inverses): one chained launch (gh_chol.hip, trsv_fwd_chain_direct; w and z must be different arrays).  `scratch` needs
 * (n/128 + 1) * 4 bytes of device memory, zeroed here.  w is read only. */
int gh_dev_trsv_lower(const double* l, int64_t ldl, const double* dinv, int64_t n,
                      const double* w, double* z, void* scratch, void* stream);
/* x = L^-T w for the same block (trsv_bwd_chain); same scratch; w is read only.  After either call
 * ((int32_t*)scratch)[n/128] != 0 means a workgroup gave up waiting for its predecessor (2 s). */
int gh_dev_trsv_lower_t(const double* l, int64_t ldl, const double* dinv, int64_t n,
                        const double* w, double* x, void* scratch, void* stream);
/* in-place lower Cholesky of the n x n block `a`; dinv receives the inverses of
 * its 128x128 diagonal blocks, (n/128) x 128 x 128; *info_dev (device int64) is
 * set to base_index + failing pivot (1-based) when not positive definite. */
int gh_dev_potrf_block(double* a, int64_t lda, int64_t n, double* dinv,
                       int64_t* info_dev, int64_t base_index, void* stream);
/* a21 (m x n) <- a21 * L11^-T using L11 (n x n, lower) and its diagonal-block inverses */
int gh_dev_trsm_right(const double* l11, int64_t ld11, const double* dinv,
                      double* a21, int64_t lda, int64_t m, int64_t n, void* stream);
/* c (m x n) -= a (m x k) * b (n x k)^T ; lower != 0: only tiles on/below the diagonal of the
 * square c are updated (SYRK-shaped, a and b rows aligned with c rows/cols). */
int gh_dev_gemm_nt(double* c, int64_t ldc, const double* a, int64_t lda,
                   const double* b, int64_t ldb, int64_t m, int64_t n, int64_t k,
                   int32_t lower, void* stream);
/* the same update on a STAIRCASE-shaped c, as ONE launch: row group g (group_rows rows of c and of a, g = 0 .. n_groups-1) is
 * updated over its first group_cols[g] columns, c[g-th rows, 0:group_cols[g]) -= a[g-th rows] * b[0:group_cols[g])^T; group_cols
 * (a HOST array) is non-decreasing, everything a multiple of 128.  The per-rank trailing update of a solver that owns whole tile
 * rows: every tile row reaches as far as its own diagonal tile.  Bit-identical to one gh_dev_gemm_nt per group. */
int gh_dev_gemm_nt_stair(double* c, int64_t ldc, const double* a, int64_t lda, const double* b, int64_t ldb,
                         int64_t group_rows, int32_t n_groups, const int64_t* group_cols, int64_t k, void* stream);
/* general form: c = beta*c + alpha * sum_k A(m,k) B(n,k); by default A(m,k) = a[m*lda + k] and
 * B(n,k) = b[n*ldb + k] ("k-major"); flags select the transposed layouts, SYRK-style lower-only
 * tile sets and k-range clipping for triangular operands. */
enum {
  GH_GEMM_A_MMAJOR = 1,   /* A(m,k) = a[k*lda + m]                                   */
  GH_GEMM_B_NMAJOR = 2,   /* B(n,k) = b[k*ldb + n]                                   */
  GH_GEMM_LOWER    = 4,   /* m >= n: only tiles on/below the diagonal (a lower trapezoid) */
  GH_GEMM_KLO_MAX  = 8,   /* k starts at max(tile row0, tile col0)                   */
  GH_GEMM_KHI_COL  = 16,  /* k ends at tile col0 + 128                               */
  GH_GEMM_KHI_ROW  = 32   /* k ends at tile row0 + 128                               */
};
int gh_dev_gemm(double* c, int64_t ldc, const double* a, int64_t lda,
                const double* b, int64_t ldb, int64_t m, int64_t n, int64_t k,
                double alpha, double beta, int32_t flags, void* stream);
/* Diagonally pivoted Cholesky with rank truncation (LAPACK dpstrf's job; the factorisation that replaces the SVD of
 * utils.py:11-33 for sampling, gp.py sample_conditional / sample), batched: nbatch symmetric m x m matrices at a + b * stride_a
 * (any m >= 1, any lda >= m; nothing needs to be a multiple of 128).  No rows or columns are swapped.  Per member, with d = diag(A)
 * and every index free: for j = 0, 1, ...: p = the free index with the largest d (ties: the lowest); stop unless d[p] > tol;
 * c = A[:, p] - L[:, :j] L[p, :j]; stop unless c[p] > 0 and finite; c[i] = 0 exactly for i no longer free; L[:, j] = c / sqrt(c[p]);
 * d -= L[:, j]^2; p leaves the free set; piv[j] = p.  Outputs: l (m x m at l + b * stride_l, leading dimension ldl; columns >= rank
 * exactly zero; lower triangular in pivot order, L[piv[i], j] == 0 for i < j; L L^T approximates A with no permutation, every
 * entry within tol in exact arithmetic), piv (nbatch, m) int64 (entries >= rank are -1), rank (nbatch) int64, resid_diag (nbatch)
 * or NULL: the largest remaining d over the free indices (0 when none is left).  tol < 0 means m * eps * max(d_0, 0).  A member
 * whose diagonal holds a non-finite value on entry gets rank = -1 and NaN in l.  A is destroyed.  Work memory comes from the
 * library's block cache; the call returns when the stream has completed.  Two calls give the same bits. */
int gh_dev_pstrf(double* a, int64_t lda, int64_t stride_a, int64_t m, int32_t nbatch, double tol,
                 double* l, int64_t ldl, int64_t stride_l, int64_t* piv, int64_t* rank, double* resid_diag, void* stream);
/* sum_i 2*log(a[i*lda+i]) over the n diagonal entries, accumulated into *out_dev */
int gh_dev_logdet_accum(const double* a, int64_t lda, int64_t n, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* GEORGE_AMD_H_ */
