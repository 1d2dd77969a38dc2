/*
 * mfx.h -- C ABI of libmfx.so: MI355X-native CCD++ / ALS matrix factorization.
 *
 * This is the drop-in boundary for the GPU path of Zialus/CUDA-Recommender: the two
 * solver entry points the reference's driver calls (src/main.cpp:11-17 -> runCUDA ->
 * kernel_wrapper_ccdpp_NV / kernel_wrapper_als_NV, cuda_src/CCD_CUDA.h:49,
 * cuda_src/ALS_CUDA.h:40), restated over plain pointers and sizes so that any host
 * language can bind them.  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - All functions return 0 on success and a negative mfx_status on failure;
 *     mfx_last_error() returns a thread-local human readable message.  Nothing here
 *     calls exit()/abort() or resets the device (the reference's cudaDeviceReset(),
 *     cuda_src/CCD_CUDA.cu:167,177, is deliberately NOT reproduced).
 *   - Caller owns every buffer passed in; the library owns device memory behind handles.
 *   - Indices are 0-based uint32, values fp32 (reference: DTYPE float, src/pmf_util.h:26).
 *   - Factor layouts are the reference's:
 *       CCD++ : W flat [k][rows]  (W[t*rows+i]),  H flat [k][cols]   (cuda_src/CCD_CUDA.cu:255-261)
 *       ALS   : W flat [rows][k]  (W[i*k+c]),     H flat [cols][k]   (cuda_src/ALS_CUDA.cu:229-243)
 *   - There is no CPU fallback: every compute entry point fails with MFX_ERR_NO_DEVICE
 *     when no HIP device is usable.
 */
#ifndef MFX_H
#define MFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI revision: bumped whenever a struct layout or an entry point's argument list changes (2: mfx_params grew the
 * opt-in extension fields and mfx_als_half a `variant` argument; kernel_variant -1).  A binding must compare it
 * with mfx_version() before its first call -- mfx/_lib.py does. */
#define MFX_VERSION 2

typedef enum mfx_status {
    MFX_OK = 0,
    MFX_ERR_INVALID = -1,   /* bad argument / inconsistent sizes */
    MFX_ERR_NO_DEVICE = -2, /* no usable HIP device (never silently falls back to the CPU) */
    MFX_ERR_HIP = -3,       /* a HIP runtime call failed ("CCD FAILED: %s", CCD_CUDA.cu:174) */
    MFX_ERR_COMM = -4,      /* RCCL missing or a collective failed */
    MFX_ERR_ALLOC = -5
} mfx_status;

/* Where the arrays of an mfx_csx / mfx_coo / factor argument live. */
typedef enum mfx_memspace { MFX_HOST = 0, MFX_DEVICE = 1 } mfx_memspace;

/* Dual CSR+CSC rating matrix == the six raw-pointer getters of the reference's
 * SparseMatrix (src/pmf_util.h:83-105).  Both orientations must describe the same
 * matrix; within a row/column the order of entries is the summation order. */
typedef struct mfx_csx {
    int64_t rows, cols, nnz;
    const uint32_t* csc_col_ptr; /* [cols+1] */
    const uint32_t* csc_row_idx; /* [nnz]    */
    const float* csc_val;        /* [nnz]    */
    const uint32_t* csr_row_ptr; /* [rows+1] */
    const uint32_t* csr_col_idx; /* [nnz]    */
    const float* csr_val;        /* [nnz]    */
} mfx_csx;

/* COO test set == reference TestData getters (src/pmf_util.h:196-206).  nnz may be 0. */
typedef struct mfx_coo {
    int64_t nnz;
    const uint32_t* row;
    const uint32_t* col;
    const float* val;
} mfx_coo;

/* The fields of the reference's `parameter` (src/pmf.h:8-43) that the GPU path reads
 * (cuda_src/CCD_CUDA.cu:225-231), plus the knobs this implementation adds. */
typedef struct mfx_params {
    uint32_t k;                /* rank                         (-k, default 10)  */
    float lambda;              /* regularisation               (-l, default 0.1) */
    int32_t maxiter;           /* outer iterations             (-t, default 5)   */
    int32_t maxinneriter;      /* CCD++ inner iterations T     (-T, default 1)   */
    uint32_t nBlocks;          /* accepted and ignored: kernels pick their own geometry */
    uint32_t nThreadsPerBlock; /* accepted and ignored                                   */
    int32_t verbose;           /* 1: print the reference's "[-INFO-] iteration num" line */
    int32_t device;            /* HIP device ordinal (reference hard-codes 0)            */
    int32_t schedule;          /* CCD++ kernel schedule: 0 = as written (separate add-back,
                                  sweeps, subtract launches, one per reference kernel),
                                  1 = fused passes (default; same arithmetic, fewer bytes).
                                  ALS: 0 = as written (explicit Cholesky inverse in the reference's operation
                                  order, bit-identical to src/ALS.cpp), 1 = MFMA Gramian + Cholesky solve */
    int32_t kernel_variant;    /* -1 = REFERENCE-ORDER parity mode (schedule 0 only, single GPU): every rank-one sum is added strictly
                                  left to right in unfused fp32 exactly like src/CCD.cpp:6-16 -- W, H and both residual copies come out
                                  bit-identical to the reference's CPU solver (csrc/ccd_reforder.hip; the CCD++ counterpart of ALS
                                  schedule 0; the subtraction of a rank and the add-back of the next are applied in one pass, same roundings); ~8x slower than the default path;
                                  0 = wave-per-segment kernels (schedule 0 only), 1 = flat-stream kernels (default),
                                  2 = force the scatter layout (csrc/ccd_scatter.hip), which hyper-sparse shapes
                                  get on their own: < 8 entries per (LDS panel, row / column) pair;
                                  3 = the same with explicit 32-bit segment ids in the stream (what a layout
                                  falls back to when some one-byte step between consecutive ids overflows) */
    int32_t profile;           /* 1: bracket every launch with HIP events (mfx_*_kernel_times) */
    int32_t tiles_per_span;    /* flat-stream span length / 256; 0 = choose from nnz */
    int32_t panel_rows;        /* panels of the gathered index space. 0 = choose (LDS panels, 64 KB of LDS per
                                  workgroup, when segments stay long enough; else 2 MB cache panels served by
                                  L2; else none), -1 = off (plain layout, gather from L2 / Infinity Cache),
                                  > 0 = explicit LDS panel of that many entries, < -1 = explicit cache
                                  panel of -panel_rows entries */
    int32_t wg_waves;          /* wavefronts per workgroup of the panel kernel: 4, 8 or 16; 0 = 16 */
    int32_t graph;             /* 0 = replay each outer iteration of the fused schedule as one hipGraph (single
                                  GPU, no per-launch profiling): removes host launch cost when the kernels are
                                  only a few microseconds long; -1 = always launch eagerly */
    int32_t layout_build;      /* where the one-time panel-major layout is built: 0 = on the GPU when the pattern
                                  allows it (inside every segment the entries of one panel are consecutive, e.g.
                                  ascending indices -- what every CSR/CSC converter produces), else on the host;
                                  1 = host builder; 2 = GPU builder or MFX_ERR_INVALID */
    /* ---- opt-in extensions, all 0 by default.  The reference PARSES -N, -e, -p, -q (src/pmf.h:33-36) and reads none
     * of them in its solvers, so a drop-in must ignore them by default too; set these to give them the meaning they
     * have in LIBPMF 1.41's ccd-r1.cpp, of which the reference is a fork (CCD++ only, single GPU for eps / rank_trace).
     * do_nmf and eps are "parity unpinned" (no code or fixture in the reference tree; checked against the oracle's
     * restatement of the published algorithm); rank_trace is the reference's own calrmse_r1 (src/tools.cpp:261-270),
     * whose call site is commented out at src/CCD.cpp:141-148. */
    int32_t do_nmf;            /* -N: new coordinate values are clamped at 0 (non-negative factorisation) */
    float eps;                 /* -e: > 0 enables the function-decrease stopping rule of the inner iterations (and of the
                                  rank loop after five ranks that stop at once); costs one host sync per inner iteration */
    int32_t rank_trace;        /* -p with -q: test RMSE after every rank (mfx_ccd_rank_trace); with verbose also printed
                                  as the reference's commented line "iter %d rank %d time %f rmse %f" */
} mfx_params;

/* One outer iteration's numbers == the fields of the reference's log line
 * (cuda_src/CCD_CUDA.cu:405-406, cuda_src/ALS_CUDA.cu:360-361), in seconds. */
typedef struct mfx_iter_report {
    double rank_time;   /* CCD++: rank-one sweeps (GPU time, HIP events)            */
    double update_time; /* CCD++: residual updates; ALS: the whole iteration        */
    double rmse;        /* test RMSE after this iteration (0 if no test set)        */
    double rmse_time;
} mfx_iter_report;

const char* mfx_last_error(void);
int mfx_version(void);
/* Number of usable HIP devices (0 if none); never fails. */
int mfx_device_count(void);
void mfx_params_default(mfx_params* p); /* reference defaults, src/pmf.h:26-42 */

/* ------------------------------------------------------------------------------------
 * One-shot solvers: exactly what runCUDA() calls (src/main.cpp:11-17).
 * Replaces kernel_wrapper_ccdpp_NV (cuda_src/CCD_CUDA.cu:164-179) / ccdpp_NV (:224-451).
 *   W [k][rows] in: initial factors (initial_col, src/tools.cpp:165-173); out: result.
 *   H [k][cols] in: ignored -- CCD++ starts from H = 0 (CCD_CUDA.cu:287); out: result.
 *   reports: NULL or [maxiter].
 * ---------------------------------------------------------------------------------- */
int mfx_ccdpp_run(const mfx_csx* R, const mfx_coo* T, float* W, float* H, const mfx_params* p,
                  mfx_iter_report* reports);
/* Replaces kernel_wrapper_als_NV (cuda_src/ALS_CUDA.cu:183-198) / als_NV (:200-406).
 *   W [rows][k] in: ignored (overwritten before first read); H [cols][k] in: initial. */
int mfx_als_run(const mfx_csx* R, const mfx_coo* T, float* W, float* H, const mfx_params* p,
                mfx_iter_report* reports);

/* ------------------------------------------------------------------------------------
 * Resident solvers: the same loops split into create / iterate / fetch so that a caller
 * (bench, a service, a multi-GPU driver) can keep R in HBM across calls and time only
 * the iterations.  `space` says whether R, T and the factor pointers are host or device
 * pointers (device pointers must belong to p->device).
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_comm_s* mfx_comm_t;
typedef struct mfx_ccd_s* mfx_ccd_t;
typedef struct mfx_als_s* mfx_als_t;

/* Multi-GPU description of one user-row-block shard.  R passed to
 * mfx_ccd_create is then the LOCAL sub-matrix: rows = this rank's rows, cols = all items,
 * csc_* = the local CSC over local row ids.  NULL means "single GPU". */
typedef struct mfx_shard {
    mfx_comm_t comm;                 /* communicator over all shards                      */
    const uint32_t* global_col_nnz;  /* [cols] |Omega_c| over ALL shards (lambda scaling) */
    int64_t global_test_nnz;         /* Zt over all shards (RMSE denominator)             */
} mfx_shard;

int mfx_ccd_create(mfx_ccd_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p,
                   mfx_memspace space, const mfx_shard* shard);
/* W [k][rows] required; H [k][cols] may be NULL (= zeros, the reference's start). */
int mfx_ccd_set_factors(mfx_ccd_t s, const float* W, const float* H, mfx_memspace space);
/* Runs n_outer more outer iterations (the iteration counter persists, so the first ever
 * iteration skips the add-back exactly like oiter == 1 in src/CCD.cpp:100).  reports:
 * NULL or [n_outer].  with_rmse = 0 skips the per-iteration test RMSE. */
int mfx_ccd_iterate(mfx_ccd_t s, int n_outer, int with_rmse, mfx_iter_report* reports);
int mfx_ccd_get_factors(mfx_ccd_t s, float* W, float* H, mfx_memspace space);
/* Copies the two residual copies out (test hook: R-hat in CSC order and in CSR order). */
int mfx_ccd_get_residual(mfx_ccd_t s, float* csc_val, float* csr_val);
/* Per-kernel GPU time of the last mfx_ccd_iterate call, measured with HIP events on the
 * solver's stream: names[i] / seconds[i] / launches[i] for i < returned count (<= cap). */
int mfx_ccd_kernel_times(mfx_ccd_t s, int cap, const char** names, double* seconds,
                         int64_t* launches);
/* Per-rank trace of the last mfx_ccd_iterate call (mfx_params.rank_trace, and the ranks the eps rule let run):
 * rmse / seconds are [outer iterations of that call][k] (up to cap entries; NaN / 0 for skipped ranks), ranks_done
 * [iters_cap] the number of ranks updated per outer iteration.  Any pointer may be NULL.  Returns the number of
 * outer iterations recorded (0 when no extension was on). */
int mfx_ccd_rank_trace(mfx_ccd_t s, int cap, double* rmse, double* seconds, int iters_cap, int32_t* ranks_done);
/* Turns the per-launch event bracketing (mfx_params.profile) on or off between iterate calls. */
int mfx_ccd_set_profile(mfx_ccd_t s, int on);
/* Layout the solver chose for one residual copy (side 0 = CSC / column segments, 1 = CSR / row
 * segments): out[0] = panels, out[1] = entries per panel (0 = plain layout), out[2] = 2 scatter
 * layout (3: with 32-bit segment ids) / 1 LDS panels / 0 cache panels or plain, out[3] = tiles per span (tile order: segments per block).  For logs,
 * benchmarks and tests. */
int mfx_ccd_layout_info(mfx_ccd_t s, int side, int32_t out[4]);
int mfx_ccd_destroy(mfx_ccd_t s);

int mfx_als_create(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p,
                   mfx_memspace space);
/* Multi-GPU ALS (SURVEY.md 8e "ALS", 8f N4): rank g owns user rows [row_lo,row_hi) for the W-half
 * and item columns [col_lo,col_hi) for the H-half; W and H are replicated and every half ends with
 * ONE grouped exchange in which every rank broadcasts its freshly solved block.  Create itself runs no collective:
 * the other ranks' block boundaries are gathered by the first mfx_als_iterate, i.e. after mfx_comm_agree.  R->rows / R->cols are the GLOBAL sizes;
 * csr_* describe the local rows (row_ptr rebased to 0, GLOBAL column indices), csc_* the local
 * columns (col_ptr rebased to 0, GLOBAL row indices); R->nnz is ignored (each orientation's count
 * is the last entry of its pointer array).  T holds the test ratings of the local rows with GLOBAL
 * indices.  Host pointers only. */
typedef struct mfx_als_shard {
    mfx_comm_t comm;
    int64_t row_lo, row_hi, col_lo, col_hi;
    int64_t global_test_nnz;
} mfx_als_shard;
int mfx_als_create_sharded(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p,
                           const mfx_als_shard* shard);
int mfx_als_set_factors(mfx_als_t s, const float* W, const float* H, mfx_memspace space);
int mfx_als_iterate(mfx_als_t s, int n_iter, int with_rmse, mfx_iter_report* reports);
int mfx_als_get_factors(mfx_als_t s, float* W, float* H, mfx_memspace space);
int mfx_als_kernel_times(mfx_als_t s, int cap, const char** names, double* seconds,
                         int64_t* launches);
int mfx_als_destroy(mfx_als_t s);

/* Implicit-feedback ALS (Hu, Koren, Volinsky 2008) on the ALS factor layout.  R holds interaction strengths r >= 0;
 * every (user, item) pair is in the loss with preference p = (r > 0) and confidence c = 1 + w, w = fp32(alpha * r).
 * A half-sweep solves, for every segment s over the fixed other factor X (all its rows),
 *     (X^T X + lambda I + sum_{j in s} w_j x_j x_j^T) y_s = sum_{j in s, r_j > 0} (1 + w_j) x_j
 * (an empty segment gives y = 0; an explicit zero is no entry).  Returns an mfx_als_t: mfx_als_set_factors / _iterate /
 * _get_factors / _kernel_times / _destroy work on it unchanged (iterate fills update_time, rmse stays 0).  Reads k,
 * lambda, device, profile, verbose of *p; schedule must be 1 (no as-written mode exists for this method).  R: both
 * orientations, values finite and >= 0 with alpha * r finite (checked on the device).  Single GPU.
 * MFX_ERR_INVALID without touching the device: alpha < 0 / NaN / Inf, k outside 1..128, schedule != 1, a null argument. */
int mfx_ials_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, mfx_memspace space);
/* The objective at the current factors, in fp64:
 *     L = sum_{(u,i) in R} [c_ui (p_ui - s_ui)^2 - s_ui^2] + <W^T W, H^T H>_F + lambda (|W|^2 + |H|^2)
 * (= the sum over all rows x cols pairs of c (p - s)^2, plus the regulariser), s_ui the fp32 fused multiply-add chain
 * in ascending t.  MFX_ERR_INVALID on an explicit-ALS handle. */
int mfx_ials_loss(mfx_als_t s, double* loss);
/* Single operator for tests: one implicit half-sweep over host arrays (the counterpart of mfx_als_half):
 * Y [nseg][k] from X [nrows_x][k] and the segments ptr / idx / val. */
int mfx_ials_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                  int64_t nrows_x, const float* X, float* Y, int64_t k, float lambda, float alpha, int device);

/* Implicit ALS by block subspace sweeps ("iALS++", Rendle et al. 2021): the same objective at ranks k up to 1024 (the
 * range mfx_rec_query scores).  The solver keeps the score s_j = <x_j, y> of every stored pair and a half-sweep makes,
 * for every segment from its CURRENT row y (warm start), one pass over the blocks pi_b = [b d, min(k, (b + 1) d)),
 * b = 0, 1, ... of d = `block` coordinates; one step is the exact minimiser of the segment's objective over y_pi:
 *     g = sum_{r_j > 0} (w_j s_j - (1 + w_j)) x_jpi + G[pi, :] y,     A = sum_{r_j > 0} w_j x_jpi x_jpi^T + G[pi, pi],
 *     Delta = A^-1 g,     y_pi <- y_pi - Delta,     s_j <- s_j - <x_jpi, Delta>          (G = X^T X + lambda I)
 * (an empty segment gives y = 0; an explicit zero is no entry).  With a single block (d >= k) a half-sweep solves the
 * system of mfx_ials_half and does not read its start (the residual of a start is formed in fp32, so a start far from the
 * answer would only add its rounding: the rows start from zero); otherwise it is a different method with different
 * iterates, whose loss still falls monotonically.  Cost per stored pair k d instead of k^2.
 * block: 0 = chosen from k as min(k, 64), else 1 <= block <= 128 (values above k act as k).  Returns an mfx_als_t:
 * mfx_als_set_factors / _iterate / _get_factors / _kernel_times / _destroy and mfx_ials_loss work on it.
 * mfx_als_set_factors: H required; W NULL = zeros (W is the warm start of the first W-half -- unlike the exact solvers
 * it IS read).  One iterate step = W-half over H, then H-half over the new W.  Memory on the device besides the matrix
 * and the factors: one float per stored pair, a block-major copy of the larger factor, k^2 floats.  Fold-in
 * for models trained here: mfx_rec_fold_in_block_setup (mfx_rec_fold_in_setup solves k <= 128 only).  Single GPU.
 * MFX_ERR_INVALID without touching the device: k outside 1..1024 ("rank"), block outside 0..128 ("block"), alpha < 0 /
 * NaN / Inf ("alpha"), schedule != 1 ("schedule"), a null argument. */
int mfx_ials_block_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, int32_t block,
                          mfx_memspace space);
/* Single operator for tests: one half-sweep from Y_in [nseg][k] (NULL = zeros) to Y_out [nseg][k], host pointers. */
int mfx_ials_block_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                        int64_t nrows_x, const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block,
                        float lambda, float alpha, int device);

/* Implicit ALS by preconditioned conjugate gradients: the same objective at ranks k up to 1024, every half-sweep solving its
 * systems to a stated tolerance.  A segment's system over the fixed side X is
 *     A y = b,   A = G + sum_{r_j > 0} w_j x_j x_j^T,   b = sum_{r_j > 0} fp32(1 + w_j) x_j,   G = X^T X + lambda I,
 * the fixed base plus a matrix of the rank of the segment, so conjugate gradients preconditioned by Minv ~ G^-1 end, in exact
 * arithmetic, after n + 1 steps on a segment of n entries.  A half-sweep forms G, inverts it on the device (mfx_spd_inverse's
 * kernels) and runs the recurrence of mfx_rec_fold_in_cg_setup on every segment from its CURRENT row (warm start): at most
 * `steps` steps, a row stops once |b - A y| <= tol |b| (2-norms, fp32; tol = 0: every row takes `steps` steps unless its
 * direction vanishes).  An empty segment gives y = 0.  Returns an mfx_als_t: mfx_als_set_factors / _iterate / _get_factors /
 * _kernel_times / _destroy and mfx_ials_loss work on it as on mfx_ials_block_create's.  mfx_als_set_factors: H required;
 * W NULL = the first W-half starts cold (from zero), else W is its warm start.  One iterate step = W-half over H, then
 * H-half over the new W.  A failed inverse (G not positive definite) or failed rows are reported as the other solvers
 * report a failed system; mfx_ials_cg_stats counts them.  Memory on the device besides the matrix and the factors: the four
 * CG vectors, 16 k bytes per row of the larger side, and 5 k^2 floats.  Single GPU.
 * MFX_ERR_INVALID without touching the device: k outside 1..1024 ("rank"), steps < 1 ("steps"), tol < 0 / NaN / Inf
 * ("tol"), alpha < 0 / NaN / Inf ("alpha"), schedule != 1 ("schedule"), a null argument. */
int mfx_ials_cg_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, int32_t steps, float tol,
                       mfx_memspace space);
/* The last iteration of an mfx_ials_cg_create handle (zeros before the first): out[0..3] the W-half, out[4..7] the H-half:
 * the row-steps applied, the most steps any row took, the rows that used all `steps` without meeting tol (0 when
 * tol = 0), the failed rows.  MFX_ERR_INVALID on a handle of another kind. */
int mfx_ials_cg_stats(mfx_als_t s, int64_t out[8]);
/* Single operator for tests: one half-sweep from Y_in [nseg][k] (NULL = cold, from zero) to Y_out [nseg][k], host pointers,
 * by the code of the trainer's half.  counts: [nseg], the steps applied to every row, or NULL. */
int mfx_ials_cg_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                     int64_t nrows_x, const float* X, const float* Y_in, float* Y_out, int64_t k, float lambda, float alpha,
                     int32_t steps, float tol, int32_t* counts, int device);

/* Implicit ALS with an unobserved weight and a frequency-scaled regulariser (Rendle et al. 2021, "Revisiting the Performance
 * of iALS on Item Recommendation Benchmarks": their unobserved_weight and regularization_exp).  alpha0 > 0 weighs the
 * all-pairs term, 0 <= nu <= 1 scales the regulariser of a segment s (a user row or an item column) over the fixed factor X
 * with N rows by its n_s stored entries with r > 0:
 *     f_s(y) = sum_{r_j > 0} [(alpha0 + w_j)(1 - s_j)^2 - alpha0 s_j^2] + alpha0 y^T X^T X y + rho_s |y|^2,   w_j = fp32(alpha r_j)
 *     rho_s  = fp32((double) lambda * pow((double) n_s + (double) alpha0 * (double) N, (double) nu))
 * A half-sweep solves (G_s + sum_j w_j x_j x_j^T) y = sum_{r_j > 0} (alpha0 + w_j) x_j with G_s = G0 + rho_s I, one fp32 add
 * on the diagonal of G0 = fp32(alpha0 X^T X) (X^T X summed as for mfx_ials_create).  An empty segment, and one whose entries
 * are all explicit zeros, gives y = 0.  nu = 0: rho_s = lambda; at alpha0 = 1, nu = 0 mfx_ials_create_reg and mfx_ials_half_reg
 * equal mfx_ials_create and mfx_ials_half bit for bit.  The block step of mfx_ials_block_create_reg is
 *     A z = sum_{r_j > 0} ((alpha0 + w_j) - w_j s_j) x_jpi - P_s,   A = G_s[pi, pi] + sum_j w_j x_jpi x_jpi^T,
 *     P_s[c] = fmaf(rho_s, y[b0 + c], (Y G0[:, pi])[s][c])
 * with pi, d, z and s_j as for mfx_ials_block_create.  The handles are mfx_als_t as those of the un-suffixed functions:
 * mfx_als_set_factors / _iterate / _get_factors / _kernel_times / _destroy work on them, and mfx_ials_loss returns
 *     L = sum_{r > 0} [(alpha0 + w)(1 - s)^2 - alpha0 s^2] + alpha0 <W^T W, H^T H>_F + sum_u rho_u |w_u|^2 + sum_i rho_i |h_i|^2
 * (rho_u over N = cols, rho_i over N = rows).  MFX_ERR_INVALID without touching the device: alpha0 <= 0 / NaN / Inf
 * ("alpha0"), nu outside [0, 1] or NaN ("nu"), fp32(lambda ((1 + alpha0) max(rows, cols))^nu) not finite ("regulariser";
 * the half operators take rows = nseg, cols = nrows_x), and everything the un-suffixed function refuses. */
int mfx_ials_create_reg(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, float alpha0, float nu, mfx_memspace space);
int mfx_ials_block_create_reg(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, float alpha0, float nu, int32_t block,
                              mfx_memspace space);
int mfx_ials_half_reg(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x, const float* X,
                      float* Y, int64_t k, float lambda, float alpha, float alpha0, float nu, int device);
int mfx_ials_block_half_reg(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x,
                            const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block, float lambda, float alpha,
                            float alpha0, float nu, int device);

/* Explicit ALS by block subspace sweeps: the objective of mfx_als_create at ranks k up to 1024 (the range mfx_rec_query
 * scores), by the sweeps of mfx_ials_block_create.  For one segment (a user row or an item column), X the fixed other
 * factor and r_j the segment's stored values, the objective is
 *     f(y) = sum_j (r_j - <x_j, y>)^2 + rho |y|^2
 * with rho = lambda (reg 0: the reference's ALS, src/ALS.cpp) or rho = fp32(lambda * n), n the number of stored entries of
 * the segment (reg 1: the CCD++ objective, the one MFX_FOLD_CCD minimises at k <= 128).  The solver keeps the score
 * s_j = <x_j, y> of every stored pair and a half-sweep makes, for every segment from its CURRENT row y, one pass over the
 * blocks pi_b = [b d, min(k, (b + 1) d)), b = 0, 1, ... of d = `block` coordinates; one step is
 *     A = sum_j x_jpi x_jpi^T + rho I,     A z = sum_j (r_j - s_j) x_jpi - rho y_pi,     y_pi += z,     s_j += <x_jpi, z>
 * Every stored entry counts, explicit zeros and negative values included (the "r > 0" rule of the implicit code does not
 * apply); an empty segment gives y = 0 (src/ALS.cpp:151-157).  With a single block (d >= k) a step from any start is the
 * exact minimiser: it solves the system of mfx_als_half, and the start is not read (as in mfx_ials_block_create, the rows
 * start from zero).  With more than one block this is a different method with
 * different iterates -- a sweep is not a solve -- whose training objective never increases.  Cost per stored pair k d
 * instead of k^2.  No float atomics, every sum has a fixed order: results are bitwise reproducible.
 * block: 0 = chosen from k as min(k, 64), else 1 <= block <= 128 (values above k act as k).  reg: 0 or 1.  T: the test set
 * of mfx_als_create (or NULL); iterate reports the test RMSE as the exact solver does.  Returns an mfx_als_t:
 * mfx_als_set_factors / _iterate / _get_factors / _kernel_times / _destroy work on it.  mfx_als_set_factors: H required;
 * W NULL = zeros (W is the warm start of the first W-half: it IS read).  One iterate step = W-half over H, then H-half
 * over the new W; kernel-time names alsb_half_rows(W over H), alsb_half_cols(H over W).  Reads k, lambda, device, verbose
 * of *p; schedule must be 1.  R: both orientations, values finite (checked on the device).  Single GPU.  Memory on the
 * device besides the matrix and the factors: one float per stored pair and a block-major copy of the larger factor.
 * Fold-in for models of rank above 128: mfx_rec_fold_in_block_setup_als.  mfx_als_create and mfx_als_half keep k <= 128.
 * MFX_ERR_INVALID without touching the device: k outside 1..1024 ("rank"), block outside 0..128 ("block"), reg not 0 / 1
 * ("reg"), lambda <= 0 / NaN / Inf ("lambda"), schedule != 1 ("schedule"), a null argument. */
int mfx_als_block_create(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, int32_t block, int32_t reg,
                         mfx_memspace space);
/* Single operator for tests: one half-sweep from Y_in [nseg][k] (NULL = zeros) to Y_out [nseg][k], host pointers. */
int mfx_als_block_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                       int64_t nrows_x, const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block,
                       float lambda, int32_t reg, int device);

/* ------------------------------------------------------------------------------------
 * BPR training (Bayesian Personalised Ranking, Rendle et al. 2009) by deterministic mini-batch steps: the trainer that
 * optimises the ranking itself.  Every bit of the factors is fixed by (data, seed, parameters, batch): the sums of a
 * step are exact integer sums, so neither the order of the slots nor the launch geometry plays a part.
 *
 * Data.  Every stored entry of the CSR side of R is a positive interaction; values and the CSC side are not read.  The
 * ids of every row must be strictly ascending and below cols, the pointers ascend from 0 to nnz (mfx/dataset.from_coo
 * produces this); checked on the device at create, a violation is MFX_ERR_INVALID naming the first such row.  Factors in
 * the ALS layout, W [rows][k] and H [cols][k], 1 <= k <= 1024; rows, cols, nnz < 2^32 - 1.
 *
 * One step takes n <= batch slots; slot t holds (u, i, j) = (user, positive item, sampled item) and is SKIPPED when j is
 * in row u.  Every slot reads the factors as they were before the step.  For a slot that is not skipped:
 *   d_c = fp32(H[i][c] - H[j][c]);
 *   x   = the fp32 FMA chain acc = fmaf(W[u][c], d_c, acc) over c = 0 .. k-1 from +0 (the chain of mfx_rec_score);
 *   g   = 1 / (1 + e^x) by this sequence of single fp32 operations (round to nearest even, no contraction):
 *           xc = min(max(x, -80), 80);  n = rint(xc * 0x3FB8AA3B [1.44269502]);
 *           r  = (xc - n * 0.693359375) - n * 0xB95E8083 [-2.12194442e-4];
 *           p  = c6; p = p * r + c5; ... p = p * r + c0 (a multiply, then an add), c6 .. c0 = fp32 of 1/720, 1/120,
 *                1/24, 1/6, 1/2, 1, 1 [0x3AB60B61, 0x3C088889, 0x3D2AAAAB, 0x3E2AAAAB, 0.5, 1, 1];
 *           e  = ldexp(p, n) (exact);  g = 1 / (1 + e), the division correctly rounded.
 *         Relative error against fp64 on |x| <= 30: 2.8e-7.  Saturation: g = 1 for x <= -16.64, g = 0x05BFECBB [1.80e-35]
 *         for x >= 80; never NaN for finite x.
 *   terms: fp32(g * d_c) for row u of W, fp32(g * W[u][c]) for row i of H and its exact negative for row j of H.
 * The slot is BAD when x is not finite or a term has magnitude >= 64; a bad slot contributes nothing and is counted.
 * (batch <= 2^20 slots give a row of H at most 2^21 terms: the sums stay below 2^27, the limit of csrc/ccd_scatter.hip.)
 * Sums.  Every term is truncated toward zero to a multiple of 2^-36 and the terms of a row are added exactly, as 64-bit
 * integers; a_c = the fp32 nearest to the sum (one rounding, int64 -> fp32, ties to even, then the exact scale).
 * Update of every row touched by at least one counted slot (neither skipped nor bad), m = the number of such slots of
 * the row (for an item: as positive plus as sampled), lambda = p->lambda:
 *   new = fp32(old + fp32(lr * fp32(a_c - fp32(fp32(lambda * fp32(m)) * old))));
 * untouched rows keep their bits.  With batch = 1 this is classical BPR-SGD; a batch is the sum of its slots' steps at
 * frozen parameters, so lr times the most occurrences of one row in a batch should stay modest: that is the caller's
 * choice of batch.  Counts of a call: slots, skipped, bad, correct (x > 0 among the counted).
 *
 * The sampler is a stateless function of (seed, slot number n = 0, 1, 2, ... over the solver's life).  With
 *   fin(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)
 *   G = 0x9E3779B97F4A7C15, s0 = fin(seed + G), out(c) = fin(s0 + (c + 1) * G)           (all modulo 2^64):
 *   p = out(2n) mod nnz, j = out(2n + 1) mod cols, u = the row with csr_row_ptr[u] <= p < csr_row_ptr[u + 1],
 *   i = csr_col_idx[p]; skipped when j is in row u.
 * An epoch is nnz slots cut into steps of `batch`; the last step of an epoch is shorter when batch does not divide nnz.
 *
 * mfx_bpr_create reads k, lambda, device and profile of *p.  MFX_ERR_INVALID without touching the device: k outside
 * 1..1024, batch outside 1..2^20, lr or lambda negative or not finite, nnz = 0, cols < 2, a null argument.  Memory on the
 * device: the factors, 8 bytes beside every factor element (the accumulators), 8 bytes per row and column, the CSR
 * pointers and ids, 18 bytes per slot of a step.  After create no step's cost grows with rows + cols (this does not hold
 * for mfx_lgcn_* below, which propagates the whole graph every step: nnz * k * layers by construction).
 * mfx_bpr_set_factors copies W and H (both required); stepping or mfx_bpr_get_factors before it is MFX_ERR_INVALID and
 * leaves the handle usable.  mfx_bpr_steps runs n_steps steps from the current slot; mfx_bpr_epochs runs n_epochs
 * epochs, the first of them being the remaining steps of a started epoch; stats [4] (per epoch: [n_epochs][4]) = slots,
 * skipped, bad, correct of the call (the epoch), seconds (per epoch: [n_epochs]) its stream time; either may be NULL.
 * mfx_bpr_position: the number of the next slot.  mfx_bpr_kernel_times: stream seconds since create of the sampler, the
 * gradient kernel, the scatter of the terms and the apply, collected only when p->profile != 0 (it synchronises every step).
 * mfx_bpr_triples is the sampler on the host (no device is touched): the slots first_slot .. first_slot + count - 1 of
 * `seed` over the host matrix R; skipped [count] holds 0 / 1.
 * mfx_bpr_apply is the single operator: one step on the caller's n <= 2^20 triples and host factors, in place.  It has no
 * matrix: a slot is skipped only where skipped[t] != 0 (skipped = NULL: none); ids are checked on the device
 * (MFX_ERR_INVALID naming the first slot with u >= rows or an item >= cols; W and H are left as they were).  i == j is
 * allowed: the row is touched twice by that slot, m counts both, the terms cancel.  The solver's step is the sampler
 * followed by exactly this code path.
 *
 * Negative sampling by trials (mfx_bpr_create_neg, mfx_bpr_apply_neg).  A slot gets M = `negatives` trial items, 1 <= M <=
 * 1024, scored at the factors of before the step, and a mode picks one of them as j.  Every bit is fixed by (data, seed,
 * parameters, batch, M, mode).  Modes: MFX_BPR_NEG_UNIFORM = 0 requires M = 1 and is mfx_bpr_create; MFX_BPR_NEG_HARDEST = 1
 * (hardest of M, dynamic negative sampling, Zhang et al. 2013); MFX_BPR_NEG_WARP = 2 (Weston et al. 2011).
 * Trials of slot n: they depend neither on the mode nor on M, so the trials of M are the first M of those of M + 1.
 *   (u, i) as above; trial 1 is the sampled item above, c_1 = out(2n + 1) mod cols;
 *   trial t >= 2: c_t = fin(b_n + t * G) mod cols with b_n = fin(s1 + (n + 1) * G), s1 = fin(seed + 2 * G)  (modulo 2^64);
 *   member_t = 1 when c_t is in row u.
 * Scores: s_i = the fp32 FMA chain acc = fmaf(W[u][c], H[i][c], acc) over c = 0 .. k-1 from +0 (the chain of
 * mfx_rec_score), s_t the same chain with H[c_t]; one lane owns a chain, no sum crosses lanes.
 * HARDEST.  Eligible are the trials with member_t = 0; with none the slot is skipped.  Otherwise j = c_t of the eligible
 * trial that comes first in this order: a NaN score ranks below every number; then the greater score; then the smaller t
 * (+0 and -0, and equal infinities, are ties).  The slot (u, i, j) then takes the step above unchanged (d-chain, sigmoid,
 * bad rule, counts), so M = 1 is mfx_bpr_create bit for bit.
 * WARP.  If s_i is not finite the slot is bad.  Otherwise t = 1 .. M in order, members passed over: the first trial with
 * !(fp32(s_i - s_t) >= 1) (one fp32 subtraction, so a NaN s_t violates) is the violator, j = c_t and g = rank_weight[t - 1].
 * Without a violator the slot is skipped.  It is bad if the violator's s_t is not finite, or unless every term satisfies
 * |fp32(g * d_c)| < 64 and |fp32(g * W[u][c])| < 64 with d_c = fp32(H[i][c] - H[j][c]) (a NaN is not below 64).  Terms,
 * fixed point, counts, claim and update are those above with g in place of the sigmoid; a weight of 0 still counts the
 * slot, so its regularisation applies.  `correct` counts the counted slots with fp32(s_i - s_t) > 0.
 * Rank weights: rank_weight [M], fp32, each finite and >= 0 (else MFX_ERR_INVALID), read in WARP only.  NULL selects
 * mfx_bpr_rank_weights(cols, M, out): out[t - 1] = (float) log((double) max(1, (cols - 1) / t)), an integer division
 * (LightFM's weight: the draws needed estimate the rank of the positive item); filled on the host.
 * mfx_bpr_create_neg: mfx_bpr_create with a mode; its handle works with every mfx_bpr_* call.  Its refusals and, also
 * without touching the device: a mode out of range, M outside 1 .. 1024, UNIFORM with M != 1, a bad table.  The trial items
 * are not stored: 4 more bytes per slot of a step.  mfx_bpr_kernel_times counts the trials kernel under the sampler; in
 * WARP the gradient kernel does not run.
 * mfx_bpr_trials is the trial sampler on the host (no device is touched): items and member [count][M] of the slots
 * first_slot .. first_slot + count - 1, u and i [count] as mfx_bpr_triples gives them.  mfx_bpr_rank_weights: host only;
 * cols >= 1.
 * mfx_bpr_apply_neg is the single operator on the caller's trials: items [n][M], member [n][M] (NULL: none; it computes no
 * membership itself), n <= 2^20, host factors in place; ids are checked on the device as mfx_bpr_apply does (the first
 * slot with u >= rows, i >= cols or a trial item >= cols is named).  UNIFORM is refused here.  j_out [n] (the chosen item,
 * undefined where none was chosen) and t_out [n] (the chosen trial, 0 = none) may be NULL.  The solver's step at M > 1 or in
 * WARP is the two samplers followed by exactly this code path.
 * mfx_bpr_trial_stats, since create: out[0] = the slots that ended without a chosen trial (HARDEST: no eligible trial;
 * WARP: no violator, or s_i not finite; UNIFORM: skipped), out[1] = the sum of the chosen trial numbers t.
 * ---------------------------------------------------------------------------------- */
#define MFX_BPR_NEG_UNIFORM 0
#define MFX_BPR_NEG_HARDEST 1
#define MFX_BPR_NEG_WARP 2
typedef struct mfx_bpr_s* mfx_bpr_t;
int mfx_bpr_create(mfx_bpr_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed,
                   mfx_memspace space);
int mfx_bpr_set_factors(mfx_bpr_t s, const float* W, const float* H, mfx_memspace space);
int mfx_bpr_get_factors(mfx_bpr_t s, float* W, float* H, mfx_memspace space);
int mfx_bpr_steps(mfx_bpr_t s, int64_t n_steps, int64_t stats[4], double* seconds);
int mfx_bpr_epochs(mfx_bpr_t s, int32_t n_epochs, int64_t* stats /* [n_epochs][4] */, double* seconds /* [n_epochs] */);
int mfx_bpr_position(mfx_bpr_t s, int64_t* next_slot);
int mfx_bpr_kernel_times(mfx_bpr_t s, double seconds[4]);
int mfx_bpr_destroy(mfx_bpr_t s);
int mfx_bpr_triples(uint64_t seed, int64_t first_slot, int64_t count, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* j,
                    uint8_t* skipped);
int mfx_bpr_apply(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i,
                  const uint32_t* j, const uint8_t* skipped /* may be NULL */, float lr, float lambda, int64_t stats[4],
                  int device);
int mfx_bpr_create_neg(mfx_bpr_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed,
                       int32_t mode, int64_t negatives, const float* rank_weight /* [negatives] or NULL */, mfx_memspace space);
int mfx_bpr_trials(uint64_t seed, int64_t first_slot, int64_t count, int64_t negatives, const mfx_csx* R, uint32_t* u,
                   uint32_t* i, uint32_t* items /* [count][negatives] */, uint8_t* member /* [count][negatives] */);
int mfx_bpr_rank_weights(int64_t cols, int64_t negatives, float* out /* [negatives] */);
int mfx_bpr_apply_neg(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i,
                      int64_t negatives, const uint32_t* items /* [n][negatives] */, const uint8_t* member /* or NULL: none */,
                      int32_t mode, const float* rank_weight /* WARP: NULL = default */, float lr, float lambda,
                      int64_t stats[4], uint32_t* j_out /* [n] or NULL */, uint32_t* t_out /* [n] or NULL, 0 = none chosen */,
                      int device);
int mfx_bpr_trial_stats(mfx_bpr_t s, int64_t out[2]);

/* ------------------------------------------------------------------------------------
 * LightGCN (He et al., SIGIR 2020): BPR training on graph-propagated embeddings.  The user and item vectors that enter
 * the pairwise loss are the mean of the base embeddings and their L propagated copies under the symmetrically normalised
 * interaction graph; sampler, score chain, sigmoid, bad rule, fixed-point sums and counts are those of "BPR training"
 * above.  Every bit of the base embeddings is fixed by (data, seed, parameters, batch, layers): no bit depends on launch
 * geometry, lanes per row, tile width or batch of loads.
 *
 * Data.  Only the pattern of R is read, BOTH sides: the CSR side gives a user's items, the CSC side an item's users; values
 * are ignored.  Each side must satisfy the row rules of BPR (pointers from 0 to nnz, ids strictly ascending and in range),
 * and the CSC side must be the transpose pattern of the CSR side; all three are checked on the device at create
 * (MFX_ERR_INVALID naming the first row or column).  d_x = the degree of a user or item, s_x = fp32(1 / sqrt((double) d_x)),
 * s_x = 0 where d_x = 0; L = `layers`, 0 <= L <= 8; c_L = fp32(1 / fp32(L + 1)), one correctly rounded division.
 *
 * One propagation half-pass produces the rows of one side from the rows X of the other side.  Destination row r has the
 * entries e_0 .. e_{n-1} in stored order (CSR order for a user, CSC order for an item).  For coordinate c:
 *   the entries are cut into segments of 1024 consecutive entries;
 *   a segment's sum is the fp32 FMA chain acc = fmaf(s[src_e], X[src_e][c], acc) over its entries from +0;
 *   the segment sums are added left to right in fp32, starting from the first segment's sum;
 *   the result is fp32(s_r * total).
 * A row of at most 1024 entries is one chain, an empty row gives +0.  The constant 1024 is part of the contract.
 * Layers.  E^0 = (W0, H0), the base embeddings.  E^{l+1}: its user rows by a half-pass from the item rows of E^l, its item
 * rows by a half-pass from the user rows of E^l.  The final embeddings are fp32(c_L * (((E^0 + E^1) + ...) + E^L)), the sum
 * left to right in fp32; for L = 0 they are the base embeddings bit for bit.
 *
 * One step on n <= batch slots (u, i, j, skipped):
 *   1. (W, H) = the final embeddings of the current base;
 *   2. the step of "BPR training" on (W, H) up to its sums: g, the states and counts, the 2^-36 fixed-point sums a row, m_r
 *      = the counted slots of row r;
 *   3. G[r][c] = the fp32 nearest to the sum (one rounding, int64 -> fp32, then the exact scale) for the rows with
 *      m_r > 0, +0 elsewhere;
 *   4. D = the propagation and mean of step 1 applied to G (G's own layers, the same c_L): the normalised adjacency is
 *      symmetric, so this is the gradient with respect to the base;
 *   5. every row r with m_r > 0, or with L >= 1 and d_r > 0:
 *        new = fp32(old + fp32(lr * fp32(D[r][c] - fp32(fp32(lambda * fp32(m_r)) * old))));  other rows keep their bits.
 * With L = 0 this is the step of mfx_bpr_apply bit for bit.  Every step propagates the whole graph twice: its cost grows
 * with nnz * k * L, unlike a BPR step.
 *
 * mfx_lgcn_create reads k, lambda, device and profile of *p.  MFX_ERR_INVALID without touching the device: k outside
 * 1..1024, batch outside 1..2^20, layers outside 0..8, lr or lambda negative or not finite, nnz = 0, cols < 2, a null
 * argument or side.  Memory on the device: 32 bytes per element of the embeddings (base, final, accumulators, G, D and up
 * to two layers), both sides of the pattern, 20 bytes per row and column, 16 bytes per work item (a row or a 1024-entry
 * segment), 4 k bytes per segment of the rows above 1024 entries, 18 bytes per slot.
 * mfx_lgcn_set_base copies the base embeddings W0 [rows][k], H0 [cols][k] (both required); stepping or reading before it
 * is MFX_ERR_INVALID and leaves the handle usable.  mfx_lgcn_get_base returns the base, mfx_lgcn_get_factors the final
 * embeddings of the current base (a forward pass), which serve mfx_rec_* as any (W, H).  mfx_lgcn_steps, _epochs and
 * _position are those of mfx_bpr_*.  mfx_lgcn_kernel_times: stream seconds since create of the sampler, the forward pass,
 * the gradient kernel, the scatter, the backward pass (with the collection of G) and the update, p->profile != 0 only.
 * mfx_lgcn_propagate is the single operator of step 1 on host arrays: (W, H) from (W0, H0) over the host matrix R.
 * mfx_lgcn_apply is the single operator of one step: the caller's n <= 2^20 triples, host base embeddings in place, a slot
 * skipped only where skipped[t] != 0 (NULL: none), ids checked as mfx_bpr_apply does.  The solver's step is the sampler
 * (mfx_bpr_triples) followed by exactly this code path.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_lgcn_s* mfx_lgcn_t;
int mfx_lgcn_create(mfx_lgcn_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, int32_t layers,
                    uint64_t seed, mfx_memspace space);
int mfx_lgcn_set_base(mfx_lgcn_t s, const float* W0, const float* H0, mfx_memspace space);
int mfx_lgcn_get_base(mfx_lgcn_t s, float* W0, float* H0, mfx_memspace space);
int mfx_lgcn_get_factors(mfx_lgcn_t s, float* W, float* H, mfx_memspace space);
int mfx_lgcn_steps(mfx_lgcn_t s, int64_t n_steps, int64_t stats[4], double* seconds);
int mfx_lgcn_epochs(mfx_lgcn_t s, int32_t n_epochs, int64_t* stats /* [n_epochs][4] */, double* seconds /* [n_epochs] */);
int mfx_lgcn_position(mfx_lgcn_t s, int64_t* next_slot);
int mfx_lgcn_kernel_times(mfx_lgcn_t s, double seconds[6]);
int mfx_lgcn_destroy(mfx_lgcn_t s);
int mfx_lgcn_propagate(const mfx_csx* R, const float* W0, const float* H0, int64_t k, int32_t layers, float* W, float* H,
                       int device);
int mfx_lgcn_apply(const mfx_csx* R, int64_t k, float* W0, float* H0, int64_t n, const uint32_t* u, const uint32_t* i,
                   const uint32_t* j, const uint8_t* skipped /* may be NULL */, int32_t layers, float lr, float lambda,
                   int64_t stats[4], int device);

/* ------------------------------------------------------------------------------------
 * Hybrid BPR: BPR training on rows whose vectors are the weighted sums of the embeddings of their features (the model of
 * LightFM, Kula 2015, without biases).  A row that has no interaction still has a vector, so an item that was never rated
 * can be scored: the cold start.  Sampler, score chain, sigmoid, bad rule, fixed-point sums and counts are those of "BPR
 * training" above.  Every bit of the embedding tables is fixed by (data, features, seed, parameters, batch): no bit
 * depends on lanes per row, launch geometry, batch of loads or order of arrival.
 *
 * Data.  R is read as in "BPR training": the CSR side, values ignored.  Two feature matrices in CSR with values, Fu
 * [rows] x nfu and Fi [cols] x nfi (mfx_features: n rows, nf features, ptr [n + 1], idx and val [ptr[n]]), and two
 * embedding tables Eu [nfu][k], Ei [nfi][k], 1 <= k <= 1024.  Rules of a feature matrix: the pointers run from 0 to the
 * number of entries, the ids are strictly ascending inside a row and below nf, every value is finite with |v| <= 1, a row
 * holds at most 1024 entries; empty rows are allowed.  All of it is checked on the device at create (MFX_ERR_INVALID
 * naming the first offending row).  A NULL feature matrix is the identity (nf = n, the entry (r, 1) in row r); it gives the
 * bits of the identity passed explicitly.
 * The embedding of row r, coordinate c, with the entries (f_0, v_0) .. (f_{n-1}, v_{n-1}) in stored order:
 *   acc = fp32(v_0 * E[f_0][c]);  acc = fmaf(v_e, E[f_e][c], acc) for e = 1 .. n-1;  an empty row gives +0.
 * The chain starts from the first product and not from +0, so a row of the identity returns E's bits, -0 included.
 *
 * One step on n <= batch slots (u, i, j, skipped):
 *   1. W[u], H[i], H[j] = the embeddings of the slots' rows at the tables of before the step;
 *   2. the step of "BPR training" on those rows up to its sums, unchanged: g, the states, the bad rule, the counts, the
 *      2^-36 fixed-point sums of a row and m_r = the counted slots of row r;
 *   3. for every row with m_r > 0: G[r][c] = the fp32 nearest to the row's sum (one rounding int64 -> fp32, then the exact
 *      scale), as in step 3 of "LightGCN";
 *   4. for every such row and every entry (f, v) of it: the term fp32(v * G[r][c]), truncated toward zero to a multiple of
 *      2^-36, is added exactly (64-bit integers) into the accumulator of feature f, and m_r is added to m_f;
 *   5. every feature with m_f > 0: a_c = the fp32 nearest to its sum, and
 *        new = fp32(old + fp32(lr * fp32(a_c - fp32(fp32(lambda * fp32(m_f)) * old))));  other features keep their bits.
 * Limits.  |term| <= |G| < 64 m_r, so the conversion of a term is valid up to 2^27 (not only below 64 as for the terms of a
 * slot).  With |v| <= 1 the sum of a feature is at most 64 times the sum of m_r over the rows that carry it, at most
 * 64 * 2^21 = 2^27: the limit of a row in "BPR training", so no new bad rule is needed.
 * With the identity on both sides the step is that of mfx_bpr_apply bit for bit: G is a multiple of 2^-36, so fp32(1 * G)
 * = G truncates to itself, the feature's sum is the row's sum rounded once, rounding it again returns G, and m_f = m_r.
 * As in BPR a batch is the sum of its slots' steps at frozen parameters: lr * lambda * m_f of a feature that every row
 * carries grows with the batch and can be large; choose lr and lambda for the batch.
 *
 * mfx_hyb_create reads k, lambda, device and profile of *p; Fu and Fi live in `space` as R does.  MFX_ERR_INVALID without
 * touching the device: what mfx_bpr_create refuses, a feature matrix whose n is not rows (cols), nf = 0 or nf >= 2^32 - 1,
 * a NULL ptr.  Memory on the device: what mfx_bpr_create takes (its factors are scratch for the embedded rows), the
 * feature matrices (12 bytes per row of an identity), and per feature 12 k + 8 bytes (the table, its accumulators, count
 * and claim).  After create no step's cost grows with rows + cols or with nfu + nfi: only the rows of the slots are
 * embedded and only their features are updated.
 * mfx_hyb_set_embeddings copies Eu and Ei (both required); stepping or reading before it is MFX_ERR_INVALID and leaves the
 * handle usable.  mfx_hyb_get_embeddings returns the tables (either may be NULL), mfx_hyb_get_factors the embeddings of
 * all rows W [rows][k], H [cols][k] (a NULL side is not computed), which serve mfx_rec_* as any (W, H).  mfx_hyb_steps, _epochs and _position are those of
 * mfx_bpr_*; only uniform negatives.  mfx_hyb_kernel_times: stream seconds since create of the sampler, the embedding, the
 * gradient kernel, the scatter, the spread to the features and the apply, p->profile != 0 only.
 * mfx_hyb_embed is the single operator of the embedding on host arrays: out [F->n][k] from E [F->nf][k], any number of
 * rows.  It is also the cold start: the rows of items that were not in R, which the caller appends to H.
 * mfx_hyb_apply is the single operator of one step: the caller's n <= 2^20 triples, host feature matrices (NULL: the
 * identity) and host tables in place, a slot skipped only where skipped[t] != 0 (NULL: none), ids checked as mfx_bpr_apply
 * does (the tables are left as they were).  The solver's step is the sampler (mfx_bpr_triples) followed by exactly this
 * code path.
 * Left out: biases, trials (hardest of M and WARP would need the trial items embedded first), AdaGrad, several GPUs.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_features {
    int64_t n, nf;       /* rows, features */
    const uint32_t* ptr; /* [n + 1] */
    const uint32_t* idx; /* [ptr[n]] */
    const float* val;    /* [ptr[n]] */
} mfx_features;
typedef struct mfx_hyb_s* mfx_hyb_t;
int mfx_hyb_create(mfx_hyb_t* out, const mfx_csx* R, const mfx_features* Fu /* or NULL */, const mfx_features* Fi /* or NULL */,
                   const mfx_params* p, float lr, int64_t batch, uint64_t seed, mfx_memspace space);
int mfx_hyb_set_embeddings(mfx_hyb_t s, const float* Eu, const float* Ei, mfx_memspace space);
int mfx_hyb_get_embeddings(mfx_hyb_t s, float* Eu, float* Ei, mfx_memspace space);
int mfx_hyb_get_factors(mfx_hyb_t s, float* W, float* H, mfx_memspace space);
int mfx_hyb_steps(mfx_hyb_t s, int64_t n_steps, int64_t stats[4], double* seconds);
int mfx_hyb_epochs(mfx_hyb_t s, int32_t n_epochs, int64_t* stats /* [n_epochs][4] */, double* seconds /* [n_epochs] */);
int mfx_hyb_position(mfx_hyb_t s, int64_t* next_slot);
int mfx_hyb_kernel_times(mfx_hyb_t s, double seconds[6]);
int mfx_hyb_destroy(mfx_hyb_t s);
int mfx_hyb_embed(const mfx_features* F, const float* E, int64_t k, float* out, int device);
int mfx_hyb_apply(int64_t rows, int64_t cols, int64_t k, const mfx_features* Fu /* or NULL */, const mfx_features* Fi /* or NULL */,
                  float* Eu, float* Ei, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
                  const uint8_t* skipped /* may be NULL */, float lr, float lambda, int64_t stats[4], int device);

/* ------------------------------------------------------------------------------------
 * Item-kNN: the neighbourhood model on the interaction matrix itself (Sarwar et al. 2001; cosine, TF-IDF and BM25
 * weightings as in the usual libraries).  Every bit of the lists and of the scores is fixed by the data: the sums are
 * exact integer sums, so no order of summation, batch or tile width plays a part.
 *
 * Input.  X holds BOTH orientations of the same rows x cols matrix (users x items).  Its values are taken as given: any
 * weighting is the caller's (mfx.knn_weights in Python).  Every CSR row must hold strictly ascending ids below cols and
 * every CSC column strictly ascending ids below rows, the pointers ascending from 0 to nnz (mfx/dataset.from_coo produces
 * this); checked on the device at build, a violation is MFX_ERR_INVALID naming the first such row (column).  That the two
 * sides hold the same entries is not checked.  rows, cols, nnz < 2^32 - 1.
 *
 * Similarity.  For items i != j the term of a user u that holds both is one unfused fp32 multiply t = fp32(x_ui * x_uj).
 * The term is truncated toward zero to a multiple of 2^-36 (the conversion of csrc/ccd_scatter.hip), the terms of a pair
 * are added as 64-bit integers, and s_ij = the fp32 nearest to the sum (one rounding int64 -> fp32, ties to even, then the
 * exact scale).  Hence s_ij and s_ji have the same bits.
 * Neighbours of i: the items j != i whose integer sum is not 0, ordered by similarity descending, then item ascending;
 * the first K are kept, 1 <= K <= 1024.  Unused slots hold item 0xFFFFFFFF and similarity -INFINITY, at the tail only.
 * Storage: nbr_idx [cols][K] and nbr_sim [cols][K].
 * Limits.  A term that is not finite or of magnitude >= 64, or a column of more than 2^21 entries, makes the build fail
 * with MFX_ERR_INVALID naming the smallest such item (for a term: the smaller item i of a pair that has one is named by
 * its own list).  Under these limits no sum reaches 2^27.
 *
 * Recommendation for users given by CSR rows of (item i, value x), the form of mfx_rec_fold_in: new users and training
 * users are the same call.  For every entry and every stored neighbour slot (j, s_ij) of i that is not a pad the term is
 * fp32(x * s_ij), put on the same 2^-36 grid and added as a 64-bit integer (modulo 2^64) into the accumulator of j; the
 * score of j is the fp32 of its sum.  Eligible: the items j whose integer sum is not 0 and that are not in the row; with
 * MFX_KNN_KEEP_SEEN the row's own items stay in.  Order and padding are those of mfx_rec_query, 1 <= n_top <= 1024.
 * A row is BAD if it has a term that is not finite or of magnitude >= 64, or more than 2^21 entries: it returns all pads
 * and is counted in *bad_rows (host memory, may be NULL); the other rows of the batch are unaffected.  The rows' pointers
 * must ascend from 0 to nnz and their ids be strictly ascending and below cols: checked on the device, MFX_ERR_INVALID
 * naming the first such row.  Every row's result is independent of the batch and of the tile width.
 *
 * tile_items: 0 = automatic, min(cols rounded up to 64, M); > 0 forces the width of the accumulator tile (a test hook like
 * item_slices of mfx_rec_query): a multiple of 64, at most M = 8192 for a selection of up to 512 (K at build, n_top at
 * recommend), 8128 above.
 * mfx_knn_create_from_lists makes a handle from given lists (copied).  Checked on the device, MFX_ERR_INVALID naming the
 * first bad item: ids below cols or pad, pads at the tail only, similarities of real slots finite.  No order is required:
 * the recommendation sum is order-free.
 * mfx_knn_lists copies the lists out (either array may be NULL).  mfx_knn_neighbours: the first n_top <= K stored slots of
 * the queried items (items = NULL: 0 .. nq - 1), out_sims may be NULL; an item >= cols is MFX_ERR_INVALID naming the query.
 * mfx_knn_times: seconds of the build's checks and work order and of its similarity pass (host clock), and stream seconds
 * of the checks and of the pass of mfx_knn_recommend summed over the calls.  mfx_knn_destroy(NULL) is 0.
 * MFX_ERR_INVALID without touching the device: a null argument, K or n_top out of range, nnz = 0 or cols < 2 (build and
 * from_lists), an unknown memory space or flag, a bad tile_items.  A failed build or from_lists leaves *out NULL.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_knn_s* mfx_knn_t;
#define MFX_KNN_KEEP_SEEN 1 /* flags of mfx_knn_recommend */
int mfx_knn_build(mfx_knn_t* out, const mfx_csx* X, int32_t K, int32_t tile_items, mfx_memspace space, int device);
int mfx_knn_create_from_lists(mfx_knn_t* out, int64_t cols, int32_t K, const uint32_t* nbr_idx, const float* nbr_sim,
                              mfx_memspace space, int device);
int mfx_knn_lists(mfx_knn_t h, uint32_t* nbr_idx, float* nbr_sim, mfx_memspace space);
int mfx_knn_neighbours(mfx_knn_t h, int64_t nq, const uint32_t* items, int32_t n_top, uint32_t* out_items, float* out_sims,
                       mfx_memspace space);
int mfx_knn_recommend(mfx_knn_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                      int32_t n_top, int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows,
                      mfx_memspace space);
int mfx_knn_times(mfx_knn_t h, double seconds[4]);
int mfx_knn_destroy(mfx_knn_t h);

/* ------------------------------------------------------------------------------------
 * SLIM on given supports (Ning & Karypis 2011, the feature-selected form "fsSLIM"): the learned item-item model.  For every
 * item j the column x_.j is regressed on the K columns of its support S_j with an elastic-net penalty,
 *   minimise over w:  1/2 ||x_.j - X_S w||^2 + l2 / 2 ||w||^2 + l1 ||w||_1   (w >= 0 unless MFX_SLIM_SIGNED),
 * by covariance-update coordinate descent on the Gram matrix of the support.  Every bit of the Gram entries, of the weights
 * and of the scores is fixed by the data and this text: no bit depends on lanes per item, the workgroup shape, the tile
 * width or the batch.
 *
 * Input.  X as for item-kNN (both orientations, values as given, the same structure checks, rows, cols, nnz < 2^32 - 1).
 * support [cols][K], 1 <= K <= 128, cols * K < 2^32 - 1: the ids of list j are distinct, below cols and never j itself; unused slots hold
 * 0xFFFFFFFF, at the tail only.  Checked on the device, MFX_ERR_INVALID naming the smallest bad item.  n_j is the number of
 * real slots of list j.
 *
 * Gram.  For items a != b, G_ab is the item-kNN similarity s_ab above: the fp32 terms fp32(x_ua * x_ub), truncated to the
 * 2^-36 grid, added as 64-bit integers, and the fp32 nearest to the sum.  d_a is the same sum over the terms
 * fp32(x_ua * x_ua).  A term (of a pair or of a diagonal) that is not finite or of magnitude >= 64, or a column of more
 * than 2^21 entries, is MFX_ERR_INVALID naming the smallest such item, as for item-kNN; every item's row is formed, whether
 * a list names the item or not.  The block of item j is [K + 1][K] fp32: entry (p, t) for p, t < n_j is G of the pair
 * (S_j[p], S_j[t]), with d on the diagonal; row K holds g_t = G of the pair (j, S_j[t]); everything else is +0.  G is
 * symmetric in bits, and with S the lists of an item-kNN build of the same X, row K equals that build's nbr_sim.
 *
 * Solve of one block with n real slots: w = 0 and c = g, then sweeps; a sweep visits a = 0 .. n - 1 in order:
 *   den = fp32(d_a + l2); unless den > 0 the coordinate is skipped;
 *   z = fma(d_a, w_a, c_a);
 *   r = fp32(z - l1), t = r if r > 0 else +0;  MFX_SLIM_SIGNED: r = fp32(|z| - l1), t = copysign(r if r > 0 else +0, z);
 *   v = fp32(t / den) (correctly rounded), delta = fp32(v - w_a);
 *   a delta that is not finite ends the item: its weights are stored as zeros, its sweep count as 0, and it is counted in
 *   *failed (a block formed from X has finite entries; this concerns blocks handed to the stand-alone solve);
 *   if delta != 0: c_b = fma(-delta, G_ab, c_b) for every b < n (b = a included), then w_a = v.
 * m is the largest |delta| of the sweep.  The item stops after the first sweep with m <= tol, or after `sweeps` sweeps; the
 * number of sweeps it ran is kept per item.  Slots n .. K - 1 of w hold +0.
 *
 * Model: support, w [cols][K], the sweep counts, and the transpose by source item: for every i the pairs (j, w_ij) with i
 * in S_j.  Recommendation is that of item-kNN over the transpose: for every entry (i, x) of a query row and every stored
 * (j, w) of source i the term fp32(x * w) goes on the 2^-36 grid into the 64-bit integer of j; eligible are the j whose sum
 * is not 0 and that are not in the row (MFX_KNN_KEEP_SEEN: the row's own items stay in); order, padding, bad rows
 * (*bad_rows), the checks of the rows, n_top <= 1024 and tile_items as for the item-kNN recommendation.
 *
 * The calls.  train: checks, Gram blocks of every item in a workspace of cols * (K + 1) * K * 4 bytes (MFX_ERR_ALLOC stating
 * the size when it cannot be had), solve, transpose.  *failed (host memory, may be NULL) receives the count of failed items.
 * tile_items: the test hook of the item-kNN build, for a selection of K.  gram: the blocks alone, [cols][K + 1][K].
 * solve: n blocks [n][K + 1][K] and their real-slot counts n_real [n] (NULL: K each; a count above K is taken as K) ->
 * w [n][K], sweeps_used [n], *failed; it reads no X, so any matrices may be handed in.
 * create_from_lists: a model from a support and weights (copied; the support checked as above, weights of real slots must
 * be finite; sweep counts 0).  weights: copies support, w and the sweep counts out (any may be NULL).
 * times: seconds of train's checks and inverse lists, of its Gram pass and of its solve (host clock), and stream seconds of
 * the checks and of the pass of the recommendation summed over the calls.  destroy of NULL is 0.
 * Parameters: l1, l2, tol finite and >= 0, sweeps >= 1, flags 0 or MFX_SLIM_SIGNED.  MFX_ERR_INVALID without touching the
 * device: a null argument, K, n_top or a parameter out of range, nnz = 0 or cols < 2, an unknown memory space or flag, a bad
 * tile_items.  A failed train or create_from_lists leaves *out NULL.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_slim_s* mfx_slim_t;
#define MFX_SLIM_SIGNED 1 /* flags of mfx_slim_train and mfx_slim_solve */
int mfx_slim_train(mfx_slim_t* out, const mfx_csx* X, int32_t K, const uint32_t* support, float l1, float l2, int32_t sweeps,
                   float tol, int flags, int32_t tile_items, int64_t* failed, mfx_memspace space, int device);
int mfx_slim_gram(const mfx_csx* X, int32_t K, const uint32_t* support, int32_t tile_items, float* blocks, mfx_memspace space,
                  int device);
int mfx_slim_solve(int64_t n, int32_t K, const float* blocks, const uint32_t* n_real, float l1, float l2, int32_t sweeps,
                   float tol, int flags, float* w, int32_t* sweeps_used, int64_t* failed, mfx_memspace space, int device);
int mfx_slim_create_from_lists(mfx_slim_t* out, int64_t cols, int32_t K, const uint32_t* support, const float* w,
                               mfx_memspace space, int device);
int mfx_slim_weights(mfx_slim_t h, uint32_t* support, float* w, int32_t* sweeps_used, mfx_memspace space);
int mfx_slim_recommend(mfx_slim_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                       int32_t n_top, int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows,
                       mfx_memspace space);
int mfx_slim_times(mfx_slim_t h, double seconds[5]);
int mfx_slim_destroy(mfx_slim_t h);

/* ------------------------------------------------------------------------------------
 * EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"): the closed-form dense item-item model, the
 * full-catalogue ridge form of SLIM.  With G = X^T X + lambda I and P = G^-1 the model is B = I - P diag(P)^-1 with a zero
 * diagonal.  Every bit of G, P, B and of the scores is fixed by the data and this text: no bit depends on the workgroup
 * shape, the tile width, the batch or the schedule of the inverse.
 *
 * Input.  X as for item-kNN (both orientations, values as given, the same structure checks), 2 <= cols <= 32768; lambda
 * finite and > 0.  Every dense matrix here is [cols][cols] fp32, row-major.
 *
 * Gram.  For i != j, G_ij is the item-kNN similarity s_ij above (terms fp32(x_ui * x_uj) on the 2^-36 grid, added as 64-bit
 * integers, the fp32 nearest to the sum).  G_ii = fp32(d_i + lambda) with d_i SLIM's diagonal, the fp32 of the same sum over
 * fp32(x_ui * x_ui).  G is symmetric in bits.  A term that is not finite or of magnitude >= 64, or a column of more than
 * 2^21 entries, is MFX_ERR_INVALID naming the smallest such item; unsorted or out-of-range ids are refused as at the item-kNN
 * build.
 *
 * Inverse.  mfx_ease_inverse is the algorithm of mfx_spd_inverse (csrc/spd_inverse.hip: blocked Cholesky on a copy padded to
 * a multiple of 32, T = L^-1, P = T^T T; diagonal blocks in fp64, every block product one chain of v_mfma_f32_32x32x2_f32
 * over the summed index, ascending) for 1 <= n <= 32768.  flags = 0 runs it with workgroups of four waves that own 4 x 4
 * blocks and stage operands in LDS, MFX_EASE_INV_SIMPLE with one wavefront per block; both return the same bits for every
 * n, and for n <= 1024 the bits of mfx_spd_inverse.  P is symmetric in bits.  A pivot that is <= 0 or not finite is
 * MFX_ERR_INVALID ("not positive definite"); the output is then unspecified.  The workspace is three padded copies.
 *
 * Weights.  B_ij = fp32((-P_ij) / P_jj) for i != j, one correctly rounded division; B_ii = +0.  Row i of B holds the weights
 * from source item i to every target j.  A P_jj that is not finite or not > 0 is MFX_ERR_INVALID naming the item.
 *
 * Recommendation for users given by CSR rows of (item i, value x), checked as mfx_knn_recommend checks them.  For every
 * item j the score starts at +0 and takes the row's entries e in stored order: s_j = fma(x_e, B[i_e][j], s_j).  Eligible:
 * every item not in the row (MFX_KNN_KEEP_SEEN: every item); zero and negative scores are candidates, NaN scores are
 * dropped.  Order and padding are those of mfx_rec_query, 1 <= n_top <= 1024.  An empty row returns pads and is not bad.
 * A row with a value that is not finite, or with more than 2^21 entries, is BAD: it returns all pads and is counted in
 * *bad_rows (host memory, may be NULL); the other rows are unaffected.  tile_items: the test hook of mfx_knn_recommend.
 *
 * The calls.  gram, inverse, weights_from_inverse: the three steps alone, arrays in `space`.  train: exactly gram ->
 * inverse -> weights_from_inverse on the device; G and the inverse's workspace are freed once P stands, the weights are
 * formed in place over P.  The peak is G + 3 padded copies + P: about 21 GB at cols = 32768; an allocation that fails is
 * MFX_ERR_ALLOC stating the size.  tile_items of gram and train: the test hook of the item-kNN build.
 * create_from_weights: a model from a given B (copied), checked on the device: every entry finite, the diagonal zero, else
 * MFX_ERR_INVALID naming the first bad row.  weights: rows first .. first + count - 1 of B, [count][cols].
 * times: seconds of train's checks and work order, Gram pass, inverse and weights step (host clock), and stream seconds of
 * the checks and of the pass of the recommendation summed over the calls.  destroy of NULL is 0.
 * MFX_ERR_INVALID without touching the device: a null argument, cols < 2 or > 32768, n < 1 or > 32768, nnz = 0, lambda not
 * finite or <= 0, n_top out of range, an unknown memory space or flag, a bad tile_items.  A failed train or
 * create_from_weights leaves *out NULL.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_ease_s* mfx_ease_t;
#define MFX_EASE_INV_SIMPLE 1 /* flags of mfx_ease_inverse and mfx_ease_train: one wavefront per 32 x 32 block */
int mfx_ease_gram(const mfx_csx* X, float lambda, int32_t tile_items, float* G, mfx_memspace space, int device);
int mfx_ease_inverse(int64_t n, const float* A, float* Ainv, int flags, mfx_memspace space, int device);
int mfx_ease_weights_from_inverse(int64_t n, const float* P, float* B, mfx_memspace space, int device);
int mfx_ease_train(mfx_ease_t* out, const mfx_csx* X, float lambda, int flags, int32_t tile_items, mfx_memspace space,
                   int device);
int mfx_ease_create_from_weights(mfx_ease_t* out, int64_t cols, const float* B, mfx_memspace space, int device);
int mfx_ease_weights(mfx_ease_t h, int64_t first, int64_t count, float* B_rows, mfx_memspace space);
int mfx_ease_recommend(mfx_ease_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                       int32_t n_top, int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows,
                       mfx_memspace space);
int mfx_ease_times(mfx_ease_t h, double seconds[6]);
int mfx_ease_destroy(mfx_ease_t h);

/* ------------------------------------------------------------------------------------
 * Top-N recommendation: a resident handle over trained factors that returns, for each
 * requested user, the n_top highest-scoring items the user must not be excluded from.
 * Score of (u, i) = the fp32 fused multiply-add chain in ascending t: acc = +0, then
 * acc = fmaf(W[u,t], H[i,t], acc) for t = 0 .. k-1, one rounding per step, subnormals kept
 * (bitwise the same whatever the batch, its order, item_slices or layout).  Order: score
 * descending, then item ascending (-0 == +0); NaN scores are never returned.  Slots left
 * when fewer than n_top items are eligible hold item 0xFFFFFFFF and score -INFINITY.
 * Range: 1 <= n_top <= 1024, 1 <= k <= 1024; anything else is MFX_ERR_INVALID.
 * ---------------------------------------------------------------------------------- */
typedef struct mfx_rec_s* mfx_rec_t;
/* layout 0: CCD++ factors, W [k][rows], H [k][cols]; layout 1: ALS factors, W [rows][k], H [cols][k].
 * Copies (and repacks) W and H into library-owned device memory.
 * exclude: NULL, or a rating matrix of the same rows x cols; only csr_row_ptr / csr_col_idx are read:
 * the items each user is never recommended.  Column indices must be non-decreasing within every row
 * (checked on the device; MFX_ERR_INVALID otherwise).  `space` applies to W, H and exclude. */
int mfx_rec_create(mfx_rec_t* out, const float* W, const float* H, int64_t rows, int64_t cols, int64_t k,
                   int layout, const mfx_csx* exclude, mfx_memspace space, int device);
/* Top-n_top items of each of nusers users.  users: NULL means 0 .. nusers-1; any order, duplicates
 * allowed.  items [nusers][n_top], scores [nusers][n_top] or NULL; `space` applies to all three.
 * item_slices: 0 = automatic; > 0 forces the item dimension to be split over that many slices
 * (a test hook; item_slices * n_top must not exceed 8192). */
int mfx_rec_query(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t n_top, uint32_t* items,
                  float* scores, mfx_memspace space, int item_slices);
/* Fold-in: users given by their interactions (users who arrived after training, or whose history changed) rather
 * than by a row of W.  With the handle's H fixed, one factor row per query user is solved from the user's entries and
 * then scored like mfx_rec_query.  H_O: the rows of H the user's entries name, r: their values. */
typedef enum mfx_fold_model {
    MFX_FOLD_ALS = 0,       /* (H_O^T H_O + lambda I) w = H_O^T r                  == mfx_als_half variant 1, bit for bit */
    MFX_FOLD_ALS_EXACT = 1, /* the same system in the reference's operation order == mfx_als_half variant 0, bit for bit */
    MFX_FOLD_CCD = 2,       /* (H_O^T H_O + fp32(lambda * n_u) I) w = H_O^T r, n_u = stored entries of the row: the exact
                               minimiser of the CCD++ objective (denominator lambda |Omega| + sum v^2, mfx_rank_one_sweep)
                               over the row, H fixed */
    MFX_FOLD_IMPLICIT = 3   /* (H^T H + lambda I + sum_j w_j h_j h_j^T) w = sum_{r_j > 0} (1 + w_j) h_j, w_j = fp32(alpha r_j)
                                                                                   == mfx_ials_half, bit for bit */
} mfx_fold_model;
/* Prepares fold-in on r: keeps H row-major (unpacked from the handle's own copy: the very bits it scores with, for
 * either layout) with one all-zero row behind it, and for MFX_FOLD_IMPLICIT the base Gramian H^T H + lambda I.  May be
 * called again with another model, lambda or alpha.  MFX_ERR_INVALID: k > 128, lambda <= 0 or not finite, alpha < 0
 * or not finite, an unknown model. */
int mfx_rec_fold_in_setup(mfx_rec_t r, int model, float lambda, float alpha);
/* Solves one factor row per query user from the CSR rows ptr [nusers+1] / idx [nnz] / val [nnz] (column ids < cols,
 * non-decreasing within a row, as for the exclude matrix of mfx_rec_create; checked on the device, as are the values
 * of MFX_FOLD_IMPLICIT: finite, >= 0, alpha * r finite), then returns the n_top best items of each row with the row's
 * own items excluded, ranked as mfx_rec_query ranks.  A row without entries gets w = 0 under every model.
 * W_out [nusers][k] or NULL.  n_top = 0: solve only (items / scores ignored); else 1 <= n_top <= 1024, items
 * [nusers][n_top], scores [nusers][n_top] or NULL.  `space` applies to every array.  MFX_ERR_INVALID before the first
 * successful mfx_rec_fold_in_setup; a refused query leaves the handle usable. */
int mfx_rec_fold_in(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                    float* W_out, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space);
/* Fold-in by block subspace sweeps, the method of mfx_ials_block_create: any 1 <= k <= 1024.
 * block: 0 = ialsb_default_block(k) (k below 64, else 64), else 1..128 (clamped to k as mfx_ials_block_half does).
 * sweeps: 1..1024, the most sweeps a row gets.  tol >= 0, finite: 0 = every non-empty row gets exactly `sweeps`.
 * Keeps H row-major as mfx_rec_fold_in_setup does, G = H^T H + lambda I as mfx_ials_block_half builds it, H block-major
 * and the diagonal blocks of G (one more copy of H on the device).  One sweep over the query rows is one
 * mfx_ials_block_half from the rows' current values: with tol = 0, S sweeps equal S chained calls bit for bit.
 * tol > 0: after each sweep a row is frozen once max_c |y_new[c] - y_old[c]| <= tol * max_c |y_new[c]| (fp32); a frozen
 * row's bits never change again, and the loop ends when every row is frozen or `sweeps` is reached (the host reads one
 * counter per sweep).  A row's bits and its sweep count do not depend on the other rows of the batch.
 * A sweep is not a solve: from w = 0 the distance to the minimiser shrinks by a factor per sweep that depends on the row,
 * and at large alpha short rows are the slow ones (DESIGN.md has the table): choose sweeps / tol for the data, pass
 * the row's previous factors as W_init, or set up mfx_rec_fold_in_cg_setup, which solves and bounds the residual.
 * The last successful setup of any kind decides what mfx_rec_fold_in does; after this one it is mfx_rec_fold_in_warm
 * with W_init = NULL and sweeps_done = NULL.  MFX_ERR_INVALID: block outside 0..128, sweeps outside 1..1024, tol < 0 or
 * not finite, lambda <= 0 or not finite, alpha < 0 or not finite. */
int mfx_rec_fold_in_block_setup(mfx_rec_t r, float lambda, float alpha, int32_t block, int32_t sweeps, float tol);
/* The same for the explicit objectives, the method of mfx_als_block_create: reg 0 minimises what MFX_FOLD_ALS solves, reg 1
 * what MFX_FOLD_CCD solves (fp32(lambda * n_u) on the diagonal), at any 1 <= k <= 1024.  block, sweeps and tol as above.
 * Keeps H row-major and block-major (no Gramian).  One sweep over the query rows is one mfx_als_block_half from the
 * rows' current values: with tol = 0, S sweeps equal S chained calls bit for bit; tol > 0 freezes rows by the rule above.
 * With a single block (block >= k) one sweep is the exact solve; with more blocks a sweep is not a solve: from w = 0 the
 * distance to the minimiser shrinks by a factor per sweep that depends on the row (DESIGN.md has the sweep counts):
 * choose sweeps / tol for the data, pass the row's previous factors as W_init, or set up mfx_rec_fold_in_cg_setup (a solve
 * with a residual bound).  Values: finite (checked on the device);
 * zeros and negative values are entries like any other.
 * The last successful setup of the three kinds decides what mfx_rec_fold_in does; after this one it is
 * mfx_rec_fold_in_warm with W_init = NULL and sweeps_done = NULL.  MFX_ERR_INVALID: reg not 0 / 1, block outside 0..128,
 * sweeps outside 1..1024, tol < 0 or not finite, lambda <= 0 or not finite. */
int mfx_rec_fold_in_block_setup_als(mfx_rec_t r, float lambda, int32_t reg, int32_t block, int32_t sweeps, float tol);
/* Fold-in on the objective of mfx_ials_create_reg / mfx_ials_block_create_reg: a query row u has N = cols and n_u = its
 * entries with r > 0; rho_u is formed on the device for every query batch.  mfx_rec_fold_in_setup_reg (k <= 128) keeps
 * G0 = fp32(alpha0 H^T H) and makes mfx_rec_fold_in equal mfx_ials_half_reg of the same rows over the handle's H bit for bit;
 * mfx_rec_fold_in_block_setup_reg keeps what mfx_rec_fold_in_block_setup keeps, over G0, and one sweep equals one
 * mfx_ials_block_half_reg bit for bit.  Afterwards mfx_rec_fold_in and mfx_rec_fold_in_warm, the stop rule and "the last
 * successful setup decides" are those of the un-suffixed setups.  MFX_ERR_INVALID: what those refuse, and alpha0 / nu /
 * the regulariser as for mfx_ials_create_reg (rows = cols = the handle's cols). */
int mfx_rec_fold_in_setup_reg(mfx_rec_t r, float lambda, float alpha, float alpha0, float nu);
int mfx_rec_fold_in_block_setup_reg(mfx_rec_t r, float lambda, float alpha, float alpha0, float nu, int32_t block, int32_t sweeps, float tol);
/* Fold-in by conjugate gradients preconditioned by the inverse of the base Gramian, at any 1 <= k <= 1024: a solve with a
 * residual bound, not a sweep.  H is fixed, so the system of a row of n entries is a fixed base plus a matrix of rank n, and
 * the method ends, in exact arithmetic, after at most n + 1 steps: short rows are the cheap ones.
 * model: MFX_FOLD_ALS, MFX_FOLD_CCD or MFX_FOLD_IMPLICIT, the objectives of mfx_rec_fold_in_setup (MFX_FOLD_ALS_EXACT is an
 * order of operations, not an objective: refused).  steps: 1..1024, the most steps a row gets.  tol >= 0, finite.
 *   implicit:  A p = G p + sum_e w_e <h_e, p> h_e,  b = sum_e fp32(1 + w_e) h_e,  w_e = fp32(alpha r_e),  preconditioner Minv
 *              over the entries with r_e > 0; G = H^T H + lambda I as mfx_ials_block_half builds it, Minv [k][k] its inverse
 *              by Cholesky in fp64 on the host, rounded to fp32 and symmetric (setup time grows as k^3: README has it)
 *   explicit:  A p = rho p + sum_e <h_e, p> h_e,  b = sum_e r_e h_e,  rho = lambda (ALS) or fp32(lambda n) (CCD), over every
 *              entry, zeros and negative values included; no G, the preconditioner is the identity
 * From y = the start row (0 for mfx_rec_fold_in), r = b - A y, z = Minv r, p = z, gamma = <r, z>, a step is q = A p,
 * a = gamma / <p, q>, y += a p, r -= a q, [stop test], z = Minv r, gamma' = <r, z>, p = z + (gamma' / gamma) p.
 * A row without counting entries or with b = 0 gets w = 0 and 0 steps whatever the start row holds.  tol > 0: a row is
 * frozen once |r| <= tol |b| (2-norms, fp32); the test runs on the start row too, so a good W_init costs 0 steps, and the
 * step that reaches the bound is counted.  tol = 0: every other row gets exactly `steps` unless gamma becomes exactly 0.
 * A frozen row's bits never change again; the loop ends when every row is frozen or `steps` is reached (the host reads one
 * counter per step when tol > 0).  <p, q> < 0 or not finite (the inputs were not finite): the row comes back as NaN;
 * <p, q> exactly 0 (the direction of a row long converged underflowed) freezes the row like gamma = 0.
 * No float atomics: a row's bits and step count do not depend on the other rows of the batch, their order, the memory
 * space or the factor layout, and a row stopped after s steps has the bits of the same row run with steps = s, tol = 0.
 * Afterwards mfx_rec_fold_in is the cold start and mfx_rec_fold_in_warm is valid (sweeps_done receives the steps); query
 * checks, exclusion, item filter, scoring and padding are those of mfx_rec_fold_in.  Keeps H row-major and, for the
 * implicit model, G and Minv.  The last successful setup of the four kinds decides what mfx_rec_fold_in does.
 * MFX_ERR_INVALID (the handle keeps what it had): model unknown or MFX_FOLD_ALS_EXACT, steps outside 1..1024, tol < 0 or not
 * finite, lambda <= 0 or not finite, alpha < 0 or not finite, k > 1024. */
int mfx_rec_fold_in_cg_setup(mfx_rec_t r, int model, float lambda, float alpha, int32_t steps, float tol);
/* mfx_rec_fold_in with a start row per user and the sweep counts.  W_init [nusers][k] or NULL (start from 0);
 * sweeps_done [nusers] or NULL: the sweeps applied to each row (after mfx_rec_fold_in_cg_setup: the steps).  An empty row
 * gives w = 0 and 0 sweeps whatever W_init holds.  The query checks are those of MFX_FOLD_IMPLICIT (after
 * mfx_rec_fold_in_block_setup_als and the explicit models of mfx_rec_fold_in_cg_setup: finite values).  Valid only after
 * mfx_rec_fold_in_block_setup, mfx_rec_fold_in_block_setup_als or mfx_rec_fold_in_cg_setup: MFX_ERR_INVALID after
 * mfx_rec_fold_in_setup or no setup, and the handle stays usable. */
int mfx_rec_fold_in_warm(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                         const float* W_init, float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items,
                         float* scores, mfx_memspace space);
/* Wall-clock seconds of the last mfx_rec_fold_in / mfx_rec_fold_in_warm on r, each phase ending in a stream synchronisation: [0] host build
 * (query upload, checks, the host-side split into work items), [1] solve, [2] score (packing, top-N, copies out). */
int mfx_rec_fold_in_times(mfx_rec_t r, double seconds[3]);
/* Why an item scores what it scores for a fold-in user: the score split over the user's own interactions.
 * The fold-in row is w = A^-1 sum_e b_e h_e over the entries e = (item j_e, value r_e) of the query row, so the score of a
 * target item i is <h_i, w> = sum_e b_e <h_e, A^-1 h_i>.  The explanation is of the fold-in row of the given interactions,
 * not of a row of the handle's W.
 * Valid after mfx_rec_fold_in_setup with MFX_FOLD_ALS, MFX_FOLD_CCD or MFX_FOLD_IMPLICIT, or mfx_rec_fold_in_setup_reg.
 * MFX_ERR_INVALID (the handle stays usable) before any setup, after MFX_FOLD_ALS_EXACT (its rows are not the bits of the
 * MFMA system: use MFX_FOLD_ALS), after any block setup (a sweep is not a solve: the split does not hold) and after
 * mfx_rec_fold_in_cg_setup (the split here uses the factor of the row's system: there mfx_rec_explain_cg explains).
 * Query rows ptr / idx / val: as for mfx_rec_fold_in, with the same checks.  targets [nusers][n_targets]: item ids below
 * cols, or 0xFFFFFFFF = padding (checked on the device), so the padded `items` of mfx_rec_fold_in may be passed as they
 * are; a target may repeat and may be one of the row's own items.  The exclusion matrix and the item filter play no part.
 * 1 <= n_targets <= 64, 0 <= n_expl <= 64 (0: expl_items / expl_contrib are not read), nusers = 0: MFX_OK, nothing touched.
 *   system A of the row and weight b_e of an entry, per setup:
 *     MFX_FOLD_ALS       sum h h^T + lambda I                     b_e = r_e                          every entry counts
 *     MFX_FOLD_CCD       sum h h^T + fp32(lambda n) I             b_e = r_e                          every entry counts
 *     MFX_FOLD_IMPLICIT  G + sum w_e h h^T, w_e = fp32(alpha r_e)  b_e = fp32(1 + w_e)                r_e > 0 counts
 *     _setup_reg         G0 + rho I + sum w_e h h^T               b_e = fp32(alpha0 + w_e)           r_e > 0 counts
 *   W_out [nusers][k] or NULL: the fold-in row, bit for bit what mfx_rec_fold_in returns for the row under the same
 *     setup (an empty row: 0).
 *   totals [nusers][n_targets] or NULL: the score chain of mfx_rec_query over (W_out[q], H[target]), bit for bit -- what
 *     mfx_rec_fold_in reports for that item; -INFINITY for a padding target.
 *   Z_out [nusers][n_targets][k] or NULL: z = A^-1 h_target by the factor L that gave W_out[q] and the same forward and
 *     backward substitution, one more right-hand side per target; 0 for a padding target and for an empty row.
 *   contribution of entry e to target t: d = the fmaf chain over c = 0 .. k-1 ascending from +0 of Z[q][t][c] * H[j_e][c]
 *     (H: the handle's own bits), c_e = fp32(b_e * d), one rounding: bit-determined by the bits of Z_out.
 *   expl_items / expl_contrib [nusers][n_targets][n_expl]: the counting entries of the row by c_e descending, then by
 *     position in the row ascending (-0 == +0; a NaN contribution is dropped), padded with (0xFFFFFFFF, -INFINITY); two
 *     entries with the same item id are two entries; every slot of a padding target is padding.
 * A slot's results do not depend on the batch, its order, the memory space or the factor layout.  A system that is not
 * positive definite is treated as mfx_rec_fold_in treats it (the row and what derives from it are not finite).
 * Device workspace of a call: 4 k n_targets bytes per slot for Z, what mfx_rec_fold_in takes for the same rows, the lists
 * (8 n_targets n_expl bytes per slot when `space` is MFX_HOST) and, when a row is longer than 2048 entries, two partial
 * lists per 2048 entries of the batch and target (16 n_targets n_expl bytes per 2048 entries).  The caller cuts very
 * large batches (mfx.Recommender.explain does, by max_ws_bytes). */
int mfx_rec_explain(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                    int32_t n_targets, const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib,
                    float* totals, float* W_out, float* Z_out, mfx_memspace space);
/* mfx_rec_explain at any 1 <= k <= 1024, after mfx_rec_fold_in_cg_setup: the split <h_t, w> = sum_e b_e <h_e, z>, A z = h_t,
 * holds for any method that solves for z, up to that method's residual, and conjugate gradients solve.
 * Valid only after a successful mfx_rec_fold_in_cg_setup (MFX_FOLD_ALS, MFX_FOLD_CCD or MFX_FOLD_IMPLICIT); lambda, alpha,
 * steps and tol are that setup's.  MFX_ERR_INVALID (the handle stays usable, the message names mfx_rec_fold_in_cg_setup)
 * before any setup, after mfx_rec_fold_in_setup / _setup_reg (mfx_rec_explain explains there) and after any block setup.
 * Arguments and checks are those of mfx_rec_explain, the rows checked as mfx_rec_fold_in checks them under the cg setup;
 * nusers * n_targets < 2^31.  row_steps [nusers] and target_steps [nusers][n_targets] may be NULL; `space` applies to
 * every array.
 *   W_out, row_steps: bit for bit what mfx_rec_fold_in (the cold start) and its sweeps_done give for the row.
 *   Z_out[q][t]: the iterate of A_q z = h_t from z = 0 by exactly the recurrence of mfx_rec_fold_in_cg_setup, with the A and
 *     the preconditioner of row q (the table there: implicit over the entries with r_e > 0, explicit over every entry) and
 *     b = the handle's own bits of H[target].  The stop rule is |r| <= tol |h_t| (2-norms, fp32), tested on the start too, the
 *     step that reaches it counted into target_steps; tol = 0: exactly `steps` steps unless gamma becomes exactly 0.
 *     A padding target, a row without counting entries (implicit: no r_e > 0; explicit: an empty row) and a target with
 *     h_t = 0: z = 0 and 0 steps.  <p, q> < 0 or not finite: the pair's z is NaN and frozen; <p, q> exactly 0 freezes it.
 *   totals, expl_items, expl_contrib: the definitions of mfx_rec_explain from W_out and Z_out (the score chain; b_e = r_e,
 *     or fp32(1 + fp32(alpha r_e)) over r_e > 0 for the implicit model; order, padding and duplicates as there).
 * Accuracy: the split holds up to the residuals.  With r_w = b - A w and r_z = h_t - A z (A symmetric),
 * <b, z> - <h_t, w> = <r_w, z> - <r_z, w>, so |sum_e c_e - total| <~ tol (|b| |z| + |h_t| |w|) plus fp32 rounding; a smaller
 * tol at setup tightens it.
 * No float atomics: the bits and the step count of a (row, target) pair do not depend on the batch, its order, duplicates,
 * n_targets, the other targets of the slot, the target's position in it, the memory space or the factor layout, and a pair
 * stopped after s steps has the bits of the same pair run with steps = s, tol = 0.
 * Device workspace of a call: per slot 4 k n_targets bytes each for Z, the residual, the direction and A p, and for the
 * preconditioned residual under the implicit model; 16 bytes per pair; 4 k n_targets bytes per partial slot of a row longer
 * than 2048 entries (one slot per 2048 entries); what mfx_rec_fold_in takes for the same rows under this setup, and the
 * lists as for mfx_rec_explain.  The caller cuts very large batches (mfx.Recommender.explain_cg does, by max_ws_bytes). */
int mfx_rec_explain_cg(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                       int32_t n_targets, const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib,
                       float* totals, float* W_out, float* Z_out, int32_t* row_steps, int32_t* target_steps, mfx_memspace space);
/* Wall-clock seconds of the last mfx_rec_explain or mfx_rec_explain_cg on r, each phase ending in a stream synchronisation:
 * [0] host build and checks (rows and targets), [1] solve (the row and the n_targets further right-hand sides; _cg: the row
 * solve plus the target solves), [2] totals, contributions, selection and the copies out. */
int mfx_rec_explain_times(mfx_rec_t r, double seconds[3]);
/* Item filter: keep [cols] bytes in `space`, non-zero = the item may be returned; NULL removes the filter.  Copied.
 * Applies to every later mfx_rec_query, mfx_rec_fold_in, mfx_rec_fold_in_warm and mfx_rec_similar on r until replaced:
 * the result is the unfiltered ranking with the filtered items removed and the list refilled, score bits unchanged
 * (the fold-in solve still sees all of the user's entries).  It works beside the exclude matrix of mfx_rec_create, not
 * instead of it.  MFX_ERR_INVALID: a bad memory space; the handle keeps the filter it had. */
int mfx_rec_set_item_filter(mfx_rec_t r, const uint8_t* keep, mfx_memspace space);
/* Item-to-item similarity: the n_top rows of H nearest to row q of H.  s(q, i) is the score chain of mfx_rec_query with
 * H[q] in the place of W[u]; n2[i] = s(i, i), the same chain; c[i] = an fp32 approximation of 1 / sqrt(n2[i]) within 2 ulp
 * of the fp64 value rounded to fp32, +0 where n2[i] is 0 or not finite. */
typedef enum mfx_rec_metric {
    MFX_SIM_DOT = 0,    /* ranking key and returned score: s(q, i) */
    MFX_SIM_COSINE = 1  /* ranking key: key = fp32(s(q, i) * c[i]), one rounding, subnormals kept; returned score:
                           fp32(key * c[q]).  A returned cosine may exceed 1 by an ulp or two; it is not clamped. */
} mfx_rec_metric;
/* Prepares item-to-item queries on r: the rows of H as a query operand (from the handle's own packed copy: the bits it
 * scores with, either layout; one more copy of H on the device) and the per-item n2 and c.  Idempotent. */
int mfx_rec_similar_setup(mfx_rec_t r);
/* The n2 [cols] and c [cols] that mfx_rec_similar uses, bit for bit; either may be NULL.  MFX_ERR_INVALID before
 * mfx_rec_similar_setup or with a bad memory space. */
int mfx_rec_item_norms(mfx_rec_t r, float* n2, float* c, mfx_memspace space);
/* The n_top items most similar to each of nq query items.  query_items: NULL means 0 .. nq-1; any order, duplicates
 * allowed.  items [nq][n_top], scores [nq][n_top] or NULL; `space` applies to all three; item_slices as in mfx_rec_query.
 * Order: key descending, then item ascending (-0 == +0); NaN keys are never returned; two different keys that round to
 * the same returned score stay in key order.  Padding as in mfx_rec_query.  exclude_self != 0: item q is not returned for
 * query q (other items with the same row are).  The exclude matrix of mfx_rec_create plays no part; the item filter
 * does, and a filtered-out item can still be a query.  The result does not depend on the batch, its order,
 * item_slices, the factor layout or host / device pointers.
 * MFX_ERR_INVALID, the handle left usable: before mfx_rec_similar_setup, an unknown metric, n_top outside 1..1024,
 * item_slices * n_top > 8192, a query item >= cols (checked on the device), a bad memory space. */
int mfx_rec_similar(mfx_rec_t r, int64_t nq, const uint32_t* query_items, int metric, int exclude_self, int32_t n_top,
                    uint32_t* items, float* scores, mfx_memspace space, int item_slices);
/* Exact catalogue ranks of given (user, item) pairs: where does item i stand for user u?
 * Item j is eligible for u when j < cols, j is not in u's row of the exclude matrix of mfx_rec_create, the item filter
 * (if one is set) keeps j, and j's ranking key is not NaN.  The key is the score chain of mfx_rec_query; with a filter set
 * it is fp32(score * the handle's per-item factor), as the top-N pass forms it.
 * ranks[p]: the number of items j != i eligible for u that order before i (key(u,j) > key(u,i), or equal keys and j < i;
 *   -0 == +0, +-inf ordinary values); 0xFFFFFFFF when i itself is not eligible for u.  So ranks[p] = r < 0xFFFFFFFF if and
 *   only if mfx_rec_query for u returns i at position r for every n_top > r, and 0xFFFFFFFF if and only if no query
 *   ever returns i for u.
 * scores[p] (may be NULL): the score chain of (u, i), bit for bit, eligible or not.
 * n_eligible[p] (may be NULL): the number of items eligible for u, the target included if it is; a column id repeated in
 *   an exclusion row counts once.
 * Pairs in any order, duplicates allowed; `space` applies to all five arrays; item_slices as in mfx_rec_query (0 =
 * automatic, > 0 forces the split: a test hook).  A pair's results do not depend on the batch, its order, item_slices,
 * the factor layout or the memory space.  Nothing of size users x items is stored: 12 bytes per pair during the call, and
 * from the first call on one more copy of H in the handle (cols x k, row-major, the one mfx_rec_similar_setup keeps).
 * MFX_ERR_INVALID, the handle left usable: ranks, users or items NULL with npairs > 0, a user >= rows or an item >= cols
 * (checked on the device), item_slices < 0, a bad memory space.  npairs == 0 is MFX_OK and touches nothing. */
int mfx_rec_rank(mfx_rec_t r, int64_t npairs, const uint32_t* users, const uint32_t* items, uint32_t* ranks, float* scores,
                 uint32_t* n_eligible, mfx_memspace space, int item_slices);
/* Device seconds of the last mfx_rec_rank (or mfx_rec_evaluate) on r by phase: [0] target keys, [1] counting pass,
 * [2] exclusion correction. */
int mfx_rec_rank_times(mfx_rec_t r, double seconds[3]);
/* Ranking metrics of the handle's model on a held-out set T (`space` applies to its arrays) from exact ranks, so no cutoff
 * limit and no list.  Users as in mfx_topn_metrics: R_u = the distinct test items of u with value >= min_rating, users
 * with an empty R_u are skipped, *users_evaluated is the number kept.  One mfx_rec_rank of all kept pairs runs on the
 * device; every sum below is fp64 on the host.
 * out[c] = {HR, precision, recall, NDCG} at cutoff N = cutoffs[c] >= 1 (not limited to 1024), the definitions of
 *   mfx_topn_metrics with "hit" meaning rank < N: for N <= 1024 the metrics of the lists of mfx_rec_query(n_top = N).
 * *mrr: mean over the kept users of 1 / (1 + smallest rank in R_u), 0 for a user whose targets are all ineligible.
 * *auc: for user u, P_u = its eligible targets, neg = n_eligible - |P_u|, AUC_u = mean over p in P_u of
 *   (neg - (rank_p - a_p)) / neg with a_p = the number of other targets of u ranked before p; the mean of AUC_u over the
 *   users with P_u not empty and neg > 0, whose number is *auc_users.
 * mrr, auc, users_evaluated, auc_users may be NULL; n_cut == 0 is allowed (cutoffs and out are then not read).
 * MFX_ERR_INVALID: NaN min_rating, a cutoff < 1, a test row >= rows or column >= cols, a bad memory space. */
int mfx_rec_evaluate(mfx_rec_t r, const mfx_coo* T, float min_rating, int32_t n_cut, const int32_t* cutoffs,
                     double* out /* [n_cut][4] */, double* mrr, double* auc, int64_t* users_evaluated, int64_t* auc_users,
                     mfx_memspace space);
/* Re-ranking of given candidate lists, the second stage of a two-stage recommender: the n_top best eligible items of each
 * slot's own list instead of the catalogue's.
 * Slot q is user users[q] (q when users is NULL; any order, duplicates allowed) and its candidates are
 * cand_idx[cand_ptr[q] .. cand_ptr[q+1]): a CSR of nusers rows, cand_ptr [nusers + 1] starting at 0 and non-decreasing,
 * the ids of every row strictly ascending and below cols.  All of that is checked on the device; a violation is
 * MFX_ERR_INVALID, the message names the first offending slot, and the handle stays usable.  A row may be empty or the
 * whole catalogue.  cand_idx may be NULL when every row is empty.
 * A candidate is eligible as mfx_rec_rank defines it: not in the user's row of the exclude matrix of mfx_rec_create
 * (flag MFX_CAND_NO_EXCLUDE: the exclude matrix plays no part), kept by the item filter if one is set, its key not NaN.
 * items [nusers][n_top], scores [nusers][n_top] or NULL: the eligible candidates in the order of mfx_rec_query (key
 * descending, then item ascending; -0 == +0; +-inf ordinary values), padded with (0xFFFFFFFF, -INFINITY); a returned
 * score is the score chain of mfx_rec_query, bit for bit.  n_eligible [nusers] or NULL: the eligible candidates of the
 * slot.  `space` applies to all six arrays.  A slot's result does not depend on the batch, its order, the memory space
 * or the factor layout.
 * Nothing of size users x items is stored.  Workspace during the call: 4 bytes per slot twice (the lists longer than 2048
 * candidates, the slot of every piece of work) plus 4 bytes per 2048 candidates, and, only when some list is longer than
 * 2048, 16 * n_top bytes per 2048 candidates (at most 8 bytes per candidate) for the partial lists of its pieces; from
 * the first call on the row-major copy of H that mfx_rec_rank keeps.  With `space` = MFX_HOST also the device copies
 * of the arguments and results.
 * MFX_ERR_INVALID: n_top outside 1..1024, unknown flag bits, cand_ptr or items NULL, cand_idx NULL with a non-empty
 * list, a user >= rows, a bad memory space.  nusers == 0 is MFX_OK and touches nothing. */
#define MFX_CAND_NO_EXCLUDE 1   /* do not take the handle's exclusion rows off the lists */
int mfx_rec_query_candidates(mfx_rec_t r, int64_t nusers, const uint32_t* users, const uint32_t* cand_ptr,
                             const uint32_t* cand_idx, int32_t flags, int32_t n_top, uint32_t* items, float* scores,
                             uint32_t* n_eligible, mfx_memspace space);
/* scores[p] = the score chain of (users[p], items[p]), bit for bit, eligible or not: the bits mfx_rec_rank returns in its
 * scores, without the ranks.  Pairs in any order, duplicates allowed; ids checked on the device; `space` applies to the
 * three arrays.  MFX_ERR_INVALID, the handle left usable: a NULL array with npairs > 0, a user >= rows, an item >= cols,
 * a bad memory space.  npairs == 0 is MFX_OK. */
int mfx_rec_score(mfx_rec_t r, int64_t npairs, const uint32_t* users, const uint32_t* items, float* scores,
                  mfx_memspace space);
/* Stream seconds of the last mfx_rec_query_candidates on r by phase: [0] check + stage (copies in, the validity
 * checks and their read-back, the piece table), [1] score (the kernel that scores every piece and selects within it),
 * [2] select (the merge of the lists longer than 2048 candidates; 0 when there is none).  After mfx_rec_score: [0] stage,
 * [1] score, [2] 0. */
int mfx_rec_candidates_times(mfx_rec_t r, double seconds[3]);
/* Diversity re-ranking of given candidate lists by greedy maximal marginal relevance (MMR): the page a caller shows
 * instead of the n_top nearest neighbours of one another that relevance alone returns.
 * Slot q has a user and a candidate list exactly as in mfx_rec_query_candidates: the list is a CSR row, ids strictly
 * ascending and below cols, checked on the device.  A candidate is eligible as defined there: not in the user's exclusion
 * row (flag MFX_DIV_NO_EXCLUDE: the exclude matrix plays no part), kept by the item filter, its score not NaN.  E: the
 * eligible candidates of the slot.
 *   rel(i) = the score chain of mfx_rec_query for (user, i), bit for bit;
 *   a = tradeoff as fp32, b = fp32(1 - a), D_0(i) = +0 for every i in E.
 * For s = 1 .. min(n_top, |E|):
 *   1. value_s(i) = fmaf(-b, D_{s-1}(i), fp32(a * rel(i))) for every i in E not picked yet;
 *   2. i_s = the candidate of the greatest value, then of the greater rel, then of the smaller item id; a NaN value
 *      counts as -INFINITY, and -0 == +0 in both comparisons;
 *   3. D_s(i) = sim(i_s, i) if that is greater than D_{s-1}(i), else D_{s-1}(i); a NaN similarity leaves D as it was.
 * sim by metric: MFX_SIM_DOT: sim(j, i) = the chain fma(H[j][t], H[i][t], acc) over t = 0 .. k-1 from +0, the s(q, i) of
 * mfx_rec_similar; MFX_SIM_COSINE: fp32(fp32(s(j, i) * c[i]) * c[j]), the score mfx_rec_similar(query j, MFX_SIM_COSINE)
 * returns for item i, with the c of mfx_rec_item_norms.  D starts at +0, so a similarity below 0 never raises a candidate's
 * D: items less alike than orthogonal ones are penalised like orthogonal ones, not rewarded.
 * items [nusers][n_top] in pick order; scores [nusers][n_top] or NULL: rel; values [nusers][n_top] or NULL: the value at
 * the moment of the pick as computed (it may be NaN); n_eligible [nusers] or NULL: |E|.  The positions left over hold
 * (0xFFFFFFFF, -INFINITY, -INFINITY).  A slot's result does not depend on the batch, its order, the memory space, the
 * factor layout or `form`.  With tradeoff = 1 and finite similarities value = rel, and items and scores equal those of
 * mfx_rec_query_candidates with the same flags, bit for bit.
 * users as in mfx_rec_query_candidates.  Wq: NULL, or [nusers][k] row-major query vectors in `space` that take the place
 * of the rows of W (the W_out of mfx_rec_fold_in, session vectors, anything without an id): rel is then the same chain
 * over Wq[q]; users must be NULL and MFX_DIV_NO_EXCLUDE set.
 * Ranges: 1 <= n_top <= 128; every list at most 2048 candidates (one piece of mfx_rec_query_candidates); 0 <= tradeoff
 * <= 1; 1 <= k <= 1024.  form: 0 automatic; 1 and 2 are test hooks that force the two forms of the selection kernel (1: the
 * eligible rows of H staged once in LDS, 2: re-read at every step; the same bits); form 1 where the rows of the batch's
 * longest list do not fit in LDS is MFX_ERR_INVALID.  The call runs mfx_rec_similar_setup if it has not run.
 * Workspace during the call: 8 bytes per candidate, 8 bytes per slot, nusers * kt floats with Wq, and with `space` =
 * MFX_HOST the device copies of the arguments and results.
 * MFX_ERR_INVALID, the handle left usable, the message naming the first offending slot where there is one: anything
 * outside the ranges, an unknown metric, unknown flag bits, a list that is too long, what mfx_rec_query_candidates refuses
 * about pointers and ids, Wq with users or without the flag, form outside 0 .. 2.  nusers == 0 is MFX_OK and touches nothing. */
#define MFX_DIV_NO_EXCLUDE 1   /* do not take the handle's exclusion rows off the lists */
int mfx_rec_diversify(mfx_rec_t r, int64_t nusers, const uint32_t* users, const float* Wq, const uint32_t* cand_ptr,
                      const uint32_t* cand_idx, int32_t flags, int metric, float tradeoff, int32_t n_top, uint32_t* items,
                      float* scores, float* values, uint32_t* n_eligible, mfx_memspace space, int form);
/* Stream seconds of the last mfx_rec_diversify on r by phase: [0] check + stage (copies in, the validity checks and their
 * read-back, mfx_rec_similar_setup when it runs, the packing of Wq), [1] relevance (the kernel that scores every list and
 * compacts its eligible candidates), [2] selection (the kernel of the greedy steps). */
int mfx_rec_diversify_times(mfx_rec_t r, double seconds[3]);
/* Inverted-file (IVF) retrieval, the first stage that mfx_rec_query_candidates is the second stage of: the items are
 * partitioned into nlist lists, each with a centroid; a query scores the user against the centroids, takes the best
 * nprobe lists and ranks only the items of those lists.  The clustering is the caller's (Python: mfx.ivf_kmeans).
 *
 * mfx_rec_ivf_setup builds the index on r.  assign [cols]: the list of every item, each < nlist (checked on the device);
 * centroids [nlist][k], row-major whatever the handle's layout; 1 <= nlist <= 65536; empty lists are allowed.  `space`
 * applies to both arrays, which are copied.  It may be called again: a successful call replaces the index, a refused one
 * leaves the handle as it was.  The index keeps on the device one more copy of H (packed in list order from the handle's
 * own packed H, so the bits are the ones mfx_rec_query scores with; every list padded to a multiple of 32 items, at most
 * 32 * nlist padding items), 8 bytes per item for the position -> item id table and the lists, 8 bytes per list, the
 * packed centroids, and 4 bytes per item while an item filter is set.
 * mfx_rec_ivf_lists returns the lists as built: list_ptr [nlist + 1], list_idx [cols]; list l is
 * list_idx[list_ptr[l] .. list_ptr[l+1]), item ids ascending.
 *
 * mfx_rec_ivf_probe: the lists a query probes, lists [nusers][nprobe], scores [nusers][nprobe] or NULL.  The score of
 * (user u, list l) is the fp32 FMA chain of mfx_rec_query over t = 0 .. k-1 with the centroid in H's place; lists are
 * ranked by score descending, then list id ascending; -0 == +0; a NaN score is never probed; the slots left over hold
 * (0xFFFFFFFF, -INFINITY).  So the result equals mfx_rec_query(n_top = nprobe) on a handle made from the same W with the
 * centroids as its items and no exclusion, bit for bit.
 *
 * mfx_rec_query_ivf: the top n_top of each slot over the items of its probed lists.  items [nusers][n_top], scores
 * [nusers][n_top] or NULL equal mfx_rec_query_candidates for the same users with each slot's candidate list the
 * ascending union of its probed lists: the handle's exclusion rows, the item filter (honoured whether
 * mfx_rec_set_item_filter was called before or after mfx_rec_ivf_setup), the total order, the padding with
 * (0xFFFFFFFF, -INFINITY), the score bits and the NaN rule are those.  In particular nprobe = nlist equals
 * mfx_rec_query bit for bit.  Slot q is user users[q] (q when users is NULL; any order, duplicates allowed); a slot's
 * result does not depend on the batch, its order, the memory space or the factor layout.
 * Ranges: 1 <= nprobe <= min(nlist, 1024) (the probe is a top-N pass), 1 <= n_top <= 1024, nprobe * n_top <= 8192 (the
 * per-probe partial lists go through the merge of mfx_rec_query's item slices).
 * Workspace during a query: 4 * nprobe bytes per slot for the probes, nprobe candidate lists of 8 * L bytes per slot
 * (L = the power of two >= n_top + 32, at least 64; the slots are taken in chunks so that these stay under 1 GiB), and
 * 4 bytes per (slot, probe) pair plus 12 bytes per list for the work items.
 *
 * MFX_ERR_INVALID, the handle left usable: anything outside those ranges, an assign entry >= nlist, a user id >= rows,
 * a NULL array that is needed, a bad memory space, any of mfx_rec_ivf_lists / _probe / mfx_rec_query_ivf before a
 * successful mfx_rec_ivf_setup.  nusers == 0 is MFX_OK and touches nothing.
 * mfx_rec_ivf_times: stream seconds of the last mfx_rec_query_ivf on r: [0] probe, [1] work-item build, [2] list pass,
 * [3] merge (0 for nprobe = 1); zeros before the first one. */
int mfx_rec_ivf_setup(mfx_rec_t r, int32_t nlist, const uint32_t* assign, const float* centroids, mfx_memspace space);
int mfx_rec_ivf_lists(mfx_rec_t r, uint32_t* list_ptr, uint32_t* list_idx, mfx_memspace space);
int mfx_rec_ivf_probe(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t nprobe, uint32_t* lists, float* scores,
                      mfx_memspace space);
int mfx_rec_query_ivf(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t nprobe, int32_t n_top, uint32_t* items,
                      float* scores, mfx_memspace space);
int mfx_rec_ivf_times(mfx_rec_t r, double seconds[4]);
int mfx_rec_destroy(mfx_rec_t r);

/* ------------------------------------------------------------------------------------
 * Single operators (host pointers in, host pointers out): one call per reference
 * function on the path, used by the parity tests.
 * ---------------------------------------------------------------------------------- */
/* RankOneUpdate_v_kernel / _u_kernel (cuda_src/CCD_CUDA.cu:24-58) == the sweep of
 * src/CCD.cpp:110-113: out[c] = sum(vec[idx]*val) / (lambda*|Omega_c| + sum(vec[idx]^2)),
 * 0 for an empty segment.  variant: -1 = the reference's own summation order (sequential fp32, bit-identical to
 * the CPU reference), 0 = wave-per-segment kernel, 1 = flat-stream kernel gathering
 * from L2, 2 = flat-stream kernel with LDS panels (size chosen), >= 16 = LDS panels of `variant`
 * gathered entries, <= -16 = cache panels of `-variant` entries (test hooks: force many panels on
 * small inputs). */
int mfx_rank_one_sweep(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx,
                       const float* val, int64_t vec_len, const float* vec, float lambda,
                       float* out, int variant, int device);
/* UpdateRating_DUAL_kernel_NoLoss, one copy (cuda_src/CCD_CUDA.cu:60-82) ==
 * UpdateRating_Original_float (src/CCD.cpp:18-43): val[p] +=/-= gathered[idx[p]]*per_seg[c]. */
int mfx_update_rating(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx,
                      float* val, int64_t vec_len, const float* gathered, const float* per_seg,
                      int add, int variant, int device);
/* GPU_rmse + host reduction (cuda_src/CUDA_AUX.cu:3-27, CCD_CUDA.cu:383-401) ==
 * calrmse (src/tools.cpp:235-248): fp32 products, fp64 sums. */
int mfx_test_rmse(const mfx_coo* T, const float* W, const float* H, int64_t rows, int64_t cols,
                  int64_t k, int ifALS, double* rmse_out, int device);
/* Mt_byM_multiply_k (cuda_src/ALS_CUDA.cu:65-79): A[k][k] = sum over idx of x x^T (cnt <= 2048: one wavefront's
 * share of a segment; the half-sweep below splits longer segments and adds the pieces in a fixed order). */
int mfx_als_gramian(int64_t cnt, const uint32_t* idx, int64_t nrows_x, const float* X, int64_t k,
                    float* A, int device);
/* inverseMatrix_CholeskyMethod_k (cuda_src/ALS_CUDA.cu:41-62) == choldc1 / choldcsl /
 * inverseMatrix_CholeskyMethod (src/ALS.cpp:6-64) on one k x k matrix, in the reference's operation order
 * (bit-identical to the CPU reference): Ainv = A^-1 via Cholesky, mirrored. */
int mfx_als_inverse(int64_t k, const float* A, float* Ainv, int device);
/* Ainv ~ A^-1 of one symmetric positive definite matrix A [k][k], 1 <= k <= 1024, host pointers, computed on the device by
 * a blocked Cholesky A = L L^T, a blocked L^-1 and L^-T L^-1 on the fp32 matrix cores (the diagonal blocks in fp64): the
 * preconditioner of mfx_ials_cg_create.  Ainv is exactly symmetric and its bits depend on (A, k) alone.  MFX_ERR_INVALID
 * for k outside 1..1024 (without touching the device) and for an A that is not positive definite or not finite. */
int mfx_spd_inverse(int64_t k, const float* A, float* Ainv, int device);
/* One ALS half-sweep, updateW_overH_kernel / updateH_overW_kernel
 * (cuda_src/ALS_CUDA.cu:81-181): for every segment solve (X^T X + lambda I) y = X^T r.
 * variant 1 (default path): MFMA Gramian, Cholesky factorisation and two triangular solves; variant 0:
 * "as written" -- Gramian, explicit inverse and products in the reference's own operation order
 * (src/ALS.cpp:66-79, 6-64, 129-142), bit-identical to the CPU reference; the parity mode, also selected by
 * mfx_params.schedule = 0 in mfx_als_run / mfx_als_create. */
int mfx_als_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx,
                 const float* val, int64_t nrows_x, const float* X, float* Y, int64_t k,
                 float lambda, int variant, int device);

/* ------------------------------------------------------------------------------------
 * Communicator over RCCL (the reference has no distributed code).
 * One process per GPU: rank 0 calls mfx_comm_unique_id, ships the 128 bytes to the other
 * ranks by any means (bench.py uses torch.distributed), every rank calls mfx_comm_create.
 * ---------------------------------------------------------------------------------- */
#define MFX_COMM_ID_BYTES 128
int mfx_comm_unique_id(void* id_out /* MFX_COMM_ID_BYTES */);
int mfx_comm_create(mfx_comm_t* out, const void* id, int rank, int nranks, int device);
/* In-process loopback communicator: the `nranks` ranks of `group` are threads of ONE process (each
 * driving its own solver, on the same or on different devices); collectives are staged through
 * host memory and summed in rank order.  Slow by design -- it exists to run the sharded solver path
 * through the real kernels where RCCL cannot (two ranks on one GPU); production uses mfx_comm_create. */
int mfx_comm_create_local(mfx_comm_t* out, int group, int rank, int nranks, int device);
/* Collective over all ranks: *global_status = the worst (most negative) local_status.  Protocol for a
 * sharded solve: every rank runs its own setup (extract its shard, mfx_ccd_create / mfx_als_create_sharded,
 * set factors), then ALL ranks -- the ones whose setup failed too, with their error code -- call this once;
 * only if *global_status == MFX_OK does anyone go on to iterate.  No solver entry point runs a collective
 * before its first iterate call, so a failed rank can never leave the others waiting inside one.  (On RCCL
 * this is also where the lazy connection setup is paid.) */
int mfx_comm_agree(mfx_comm_t c, int local_status, int* global_status);
/* For a rank that fails AFTER the collectives started: releases the ranks waiting for it (loopback group:
 * every present and future collective returns MFX_ERR_COMM; RCCL: ncclCommAbort on every communicator of the
 * same unique id in this process).  The communicator can only be destroyed afterwards. */
int mfx_comm_abort(mfx_comm_t c);
int mfx_comm_rank(mfx_comm_t c);
int mfx_comm_size(mfx_comm_t c);
int mfx_comm_destroy(mfx_comm_t c);

/* ------------------------------------------------------------------------------------
 * Host-side helpers on the path (no GPU needed).
 * ---------------------------------------------------------------------------------- */
/* initial_col (src/tools.cpp:165-173): X flat [k][n], srand(0) then glibc rand() consumed
 * with i (0..n) outer and j (0..k) inner: X[j*n+i] = 0.1f*(float(rand())/RAND_MAX)+0.001f.
 * CCD++ calls it as (W, k, rows)/(H, k, cols); ALS as (W, rows, k)/(H, cols, k)
 * (src/main.cpp:86-98). */
void mfx_initial_col(float* X, int64_t k, int64_t n);
/* nnz-balanced contiguous row-block partition: bounds[g] .. bounds[g+1] are shard g's rows
 * (prefix sums of csr_row_ptr, SURVEY.md 8e "Partition").  bounds has nshards+1 entries. */
int mfx_partition_rows(int64_t rows, const uint32_t* csr_row_ptr, int nshards, int64_t* bounds);
/* Extracts shard [row_lo,row_hi) of R into caller-allocated arrays: local CSR (row_ptr
 * rebased to 0) and local CSC over local row ids (entries keep R's per-column order).
 * local_nnz = csr_row_ptr[row_hi]-csr_row_ptr[row_lo] sizes the idx/val arrays. */
int mfx_extract_shard(const mfx_csx* R, int64_t row_lo, int64_t row_hi, uint32_t* l_csr_row_ptr,
                      uint32_t* l_csr_col_idx, float* l_csr_val, uint32_t* l_csc_col_ptr,
                      uint32_t* l_csc_row_idx, float* l_csc_val);
/* Ranking metrics of top-N lists (host pointers) against a test set.  For listed user u, R_u = the
 * distinct test items of u with value >= min_rating (-INFINITY: all); users with an empty R_u are
 * skipped and *users_evaluated (may be NULL) is the number kept.  Padding items (0xFFFFFFFF) never
 * count; a repeated item counts once.  out = {HR, precision, recall, NDCG}, means over the kept
 * users of [hits > 0], hits / n_top, hits / |R_u| and DCG / IDCG with gain 1 / log2(rank + 2)
 * (rank 0-based, IDCG over min(n_top, |R_u|) ranks); fp64 throughout. */
int mfx_topn_metrics(int64_t nusers, const uint32_t* users, int32_t n_top, const uint32_t* items,
                     const mfx_coo* T, float min_rating, double out[4], int64_t* users_evaluated);

#ifdef __cplusplus
}
#endif
#endif /* MFX_H */
