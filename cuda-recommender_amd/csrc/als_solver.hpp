// als_solver.hpp -- resident ALS solver (replaces als_NV, cuda_src/ALS_CUDA.cu:200-406).
//
// Per half-sweep and per segment (user row / item column): A = sum x x^T + lambda I on the fp32
// matrix cores (v_mfma_f32_32x32x2_f32, exact fp32), b = sum r x, Cholesky A = L L^T in LDS and two
// triangular solves.  No device-side malloc, no per-thread k^2 scratch (the reference's
// updateW_overH_kernel does both, ALS_CUDA.cu:93-94).
#pragma once

#include <vector>

#include "comm.hpp"
#include "common.hpp"

namespace mfx {

struct AlsItem {      // one wavefront's work: entries [lo, hi) of segment `seg`
    uint32_t seg, lo, hi;
    int32_t slot;     // < 0: the whole segment, solve in place; >= 0: partial Gramian slot
};
struct AlsReduce {    // a segment whose Gramian was split over `nslots` consecutive slots
    uint32_t seg, slot0, nslots;
};

constexpr uint32_t kAlsChunk = 2048;  // gathered rows per wavefront before a segment is split (AlsHalf::build's `chunk`)
constexpr uint32_t kAlsEntryPad = 128;  // entries behind AlsHalf::idx / val that the Gramian kernels may read (and ignore)
constexpr uint32_t kPhaseCopies = 1024;  // MFX_ALS_PHASES=1: copies of the eight phase counters, one per blockIdx.x % kPhaseCopies

// One orientation (rows over H, or columns over W).
struct AlsHalf {
    uint32_t nseg = 0;
    uint64_t nnz = 0;
    DevBuf<uint32_t> ptr, idx;
    DevBuf<float> val;
    DevBuf<AlsItem> items;
    DevBuf<AlsReduce> reduces;
    uint32_t nitems = 0, nreduces = 0, nslots = 0;
    // G = number of factor rows the indices address: every idx must be < G (checked on the device)
    int build(uint32_t nseg, uint64_t nnz, uint32_t G, const uint32_t* ptr, const uint32_t* idx, const float* val,
              mfx_memspace space, uint32_t chunk, hipStream_t st);
};

// Implicit ALS by block subspace sweeps (ials_block.hip): what one half-sweep at rank k <= 1024 with blocks of d <= 128
// coordinates keeps on the device besides the factors.  One set serves both orientations.
struct IalsBlock {
    uint32_t k = 0, d = 0;
    DevBuf<float> G, gpart;  // base Gramian [k][k] of the fixed side, its per-partition tile partials
    DevBuf<float> Xb;        // the fixed side block-major: block b is [rows + 1][width of b], the last row all zeros
    DevBuf<float> Gbb;       // the diagonal blocks of G, block b contiguous [width][width] at b d d
    DevBuf<float> P, Z;      // [nseg][width]: G[block, :] y and the step of the current block
    DevBuf<float> score;     // [nnz + kAlsEntryPad]: <x_j, y> of every stored pair in the orientation of the half
    DevBuf<float> ws;        // partial slots of split segments (als_ws_floats at rank d)
    int alloc(uint32_t k, uint32_t d, uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st);
    // P, Z, score and ws alone, for another set of segments over the same fixed side (fold-in: once per query)
    int alloc_half(uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st);
    // explicit ALS by block sweeps (alsb_*): Xb and the per-half part, no G, gpart, Gbb
    int alloc_explicit(uint32_t k, uint32_t d, uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st);
    // G and gpart alone, for ialsb_gramian over up to max_rows_x rows (implicit ALS by conjugate gradients)
    int alloc_gramian(uint32_t k, uint32_t max_rows_x);
};
constexpr uint32_t kIalsBlockMaxRank = 1024, kIalsBlockMaxBlock = 128;
inline uint32_t ialsb_default_block(uint32_t k) { return k < 64 ? k : 64; }  // mfx_ials_block_create, block = 0
// G = X^T X + lambda I into b.G, any k <= 1024 (32 x 32 MFMA tiles over row partitions, summed in partition order)
int ialsb_gramian(IalsBlock& b, const float* X, uint32_t rows, float lambda, hipStream_t st);
// One half-sweep in place on Y [h.nseg][k] (the warm start) over X [x_rows][k] with b.G = X^T X + lambda I: the packing
// (ialsb_pack_launch: X block-major into b.Xb, the diagonal blocks of b.G into b.Gbb), then the sweep (ialsb_sweep_launch:
// the scores, then for every block in ascending order G[block, :] y, the block systems (k_ialsb_*: ialsb_step_launch) and
// the update of y and of the scores)
int ialsb_pack_launch(IalsBlock& b, const float* X, uint32_t x_rows, hipStream_t st);
// rho != NULL (mfx_ials_block_create_reg): b.G holds G0 = fp32(alpha0 X^T X) (ialsrb_gramian), rho [h.nseg] the regulariser of
// every segment (ialsr_rho_launch); P gets fmaf(rho, y_block, .) on top of Y G0[:, block] and the systems are the k_ialsrb_* ones
int ialsb_sweep_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, uint32_t* spd_fail,
                       hipStream_t st, float alpha0 = 1.f, const float* rho = nullptr);
int ialsb_half_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, uint32_t* spd_fail,
                      hipStream_t st, float alpha0 = 1.f, const float* rho = nullptr);
// Fold-in: up to `sweeps` sweeps in place on Y over a side packed before (ialsb_pack_launch).  An empty row is zero and counts
// 0 sweeps.  tol = 0: every other row gets `sweeps`, nothing is read back.  tol > 0: after each sweep a row is frozen once
// max |y_new - y_old| <= tol max |y_new| (its bits never change again), and the host reads the number of rows still moving
// to stop early.  counts: device [h.nseg] (sweeps applied to each row) or NULL.
int ialsb_fold_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, int32_t sweeps, float tol,
                      int32_t* counts, uint32_t* spd_fail, hipStream_t st, float alpha0 = 1.f, const float* rho = nullptr);
// ials_block_step.hip (als_solver.hip as the k_ialsb_* family): the systems of one block, Z [nseg][d] = the steps
int ialsb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, const float* Gbb, float alpha,
                      const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st);

// Implicit ALS with an unobserved weight alpha0 and a regulariser per segment rho_s = fp32(lambda (n_s + alpha0 N)^nu), n_s the
// segment's entries with r > 0 and N the rows of the fixed side (mfx_ials_create_reg, mfx_ials_block_create_reg).
// MFX_ERR_INVALID naming "alpha0", "nu" or "regulariser"; touches no device
int ialsr_check_params(const char* fn, float lambda, float alpha0, float nu, int64_t rows, int64_t cols);
// rho [h.nseg] of the segments of h over a fixed side of N rows (ials.hip; fp64 on the device)
int ialsr_rho_launch(const AlsHalf& h, uint32_t N, float lambda, float alpha0, float nu, float* rho, hipStream_t st);
// G[i] = fp32(alpha0 G[i]) over n floats; G0 = fp32(alpha0 X^T X) for k <= 128 (ials_base_gramian with lambda = 0, then the
// scale) and for any k <= 1024 into b.G (ialsb_gramian likewise)
int ialsr_scale_launch(float* G, size_t n, float alpha0, hipStream_t st);
int ialsr_base_gramian(const float* X, uint32_t rows, uint32_t k, float alpha0, float* part, float* G0, hipStream_t st);
int ialsrb_gramian(IalsBlock& b, const float* X, uint32_t rows, float alpha0, hipStream_t st);
// ials_reg_half.hip (als_solver.hip as the k_ialsr_* family): the half-sweep, k <= 128
int ialsr_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const float* G0, float alpha, float alpha0,
                      const float* rho, float* ws, uint32_t* spd_fail, hipStream_t st);
// ials_reg_block_step.hip (the k_ialsrb_* family): the systems of one block
int ialsrb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, const float* Gbb, float alpha, float alpha0,
                       const float* rho, const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st);
// the objective of these handles (generalises ials_loss_launch; nu = 0 takes the regulariser from the Gramians' traces)
size_t ialsr_loss_ws_doubles(uint32_t k);
int ialsr_loss_launch(const AlsHalf& rows, const float* W, uint32_t m, const float* H, uint32_t n, uint32_t k, float lambda, float alpha,
                      float alpha0, float nu, const float* rho_rows, const float* rho_cols, double* ws, double* out, hipStream_t st);

// Explicit ALS by block subspace sweeps (mfx_als_block_create; the explicit part of ials_block.hip): the objective
// sum_j (r_j - <x_j, y>)^2 + rho |y|^2 of a segment, rho = lambda (reg 0) or fp32(lambda * n) for n stored entries (reg 1),
// minimised block by block from the segment's current row.  No base Gramian: b.G, b.gpart, b.Gbb stay empty
// (IalsBlock::alloc_explicit).  The same three launches as above: the packing (X block-major), one sweep in place on Y (the
// scores, then for every block P = rho y_block, the block systems (k_alsb_*: alsb_step_launch) and the update), and both.
int alsb_pack_launch(IalsBlock& b, const float* X, uint32_t x_rows, hipStream_t st);
int alsb_sweep_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg,
                      uint32_t* spd_fail, hipStream_t st);
int alsb_half_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg,
                     uint32_t* spd_fail, hipStream_t st);
// Fold-in with the stop rule of ialsb_fold_launch, over a side packed before (alsb_pack_launch)
int alsb_fold_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg, int32_t sweeps,
                     float tol, int32_t* counts, uint32_t* spd_fail, hipStream_t st);
// als_block_step.hip (als_solver.hip as the k_alsb_* family): the systems of one block, Z [nseg][d] = the steps;
// P [nseg][d] = rho y_block
int alsb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, float lambda, int32_t reg,
                     const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st);
// MFX_ERR_INVALID unless every value is finite (device-side check)
int als_check_finite(const float* d_val, uint64_t n, const char* what, hipStream_t st);

// Fold-in by preconditioned conjugate gradients (rec_foldin_cg.hip; mfx_rec_fold_in_cg_setup): every row's system
// is the fixed base plus a matrix of the rank of the row, so CG preconditioned by the inverse of the base ends after n + 1 steps
// on a row of n entries.  reg 0: the implicit objective, A = G + sum_e w_e h_e h_e^T with G = H^T H + lambda I as ialsb_gramian
// builds it and Minv a symmetric fp32 approximation of G^-1 (both [k][k], device); reg 1 / 2: the explicit objective with
// rho = lambda / fp32(lambda * n) for a row of n entries, no G, the identity as preconditioner.
struct FoldCg {
    int32_t reg = 0;
    float lambda = 0.f, alpha = 0.f;
    const float* G = nullptr;
    const float* Minv = nullptr;
    int32_t steps = 1;  // the most steps a row gets
    float tol = 0.f;    // > 0: a row is frozen once |b - A y| <= tol |b| (2-norms, fp32), tested on the start row too
};
// Minv [k][k] (host) from G [k][k] (host, symmetric): Cholesky and inverse in fp64 in a fixed loop order, rounded to fp32, the
// upper triangle mirrored.  MFX_ERR_INVALID when G is not positive definite.
int foldcg_inverse(const float* G, uint32_t k, float* Minv);
// Up to m.steps steps in place on Y [h.nseg][k] over X [x_rows + 1][k] (last row zeros).  warm: Y holds the start rows, else
// Y must be zero.  A row without entries or with b = 0 is zero and counts 0 steps.  tol = 0: nothing is read back; tol > 0: the
// host reads one counter per step and stops when every row is frozen.  counts: device [h.nseg] (steps applied) or NULL.
// *fail counts the rows that met <p, A p> < 0 or a non-finite one (they come back as NaN).
// ws: NULL = the call allocates its vectors and frees them; else a caller-owned set (FoldCgWs::alloc) large enough for h, k
// and m.steps, reused from call to call.  frozen of ws then tells afterwards which rows met the stop rule.
struct FoldCgWs {
    DevBuf<float> R, Z, P, Q;    // [max_seg][k] each: 16 k bytes per row
    DevBuf<float> part, bb, gamma;
    DevBuf<uint32_t> frozen, active;
    int alloc(uint32_t max_seg, uint32_t k, uint32_t nslots, int32_t steps);
};
int foldcg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, const FoldCg& m, float* Y, bool warm, int32_t* counts,
                  uint32_t* fail, hipStream_t st, FoldCgWs* ws = nullptr);

// Device inverse of one symmetric positive definite matrix (spd_inverse.hip; mfx_spd_inverse): Minv [k][k] ~ G^-1
// for G [k][k], both fp32 on the device, 1 <= k <= 1024, by a blocked Cholesky G = L L^T, a blocked L^-1 and Minv = L^-T L^-1
// on 32 x 32 MFMA tiles (the diagonal blocks in fp64 in LDS).  G is not modified; Minv is exactly symmetric and its bits depend
// on (G, k) alone.  ws: spd_inverse_ws_floats(k) floats.  Stream-ordered launches only; nothing is read back.  A pivot <= 0 or
// not finite counts into *fail (device) and the stages still run to their end: Minv is then unspecified.
size_t spd_inverse_ws_floats(uint32_t k);
int spd_inverse_launch(const float* G, uint32_t k, float* Minv, float* ws, uint32_t* fail, hipStream_t st);
int spd_inverse_op(int64_t k, const float* A, float* Ainv, int device);  // host pointers; MFX_ERR_INVALID when A is not positive definite

// Implicit ALS by preconditioned conjugate gradients (ials_cg.hip; mfx_ials_cg_create): what a half-sweep at rank
// k <= 1024 keeps on the device besides the factors.  One set serves both orientations.  The four CG vectors are allocated
// once for the larger side: 16 k bytes per row of it on top of the factors.
struct IalsCg {
    uint32_t k = 0;
    IalsBlock gb;                 // G and its partials alone (IalsBlock::alloc_gramian)
    DevBuf<float> Minv, inv_ws;   // [k][k] ~ G^-1, the workspace of spd_inverse_launch
    FoldCgWs ws;
    DevBuf<int32_t> counts;       // [max_seg]: steps applied to every row of the last half
    int alloc(uint32_t k, uint32_t max_rows_x, uint32_t max_seg, uint32_t nslots, int32_t steps);
};
// One half in place on Y [h.nseg][k] over X [x_rows + 1][k] (last row zeros): G = ialsb_gramian(X, lambda), Minv =
// spd_inverse_launch(G), foldcg_launch from Y (warm) or from zero (Y must be zero).  fails: device [2], the inverse's pivots and
// the rows that failed, added to; stats: device [3], set to the row-steps applied, the most steps of a row and the rows that
// used all `steps` without meeting tol (0 when tol = 0).  ev_gram / ev_inv (or NULL): recorded after the Gramian / the inverse.
int ialscg_half_launch(IalsCg& c, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, bool warm, float lambda, float alpha,
                       int32_t steps, float tol, uint32_t* fails, unsigned long long* stats, hipEvent_t ev_gram, hipEvent_t ev_inv,
                       hipStream_t st);

// What a trainer is: how a half-sweep solves its segments, on which objective, with which parameters, and the device state
// built for that pair (FoldPlan of recommend.hpp is the same thing for fold-in).  The pairs that exist are the rows of
// kAlsPairs (als_host.hip); als_plan_half is the one place that knows which launches make a half-sweep of each.
struct AlsSpec;
struct AlsPair;
struct AlsPlan {
    // Direct: one closed-form solve per segment at k <= 128 by the MFMA half-sweep families; DirectExact: the same system in
    // the reference's order of operations (schedule 0, variant 0); Blocks: block subspace sweeps; Cg: conjugate gradients
    enum class Method { Direct, DirectExact, Blocks, Cg };
    // what goes on the diagonal: Als lambda, Ccd fp32(lambda * entries of the segment), Implicit the base Gramian's lambda,
    // ImplicitReg fp32(lambda (n + alpha0 N)^nu) per segment, with alpha0 the weight of the unobserved pairs
    enum class Objective { Als, Ccd, Implicit, ImplicitReg };
    Method method = Method::Direct;
    Objective objective = Objective::Als;
    const AlsPair* pair = nullptr;  // the row of kAlsPairs
    uint32_t k = 0;
    float lambda = 0.f, alpha = 0.f, alpha0 = 1.f, nu = 0.f;  // alpha: 0 on an explicit objective
    uint32_t block = 0;  // Blocks: the width used, min(k, the width asked for or ialsb_default_block(k))
    int32_t cap = 0;     // Cg: the most steps a row gets in one half
    float tol = 0.f;
    DevBuf<float> ws;                  // Direct: partial slots of split segments (als_ws_floats at rank k)
    DevBuf<float> G, gpart;            // Direct, implicit: base Gramian [k][k] of the fixed side, its per-partition partials
    IalsBlock bs;                      // Blocks
    IalsCg cgs;                        // Cg
    DevBuf<uint32_t> cg_fail;          // Cg [4]: inverse pivots and failed rows of the W-half, of the H-half
    DevBuf<unsigned long long> cg_cnt; // Cg [6]: the three counts of ialscg_half_launch, W-half then H-half
    DevBuf<float> rho_rows, rho_cols;  // ImplicitReg [rows], [cols]: formed once, the pattern of R is fixed (a one-shot: rho_rows)
    DevBuf<double> loss_ws;            // implicit: fp64 Gramians + entry partials of the objective

    bool implicit() const { return objective == Objective::Implicit || objective == Objective::ImplicitReg; }
    bool direct() const { return method == Method::Direct || method == Method::DirectExact; }
    bool has_base_gramian() const { return implicit(); }  // a half-sweep starts with the Gramian of the fixed side (ev_gram)
    bool has_inverse() const { return method == Method::Cg; }  // ... and inverts it (ev_inv)
    bool warm_start() const { return method == Method::Blocks || method == Method::Cg; }  // a half-sweep starts from Y's rows
    size_t loss_ws_doubles() const;
    // the parameters of a checked spec (als_spec_check) at rank k; touches no device
    int set(const AlsSpec& s, uint32_t k, float lambda);
    // the buffers of the pair for halves of up to max_seg segments, nnz entries and nslots partial slots over up to max_rows_x
    // fixed rows (rho_*, loss_ws: by the caller)
    int alloc(uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st);
    // the values a half may hold: implicit finite, >= 0 and alpha * value finite; Blocks on an explicit objective finite
    int check_values(const AlsHalf& h, const char* what, hipStream_t st) const;
};

// What an entry point asks for: the pair, the parameters as the caller gave them and the entry point's name for the texts.
struct AlsSpec {
    AlsPlan::Method method;
    AlsPlan::Objective objective;
    const char* fn;
    bool half = false;  // a single-half entry point (rows = segments, cols = fixed rows), not a create
    float alpha = 0.f, alpha0 = 1.f, nu = 0.f;
    int32_t block = 0, reg = 0, cap = 1;  // block: the width asked for (Blocks), 0 = chosen from k; reg: of the explicit Blocks
    float tol = 0.f;
    int32_t schedule = 1;              // a create: mfx_params::schedule and the memory space, filled in by AlsSolver::create
    mfx_memspace space = MFX_HOST;
};
// MFX_ERR_INVALID with the entry point's own text for the first thing wrong, in the entry point's own order; touches no device
int als_spec_check(const AlsSpec& s, int64_t k, float lambda, int64_t rows, int64_t cols, int64_t nnz);

// One half-sweep of a plan: Y [h.nseg][k] over the fixed X [x_rows + 1][k] (last row zeros; Blocks: [x_rows][k] will do).
// warm (Cg): Y holds the start rows, else Y must be zero.  rho (ImplicitReg): the regulariser of h's segments.  ev_gram /
// ev_inv (or NULL): recorded after the base Gramian / its inverse, where the plan has one.  fails: device, the failed systems
// are added to it ([1]; Cg [2]: the inverse's pivots and the failed rows); stats: Cg, device [3] (ialscg_half_launch).
int als_plan_half(AlsPlan& pl, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, bool warm, const float* rho, hipEvent_t ev_gram,
                  hipEvent_t ev_inv, uint32_t* fails, unsigned long long* stats, hipStream_t st, unsigned long long* phases = nullptr);

class AlsSolver {
public:
    // every mfx_*_create of an ALS trainer: checks the spec, then builds the solver and the plan of the pair
    static int create(AlsSolver** out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space, const mfx_als_shard* shard,
                      const AlsSpec& spec);
    // the last iteration of a Cg handle, W-half then H-half: row-steps, most steps of a row, rows out of steps, failed rows
    int cg_stats(int64_t out[8]);
    int loss(double* out);  // implicit only: the objective at the current factors (ials.hip)
    ~AlsSolver();
    int set_factors(const float* W, const float* H, mfx_memspace space);
    int iterate(int n_iter, int with_rmse, mfx_iter_report* reports);
    int get_factors(float* W, float* H, mfx_memspace space);
    int kernel_times(int cap, const char** names, double* seconds, int64_t* launches);

private:
    AlsSolver() = default;
    int init(const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space, const mfx_als_shard* shard, const AlsSpec& spec);
    int exchange(float* X, const std::vector<int64_t>& bounds);  // every rank broadcasts its block of X (one grouped call)
    int meet_shards();  // first iterate() of a sharded solve: gathers everyone's block boundaries (never in create)
    // One half-sweep of iterate(), half 0: W (this rank's rows from row_lo_ on) over H, half 1: H over W
    int half_sweep(int half);
    int device_ = 0;
    hipStream_t st_ = nullptr;
    mfx_params p_{};
    uint32_t m_ = 0, n_ = 0, k_ = 0;
    // sharded solve: this rank's row / column block and everyone's block boundaries
    mfx_comm_s* comm_ = nullptr;
    uint32_t row_lo_ = 0, col_lo_ = 0, row_hi_ = 0, col_hi_ = 0;
    std::vector<int64_t> row_bounds_, col_bounds_;
    bool shards_met_ = false;  // both boundary vectors gathered AND validated (meet_shards)
    int64_t global_test_nnz_ = 0;
    AlsHalf rows_, cols_;
    DevBuf<float> W_, H_;
    AlsPlan plan_;
    DevBuf<uint32_t> spd_fail_;
    DevBuf<unsigned long long> phases_;  // MFX_ALS_PHASES=1: per-phase clocks of the half-sweep kernels (diagnostic)
    int print_phases(const char* what);
    int64_t nnz_test_ = 0;
    DevBuf<uint32_t> t_row_, t_col_;
    DevBuf<float> t_val_;
    DevBuf<double> rmse_partials_, rmse_sum_;
    int64_t iter_ = 0;
    double update_acc_ = 0;
    bool factors_set_ = false;
    hipEvent_t ev_[8] = {};
    // [0], [1]: the two half-sweeps; with a base Gramian: [2], [3] those of H and W; with an inverse: [4], [5] those
    double t_half_[6] = {0, 0, 0, 0, 0, 0};
    int64_t n_half_[6] = {0, 0, 0, 0, 0, 0};
    DevBuf<double> loss_;   // implicit: the objective
    bool w_cold_ = false;   // Cg: set_factors got no W, the next W-half starts from zero
    int64_t cg_stats_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool cg_stats_set_ = false;
};

// Launches one half-sweep: Y[seg] = argmin over segment `seg` given factor rows X[x_rows + 1][k],
// whose last row must be all zeros.
int als_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, float lambda, float* ws,
                    uint32_t* spd_fail, hipStream_t st, unsigned long long* phases = nullptr);
// The same with fp32(lambda * n) on the diagonal of a segment of n entries (k_alsn_*, als_nreg.hip): the exact minimiser of the
// CCD++ objective over one segment, X fixed
int als_half_nreg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, float lambda, float* ws,
                         uint32_t* spd_fail, hipStream_t st);
// Implicit half-sweep (k_ials_*): G = the base Gramian X^T X + lambda I of all x_rows rows (ials_base_gramian)
int ials_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const float* G, float alpha,
                     float* ws, uint32_t* spd_fail, hipStream_t st);
// ials.hip: G = X^T X + lambda I over X [rows][k] (MFMA partials `part`, summed in a fixed order)
uint32_t ials_base_parts(uint32_t rows);
size_t ials_base_ws_floats(uint32_t rows, uint32_t k);
int ials_base_gramian(const float* X, uint32_t rows, uint32_t k, float lambda, float* part, float* G, hipStream_t st);
// MFX_ERR_INVALID unless every value is finite, >= 0 and alpha * value is finite (device-side check)
int ials_check_values(const float* d_val, uint64_t n, float alpha, const char* what, hipStream_t st);
// the implicit objective over the training rows (CSR orientation) into *out (device, fp64)
size_t ials_loss_ws_doubles(uint32_t k);
int ials_loss_launch(const AlsHalf& rows, const float* W, uint32_t m, const float* H, uint32_t n, uint32_t k, float lambda, float alpha,
                     double* ws, double* out, hipStream_t st);
// floats of workspace needed for `nslots` partial slots at rank k
size_t als_ws_floats(uint32_t nslots, uint32_t k);

// The half-sweeps with more right-hand sides (als_mrhs.hip, als_nreg_mrhs.hip, ials_half_mrhs.hip, ials_reg_half_mrhs.hip:
// the k_alsm_*, k_alsnm_*, k_ialsm_*, k_ialsrm_* families of als_solver.hip): Y as the family without computes it, bit for bit,
// and Z[seg][t] = A_seg^-1 X[targets[seg][t]] by the same factor and the same substitution code.  A target >= x_rows (the
// padding id 0xFFFFFFFF) reads the zero row; the caller zeroes Z (an empty segment writes none of it) and checks the ids.
struct AlsMrhs {
    const uint32_t* targets = nullptr;  // [nseg][n_targets]
    uint32_t n_targets = 0;
    float* Z = nullptr;                 // [nseg][n_targets][k]
    float lambda = 0.f;                 // als_half_mrhs_launch, als_half_nreg_mrhs_launch
    float alpha = 0.f;                  // the implicit two: as ials_half_launch / ialsr_half_launch take them
    const float* G = nullptr;
    float alpha0 = 1.f;                 // ialsr_half_mrhs_launch
    const float* rho = nullptr;
};
int als_half_mrhs_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const AlsMrhs& m, float* ws,
                         uint32_t* spd_fail, hipStream_t st);
int als_half_nreg_mrhs_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const AlsMrhs& m, float* ws,
                              uint32_t* spd_fail, hipStream_t st);
int ials_half_mrhs_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const AlsMrhs& m, float* ws,
                          uint32_t* spd_fail, hipStream_t st);
int ialsr_half_mrhs_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const AlsMrhs& m, float* ws,
                           uint32_t* spd_fail, hipStream_t st);

// The half-sweep "as written" (als_exact.hip): the reference's arithmetic in its order, bit for bit.
int als_half_exact_launch(const AlsHalf& h, const float* X, float* Y, uint32_t k, float lambda, uint32_t* spd_fail, hipStream_t st);
// inverseMatrix_CholeskyMethod on one k x k matrix (host pointers), same arithmetic
int als_inverse_op(int64_t k, const float* A, float* Ainv, int device);

// The k x k Gramian (no lambda) of ONE unsplit item over `cnt` gathered rows into A (device); val, Y: the item's (unused)
// ratings and solution row
int als_gramian_launch(const AlsItem* item, const uint32_t* idx, const float* val, uint32_t cnt, const float* X, uint32_t x_rows, float* Y,
                       uint32_t k, uint32_t* spd_fail, float* A, hipStream_t st);

// ---- One-shot entry points (host pointers in and out; als_host.hip) ----------------------------------------------------
struct OpStream {  // a stream of the call's own, drained and destroyed on every way out
    hipStream_t st = nullptr;
    ~OpStream() { if (st) { (void) hipStreamSynchronize(st); (void) hipStreamDestroy(st); } }
};
// What the one-shot half-sweeps share: the stream, the segments as an AlsHalf, X and Y on the device, the failure counter.
struct HalfOp {
    OpStream os;
    AlsHalf h;
    DevBuf<float> X, Y;
    DevBuf<uint32_t> fail_cnt;
    // selects the device, creates the stream, builds h over nrows_x factor rows
    int open(int device, int64_t nseg, int64_t nnz, int64_t nrows_x, const uint32_t* ptr, const uint32_t* idx, const float* val);
    // X [nrows_x][k] (zero_row: with the all-zero row nrows_x behind it), Y [nseg][k] = Y_in or zeros, fail_cnt = 0
    int upload(const float* X_in, int64_t nrows_x, int64_t k, bool zero_row, const float* Y_in);
    int download(float* Y_out);  // Y to the host, after everything queued on the stream
};

int als_gramian_op(int64_t cnt, const uint32_t* idx, int64_t nrows_x, const float* X, int64_t k, float* A,
                   int device);
// The segments of a single-half entry point as the caller gave them
struct HalfSegs {
    int64_t nseg, nnz;
    const uint32_t* ptr;
    const uint32_t* idx;
    const float* val;
    int64_t nrows_x;
};
// One half-sweep of the pair of a checked spec, by als_plan_half over buffers that AlsPlan::alloc sized to this half: every
// mfx_*_half.  Y_in: the start rows (Blocks, Cg) or NULL; counts (Cg): host [nseg], the steps applied to each row, or NULL
int als_plan_half_op(const AlsSpec& spec, const HalfSegs& g, const float* X, const float* Y_in, float* Y_out, int64_t k, float lambda,
                     int32_t* counts, int device);

}  // namespace mfx

struct mfx_als_s {
    mfx::AlsSolver* impl;
};
