// bpr.hpp -- the host interface of BPR training (bpr.hip: mfx_bpr_*).  The contract is in include/mfx.h, DESIGN 5.15 has the
// choice of the accumulation and the measurements, DESIGN 5.17 the trials (bpr_neg.hip: hardest-of-M and WARP negative
// sampling).  No device code here: api.hip includes this file.
#pragma once

#include "common.hpp"

namespace mfx {

// The device state of one step on given triples: the factors, the 64-bit fixed-point accumulators beside them, the claim
// and count words of every row and the slot arrays.  The solver owns one for its life, mfx_bpr_apply one for its call.
class BprCore {
public:
    ~BprCore();
    int init(int64_t rows, int64_t cols, int64_t k, int64_t batch, int device);
    int upload(const float* W, const float* H, mfx_memspace space);
    int download(float* W, float* H, mfx_memspace space);
    // One step over the n slots that sit in u_, i_, j_, skip_ (device); the four counts are ADDED to stats_ (device).
    // With neg_mode_ = MFX_BPR_NEG_WARP the gradient kernel is left out: trials() has written g_ and state_ already.
    int step(uint32_t n, float lr, float lambda);
    // The two halves of step: k_bpr_grad and k_bpr_scatter on the factors in W_ and H_, then k_bpr_apply.  lgcn.hip runs the
    // first half on its final embeddings and applies the sums itself.
    int grad_scatter(uint32_t n);
    int apply(uint32_t n, float lr, float lambda);
    // k_bpr_sample: the slots base .. base + n - 1 of the stream s0 over the matrix (ptr, idx) into u_, i_, j_, skip_.
    int sample(uint64_t s0, uint64_t base, uint32_t n, const uint32_t* ptr, const uint32_t* idx, uint32_t nnz);
    // The caller's n host slots into u_, i_, j_, skip_ (skipped = NULL: none), ids checked on the device under the name fn.
    int set_slots(const char* fn, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j, const uint8_t* skipped);
    // bpr_neg.hip.  init_neg after init: the mode, the number of trials M, the rank weights (WARP; NULL = the default table).
    // trials: k_bpr_trials over the n slots whose u_ and i_ are set.  Trial items from `items` [n][M] with `member` [n][M]
    // (NULL: none), or, with items = NULL, from the stream s1 at the slot numbers base + t over the matrix (ptr, idx) with
    // trial 1 = j_ / skip_ as k_bpr_sample left them.  Writes j_, t_ and skip_ (HARDEST) or g_ and state_ (WARP) and ADDS
    // to stats_ (WARP) and tstats_.
    int init_neg(int mode, int negatives, const float* rank_weight);
    int trials(uint32_t n, const uint32_t* items, const uint8_t* member, uint64_t s1, uint64_t base, const uint32_t* ptr, const uint32_t* idx);

    int64_t rows_ = 0, cols_ = 0, k_ = 0, batch_ = 0;
    int device_ = 0, gs_ = 64;  // gs_: lanes that share one row in the scatter and apply kernels (a power of two >= min(k, 64))
    hipStream_t st_ = nullptr;
    DevBuf<float> W_, H_, g_;
    DevBuf<unsigned long long> accW_, accH_, stats_;
    DevBuf<uint32_t> cntW_, cntH_, claimW_, claimH_, u_, i_, j_;
    DevBuf<uint8_t> skip_, state_;
    int neg_mode_ = 0, negatives_ = 1, group_ = 1;  // group_: lanes that share one slot in k_bpr_trials (a power of two <= 64)
    DevBuf<uint32_t> t_;                            // [batch] the chosen trial, 0 = none (neg_mode_ != 0 only)
    DevBuf<float> rw_;                              // [negatives] the rank weights (WARP only)
    DevBuf<unsigned long long> tstats_;             // [2] slots without a chosen trial, the sum of the chosen trial numbers
    bool profile_ = false;
    double phase_s_[4] = {0, 0, 0, 0};  // sample, gradient, scatter, apply (stream seconds, profile_ only)
    hipEvent_t ev_[7] = {};  // [0..4] around the four phases of a step, [5], [6] around a call of the solver
};

class BprSolver {
public:
    static int create(BprSolver** out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed, mfx_memspace space,
                      const char* fn = "mfx_bpr_create", int mode = MFX_BPR_NEG_UNIFORM, int64_t negatives = 1, const float* rank_weight = nullptr);
    int set_factors(const float* W, const float* H, mfx_memspace space);
    int get_factors(float* W, float* H, mfx_memspace space);
    int steps(int64_t n_steps, int64_t stats[4], double* seconds);
    int epochs(int32_t n_epochs, int64_t* stats, double* seconds);
    int64_t position() const { return (int64_t) pos_; }
    void times(double seconds[4]) const;
    void trial_stats(int64_t out[2]) const { out[0] = tstat_[0]; out[1] = tstat_[1]; }

private:
    BprSolver() = default;
    int run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds);
    BprCore core_;
    DevBuf<uint32_t> ptr_, idx_;
    int64_t nnz_ = 0;
    float lr_ = 0.f, lambda_ = 0.f;
    uint64_t seed_ = 0, pos_ = 0;
    int64_t tstat_[2] = {0, 0};
    bool have_factors_ = false;
};

int bpr_check_rows(const uint32_t* ptr, const uint32_t* idx, uint32_t rows, uint32_t cols, uint32_t nnz, hipStream_t st, uint32_t* first_bad);
int bpr_triples(uint64_t seed, int64_t first_slot, int64_t count, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* j, uint8_t* skipped);
int bpr_apply(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
              const uint8_t* skipped, float lr, float lambda, int64_t stats[4], int device);

// bpr_neg.hip
int bpr_check_neg(const char* fn, int mode, int64_t negatives, const float* rank_weight);
int bpr_rank_weights(int64_t cols, int64_t negatives, float* out);
int bpr_trials(uint64_t seed, int64_t first_slot, int64_t count, int64_t negatives, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* items,
               uint8_t* member);
int bpr_apply_neg(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i, int64_t negatives,
                  const uint32_t* items, const uint8_t* member, int mode, const float* rank_weight, float lr, float lambda, int64_t stats[4],
                  uint32_t* j_out, uint32_t* t_out, int device);

}  // namespace mfx

struct mfx_bpr_s {
    mfx::BprSolver* impl;
};
