// bpr.hpp -- the host interface of BPR training (bpr.hip: mfx_bpr_*).  The contract is in include/mfx.h, DESIGN 5.15 has the
// choice of the accumulation and the measurements.  No device code here: api.hip includes this file.
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
    int step(uint32_t n, float lr, float lambda);

    int64_t rows_ = 0, cols_ = 0, k_ = 0, batch_ = 0;
    int device_ = 0, gs_ = 64;  // gs_: lanes that share one row in the scatter and apply kernels (a power of two >= min(k, 64))
    hipStream_t st_ = nullptr;
    DevBuf<float> W_, H_, g_;
    DevBuf<unsigned long long> accW_, accH_, stats_;
    DevBuf<uint32_t> cntW_, cntH_, claimW_, claimH_, u_, i_, j_;
    DevBuf<uint8_t> skip_, state_;
    bool profile_ = false;
    double phase_s_[4] = {0, 0, 0, 0};  // sample, gradient, scatter, apply (stream seconds, profile_ only)
    hipEvent_t ev_[7] = {};  // [0..4] around the four phases of a step, [5], [6] around a call of the solver
};

class BprSolver {
public:
    static int create(BprSolver** out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed, mfx_memspace space);
    int set_factors(const float* W, const float* H, mfx_memspace space);
    int get_factors(float* W, float* H, mfx_memspace space);
    int steps(int64_t n_steps, int64_t stats[4], double* seconds);
    int epochs(int32_t n_epochs, int64_t* stats, double* seconds);
    int64_t position() const { return (int64_t) pos_; }
    void times(double seconds[4]) const;

private:
    BprSolver() = default;
    int run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds);
    BprCore core_;
    DevBuf<uint32_t> ptr_, idx_;
    int64_t nnz_ = 0;
    float lr_ = 0.f, lambda_ = 0.f;
    uint64_t seed_ = 0, pos_ = 0;
    bool have_factors_ = false;
};

int bpr_triples(uint64_t seed, int64_t first_slot, int64_t count, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* j, uint8_t* skipped);
int bpr_apply(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
              const uint8_t* skipped, float lr, float lambda, int64_t stats[4], int device);

}  // namespace mfx

struct mfx_bpr_s {
    mfx::BprSolver* impl;
};
