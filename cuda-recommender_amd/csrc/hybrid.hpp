// hybrid.hpp -- the host interface of hybrid BPR training (hybrid.hip: mfx_hyb_*): BPR on rows whose vectors are the weighted
// sums of the embeddings of their features (LightFM's model without biases).  The contract is in include/mfx.h ("Hybrid
// BPR"), DESIGN 5.23 has the choices and the measurements.  No device code here: api.hip includes this file.
#pragma once

#include "bpr.hpp"

namespace mfx {

// One side's feature matrix (CSR with values) and its embedding table with the step's state of every feature.
struct HybSide {
    int64_t n = 0, nf = 0, nnz = 0;      // rows of the side, features, entries
    DevBuf<uint32_t> ptr, idx;           // [n + 1], [nnz]
    DevBuf<float> val;                   // [nnz]
    DevBuf<float> E;                     // [nf][k]
    DevBuf<unsigned long long> acc;      // [nf][k] the sums of the step, 0 between steps
    DevBuf<uint32_t> cnt, claim;         // [nf] m_f, 0 between steps; the smallest key 3 t + role that spread into f, 2^32 - 1 between steps
    // Uploads F (NULL: the identity on n rows) and checks its rows on the device; `what` names the side in a refusal.
    int init(const char* fn, const char* what, const mfx_features* F, int64_t n, mfx_memspace space, hipStream_t st);
    int alloc_state(int64_t k, hipStream_t st);
};

// The device state of one hybrid step: a BprCore whose factors are scratch for the embedded rows, and the two sides.
class HybCore {
public:
    ~HybCore();
    int init(const char* fn, int64_t rows, int64_t cols, int64_t k, int64_t batch, const mfx_features* Fu, const mfx_features* Fi,
             mfx_memspace space, int device);
    int set_tables(const float* Eu, const float* Ei, mfx_memspace space);
    int get_tables(float* Eu, float* Ei, mfx_memspace space);
    int materialise(bool users, bool items);  // every row of the sides asked for into bpr_.W_, bpr_.H_
    // One step over the n slots in bpr_.u_, i_, j_, skip_; the counts are ADDED to bpr_.stats_.
    int step(uint32_t n, float lr, float lambda);

    BprCore bpr_;
    HybSide user_, item_;
    bool profile_ = false;
    double phase_s_[6] = {0, 0, 0, 0, 0, 0};  // sample, embed, gradient, scatter, spread, apply
    hipEvent_t ev_[4] = {};                   // before the sampler, before the embedding, after the spread, after the apply
};

class HybSolver {
public:
    static int create(HybSolver** out, const mfx_csx* R, const mfx_features* Fu, const mfx_features* Fi, const mfx_params* p, float lr,
                      int64_t batch, uint64_t seed, mfx_memspace space);
    int set_embeddings(const float* Eu, const float* Ei, mfx_memspace space);
    int get_embeddings(float* Eu, float* Ei, mfx_memspace space);
    int get_factors(float* W, float* H, mfx_memspace space);
    int steps(int64_t n_steps, int64_t stats[4], double* seconds);
    int epochs(int32_t n_epochs, int64_t* stats, double* seconds);
    int64_t position() const { return (int64_t) pos_; }
    void times(double seconds[6]) const;

private:
    HybSolver() = default;
    int run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds);
    HybCore core_;
    DevBuf<uint32_t> ptr_, idx_;  // the CSR side of R: the sampler's
    int64_t nnz_ = 0;
    float lr_ = 0.f, lambda_ = 0.f;
    uint64_t seed_ = 0, pos_ = 0;
    bool have_tables_ = false;
};

int hyb_embed(const mfx_features* F, const float* E, int64_t k, float* out, int device);
int hyb_apply(int64_t rows, int64_t cols, int64_t k, const mfx_features* Fu, const mfx_features* Fi, float* Eu, float* Ei, int64_t n,
              const uint32_t* u, const uint32_t* i, const uint32_t* j, const uint8_t* skipped, float lr, float lambda, int64_t stats[4],
              int device);

}  // namespace mfx

struct mfx_hyb_s {
    mfx::HybSolver* impl;
};
