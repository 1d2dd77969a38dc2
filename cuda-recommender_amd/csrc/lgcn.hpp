// lgcn.hpp -- the host interface of LightGCN training (lgcn.hip: mfx_lgcn_*): BPR on embeddings propagated through the
// symmetrically normalised interaction graph.  The contract is in include/mfx.h ("LightGCN"), DESIGN 5.22 has the choices
// and the measurements.  No device code here: api.hip includes this file.
#pragma once

#include "bpr.hpp"

namespace mfx {

// One side of the graph as the destination of a half-pass: its rows gather rows of the other side.
struct LgcnSide {
    int64_t n = 0;               // rows of this side
    DevBuf<uint32_t> ptr, idx;   // [n + 1], [nnz]: the ids of the other side in stored order
    DevBuf<float> s;             // [n] fp32(1 / sqrt((double) degree)), 0 for an empty row
    DevBuf<uint4> work;          // [n_work] (row, first entry, end entry, partial slot or 2^32 - 1), heaviest first
    DevBuf<uint4> heavy;         // [n_heavy] (row, first partial slot, segments, 0) of the rows above 1024 entries
    DevBuf<float> part;          // [n_part][k] the segment sums of the heavy rows
    uint32_t n_work = 0, n_heavy = 0, n_part = 0;
    uint32_t heaviest = 0;       // entries of the longest row
};

// The graph on the device and the layer buffers of one propagation-and-mean.
class LgcnGraph {
public:
    // Reads both sides of R (values ignored), checks the rows of either side and that the CSC side is the transpose pattern
    // of the CSR side, builds the scale tables and the work orders.
    int init(const char* fn, const mfx_csx* R, mfx_memspace space, int64_t k, int layers, int device, hipStream_t st);
    // (outW, outH) = the mean of (inW, inH) and its `layers_` propagated copies; in and out must not overlap.
    int propagate(const float* inW, const float* inH, float* outW, float* outH);

    int64_t rows_ = 0, cols_ = 0, nnz_ = 0, k_ = 0;
    int layers_ = 0, device_ = 0;
    hipStream_t st_ = nullptr;
    LgcnSide user_, item_;
    DevBuf<float> layerW_[2], layerH_[2];  // E^l for odd and even l >= 1 (layers_ >= 2 only)

private:
    int build_side(LgcnSide& side, const std::vector<uint32_t>& ptr);
    int half_pass(const LgcnSide& dst, const float* s_src, const float* X, float* out, const float* sum_in, float* sum_out, bool last);
};

// The device state of one LightGCN step: a BprCore whose factors are the final embeddings, the base embeddings, the
// gradient of the final embeddings and its propagated mean.
class LgcnCore {
public:
    int init(const char* fn, const mfx_csx* R, mfx_memspace space, int64_t k, int64_t batch, int layers, int device);
    int set_base(const float* W0, const float* H0, mfx_memspace space);
    int get_base(float* W0, float* H0, mfx_memspace space);
    int forward();  // the final embeddings of the current base into bpr_.W_, bpr_.H_
    // One step over the n slots in bpr_.u_, i_, j_, skip_; the counts are ADDED to bpr_.stats_.
    int step(uint32_t n, float lr, float lambda);

    BprCore bpr_;
    LgcnGraph graph_;
    DevBuf<float> W0_, H0_, GW_, GH_, DW_, DH_;
    bool profile_ = false;
    double phase_s_[6] = {0, 0, 0, 0, 0, 0};  // sample, forward, gradient, scatter, backward, update
    hipEvent_t ev_[4] = {};                   // before the sampler, before the forward pass, after the backward pass, after the update
    ~LgcnCore();
};

class LgcnSolver {
public:
    static int create(LgcnSolver** out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, int32_t layers, uint64_t seed,
                      mfx_memspace space);
    int set_base(const float* W0, const float* H0, mfx_memspace space);
    int get_base(float* W0, float* H0, mfx_memspace space);
    int get_factors(float* W, float* H, mfx_memspace space);
    int steps(int64_t n_steps, int64_t stats[4], double* seconds);
    int epochs(int32_t n_epochs, int64_t* stats, double* seconds);
    int64_t position() const { return (int64_t) pos_; }
    void times(double seconds[6]) const;

private:
    LgcnSolver() = default;
    int run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds);
    LgcnCore core_;
    float lr_ = 0.f, lambda_ = 0.f;
    uint64_t seed_ = 0, pos_ = 0;
    bool have_base_ = false;
};

int lgcn_propagate(const mfx_csx* R, const float* W0, const float* H0, int64_t k, int32_t layers, float* W, float* H, int device);
int lgcn_apply(const mfx_csx* R, int64_t k, float* W0, float* H0, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
               const uint8_t* skipped, int32_t layers, float lr, float lambda, int64_t stats[4], int device);

}  // namespace mfx

struct mfx_lgcn_s {
    mfx::LgcnSolver* impl;
};
