// slim.hpp -- the host interface of SLIM, the sparse linear item model on given supports (slim.hip: mfx_slim_*).  The
// contract is in include/mfx.h, DESIGN 5.18 has the kernels and the sizing.  No device code here: api.hip includes this file.
#pragma once

#include "common.hpp"

namespace mfx {

struct SlimParams {
    float l1, l2, tol;
    int32_t sweeps;
    int flags;
};

// The model resident on the device: the support S [cols][K], the weights w [cols][K], the sweeps run per item, and the
// transpose by source item (iptr [cols + 1], targets ascending and their weights) that recommend walks.
class Slim {
public:
    static int train(Slim** out, const mfx_csx* X, int32_t K, const uint32_t* support, const SlimParams& p, int32_t tile_items, int64_t* failed,
                     mfx_memspace space, int device);
    static int gram(const mfx_csx* X, int32_t K, const uint32_t* support, int32_t tile_items, float* blocks, mfx_memspace space, int device);
    static int solve(int64_t n, int32_t K, const float* blocks, const uint32_t* n_real, const SlimParams& p, float* w, int32_t* sweeps_used,
                     int64_t* failed, mfx_memspace space, int device);
    static int from_lists(Slim** out, int64_t cols, int32_t K, const uint32_t* support, const float* w, mfx_memspace space, int device);
    int weights(uint32_t* support, float* w, int32_t* sweeps_used, mfx_memspace space);
    int recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                  int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space);
    void times(double seconds[5]) const {
        for (int p = 0; p < 5; ++p) seconds[p] = t_[p];
    }

private:
    Slim() = default;
    int init(int64_t cols, int32_t K, int device);
    int set_support(const char* fn, const uint32_t* support, const float* w, mfx_memspace space);
    int transpose_weights();
    int64_t cols_ = 0;
    int K_ = 0, device_ = 0, cus_ = 1;
    hipStream_t st_ = nullptr;
    DevBuf<uint32_t> S_, nreal_, iptr_, tj_, tp_;  // tp: the slot of the source in the target's list
    DevBuf<float> w_, tw_;
    DevBuf<int32_t> sweeps_;
    size_t npairs_ = 0;  // real slots of S = entries of the transpose
    double t_[5] = {0, 0, 0, 0, 0};  // train: checks + inverse lists, Gram pass, solve; recommend (summed over the calls): checks, pass
};

}  // namespace mfx

struct mfx_slim_s {
    mfx::Slim* impl;
};
