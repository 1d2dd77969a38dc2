// ease.hpp -- the host interface of EASE, the closed-form dense item-item model (ease.hip and ease_inverse.hip: mfx_ease_*).
// The contract is in include/mfx.h, DESIGN 5.19 has the kernels and the sizing.  No device code here: api.hip includes this file.
#pragma once

#include "common.hpp"

namespace mfx {

constexpr uint32_t kEaseMaxCols = 32768;  // every element offset of a [cols][cols] matrix stays below 2^30

// The blocked SPD inverse of spd_inverse.hip with the cap lifted (ease_inverse.hip): Minv [n][n] ~ G^-1 for G [n][n], both
// fp32 on the device, 1 <= n <= 32768.  flags: 0 (the grouped kernels) or MFX_EASE_INV_SIMPLE (one wavefront per block);
// the bits are the same.  ws: ease_inverse_ws_floats(n) floats.  Stream-ordered launches only; nothing is read back.  A pivot
// <= 0 or not finite counts into *fail.
size_t ease_inverse_ws_floats(uint32_t n);
int ease_inverse_launch(const float* G, uint32_t n, float* Minv, float* ws, uint32_t* fail, int flags, hipStream_t st);

// The model resident on the device: B [cols][cols], row i the weights from source item i to every target.
class Ease {
public:
    static int gram(const mfx_csx* X, float lambda, int32_t tile_items, float* G, mfx_memspace space, int device);
    static int inverse(int64_t n, const float* A, float* Ainv, int flags, mfx_memspace space, int device);
    static int weights_from_inverse(int64_t n, const float* P, float* B, mfx_memspace space, int device);
    static int train(Ease** out, const mfx_csx* X, float lambda, int flags, int32_t tile_items, mfx_memspace space, int device);
    static int from_weights(Ease** out, int64_t cols, const float* B, mfx_memspace space, int device);
    int weights(int64_t first, int64_t count, float* B_rows, mfx_memspace space);
    int recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                  int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space);
    void times(double seconds[6]) const {
        for (int p = 0; p < 6; ++p) seconds[p] = t_[p];
    }

private:
    Ease() = default;
    int init(int64_t cols, int device);
    int64_t cols_ = 0;
    int device_ = 0, cus_ = 1;
    hipStream_t st_ = nullptr;
    DevBuf<float> B_;
    double t_[6] = {0, 0, 0, 0, 0, 0};  // train: checks, Gram pass, inverse, weights; recommend (summed over the calls): checks, pass
};

}  // namespace mfx

struct mfx_ease_s {
    mfx::Ease* impl;
};
