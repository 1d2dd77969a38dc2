// knn.hpp -- the host interface of the item-kNN neighbourhood model (knn.hip: mfx_knn_*).  The contract is in
// include/mfx.h, DESIGN 5.16 has the kernels and the sizing.  No device code here: api.hip includes this file.
#pragma once

#include "common.hpp"

namespace mfx {

// The neighbour lists of every item, resident on the device: nbr_idx [cols][K] and nbr_sim [cols][K].
class Knn {
public:
    static int build(Knn** out, const mfx_csx* X, int32_t K, int32_t tile_items, mfx_memspace space, int device);
    static int from_lists(Knn** out, int64_t cols, int32_t K, const uint32_t* nbr_idx, const float* nbr_sim, mfx_memspace space, int device);
    int lists(uint32_t* nbr_idx, float* nbr_sim, mfx_memspace space);
    int neighbours(int64_t nq, const uint32_t* items, int32_t n_top, uint32_t* out_items, float* out_sims, mfx_memspace space);
    int recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                  int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space);
    void times(double seconds[4]) const {
        for (int p = 0; p < 4; ++p) seconds[p] = t_[p];
    }

private:
    Knn() = default;
    int init(int64_t cols, int32_t K, int device);
    int64_t cols_ = 0;
    int K_ = 0, device_ = 0, cus_ = 1;
    hipStream_t st_ = nullptr;
    DevBuf<uint32_t> nidx_;
    DevBuf<float> nsim_;
    double t_[4] = {0, 0, 0, 0};  // build: checks + work order, similarity pass; recommend (summed over the calls): checks, pass
};

}  // namespace mfx

struct mfx_knn_s {
    mfx::Knn* impl;
};
