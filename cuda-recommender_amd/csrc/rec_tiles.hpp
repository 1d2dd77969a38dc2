// rec_tiles.hpp -- what the recommender's passes over the packed H share (recommend.hip: top-N, rec_rank.hip: ranks):
// the workgroup shape and the total order.  Device code, included by .hip files only.
#pragma once

#include <algorithm>

#include "common.hpp"

#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())

namespace mfx {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kRecWaves = 4;                 // waves per workgroup
constexpr int kRecThreads = 64 * kRecWaves;
constexpr int kRecUsers = 32 * kRecWaves;    // users per workgroup
constexpr int kTile = 32;                    // items per LDS stage (one 32 x 32 MFMA tile per wave)
constexpr uint32_t kPad = 0xFFFFFFFFu;

__device__ inline bool beats(float as, uint32_t ai, float bs, uint32_t bi) {
    return as > bs || (as == bs && ai < bi);
}

__device__ inline int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

inline int grid_for(size_t n) { return (int) std::min<size_t>((n + 255) / 256, 4096); }

}  // namespace

}  // namespace mfx
