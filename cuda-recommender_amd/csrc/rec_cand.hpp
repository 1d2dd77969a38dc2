// rec_cand.hpp -- what the kernels over candidate lists share (rec_candidates.hip: mfx_cand_*, rec_diversify.hip: mfx_div_*):
// the size of a piece, the lane-owned score chain, the exclusion-row search and the stream events around a call's phases.
// The checks of the lists themselves are Recommender::cand_stage / cand_check (recommend.hpp).  Device code, included by
// .hip files only.
#pragma once

#include "rec_tiles.hpp"

namespace mfx {

namespace {

constexpr int kCandChunk = 2048;    // candidates of one piece: 16 KiB of LDS for the sort
constexpr int kCandThreads = 256, kCandWaves = 4;

__device__ inline void wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

__device__ inline bool excluded(const uint32_t* ex, uint32_t lo, uint32_t hi, uint32_t item) {
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ex[mid] < item) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && ex[lo] == item;
}

// The score chain of rec_rank.hip's chain_score: fma over t = 0 .. k-1 ascending from +0, the row read by its lane.
__device__ inline float lane_chain(const float* wr, const float* hr, int k, int kt) {
    float acc = 0.f;
    int t = 0;
    if ((kt & 3) == 0) {
#pragma unroll 4  // (four 16-byte loads of the row in flight)
        for (; t + 4 <= k; t += 4) {
            const f32x4 h = *reinterpret_cast<const f32x4*>(hr + t);
            const f32x4 w = *reinterpret_cast<const f32x4*>(wr + t);
            acc = __builtin_fmaf(h.x, w.x, acc);
            acc = __builtin_fmaf(h.y, w.y, acc);
            acc = __builtin_fmaf(h.z, w.z, acc);
            acc = __builtin_fmaf(h.w, w.w, acc);
        }
    }
    for (; t < k; ++t) acc = __builtin_fmaf(hr[t], wr[t], acc);
    return acc;
}

struct Events {  // four stream events around the three phases
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    int create() {
        for (auto& x : e) MFX_HIP(hipEventCreate(&x));
        return MFX_OK;
    }
    ~Events() {
        for (auto x : e)
            if (x) (void) hipEventDestroy(x);
    }
};

}  // namespace

}  // namespace mfx
