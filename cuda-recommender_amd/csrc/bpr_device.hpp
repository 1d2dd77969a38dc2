// bpr_device.hpp -- what the two device units of BPR training share (bpr.hip: the step; bpr_neg.hip: the trials): the
// stateless sampler, one function for kernel and host each, the states of a slot and the single fp32 operations.  The
// contract is in include/mfx.h ("BPR training").  Included by those two units and by lgcn.hip, which runs the same step on
// propagated embeddings.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace mfx {

constexpr uint8_t kCounted = 0, kSkipped = 1, kBad = 2;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

// ---------------------------------------------------------------------------------------------- the sampler
__host__ __device__ inline uint64_t bpr_fin(uint64_t z) {  // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t bpr_stream(uint64_t seed) { return bpr_fin(seed + kGolden); }
__host__ __device__ inline uint64_t bpr_draw(uint64_t s0, uint64_t ctr) { return bpr_fin(s0 + (ctr + 1) * kGolden); }

// Slot n of the stream s0 over the matrix (ptr, idx): the entry p = a mod nnz gives the user (the row that holds p) and the
// positive item, b mod cols the sampled item, skipped when it is in the row (the search of rec_cand.hpp's excluded()).
// ptr must be non-decreasing from 0 to nnz: then every read stays inside ptr [rows + 1] and idx [nnz].
__host__ __device__ inline void bpr_sample(uint64_t s0, uint64_t n, const uint32_t* ptr, const uint32_t* idx, uint32_t rows, uint32_t cols,
                                           uint32_t nnz, uint32_t* u, uint32_t* i, uint32_t* j, uint8_t* skipped) {
    const uint32_t p = (uint32_t) (bpr_draw(s0, 2 * n) % nnz);
    const uint32_t item = (uint32_t) (bpr_draw(s0, 2 * n + 1) % cols);
    uint32_t lo = 0, hi = rows;  // ptr[lo] <= p < ptr[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    uint32_t a = ptr[lo], b = ptr[lo + 1];
    const uint32_t end = b;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (idx[mid] < item) a = mid + 1;
        else b = mid;
    }
    *u = lo;
    *i = idx[p];
    *j = item;
    *skipped = a < end && idx[a] == item;
}

// The trials of slot n beyond the first (which is bpr_sample's item): a stream of their own, s1 = fin(seed + 2 G), the
// slot's base b_n = fin(s1 + (n + 1) G) and trial t >= 2 the item fin(b_n + t G) mod cols; whether it is in row u by the
// search of bpr_sample.  Neither the mode nor the number of trials enters.
__host__ __device__ inline uint64_t bpr_trial_stream(uint64_t seed) { return bpr_fin(seed + 2 * kGolden); }
__host__ __device__ inline uint64_t bpr_trial_base(uint64_t s1, uint64_t n) { return bpr_fin(s1 + (n + 1) * kGolden); }
__host__ __device__ inline void bpr_trial(uint64_t base, uint32_t t, const uint32_t* ptr, const uint32_t* idx, uint32_t u, uint32_t cols,
                                          uint32_t* item_out, uint8_t* member) {
    const uint32_t item = (uint32_t) (bpr_fin(base + (uint64_t) t * kGolden) % cols);
    uint32_t a = ptr[u], b = ptr[u + 1];
    const uint32_t end = b;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (idx[mid] < item) a = mid + 1;
        else b = mid;
    }
    *item_out = item;
    *member = a < end && idx[a] == item;
}

// ---------------------------------------------------------------------------------------------- single fp32 operations
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

}  // namespace mfx
