// rec_foldin_cg.hpp -- what rec_foldin_cg.hip (fold-in by conjugate gradients) and rec_explain_cg.hip (the same method over
// the pairs (row, target) for mfx_rec_explain_cg) share: the lane helpers of their kernels, the dense product, the launches.
#pragma once

#include "als_solver.hpp"

namespace mfx {

constexpr int kGatherRows = 4;  // rows of H in flight per wavefront of the gathers

__device__ __forceinline__ float wave_sum(float v) {  // butterfly over the 64 lanes: the same value, in a fixed order, in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rho of a row: 0 = none (implicit: G carries lambda), 1 = lambda, 2 = fp32(lambda * n) for a row of n entries
__device__ __forceinline__ float row_rho(int32_t reg, float lambda, const uint32_t* __restrict__ ptr, uint32_t seg) {
    return reg == 2 ? lambda * (float) (ptr[seg + 1] - ptr[seg]) : lambda;
}

// out = V M (+ add) over the rows of V [nseg][k] that are not frozen, M [k][k] symmetric (k_foldcg_dense): an output row
// depends on its own input row and the k order alone, so the rows may as well be the pairs of rec_explain_cg.hip
int foldcg_dense(const float* V, uint32_t nseg, uint32_t k, const float* M, const uint32_t* frozen, const float* add, float* out,
                 hipStream_t st);

// The target solves of mfx_rec_explain_cg (rec_explain_cg.hip): for every row q of h and every t < n_targets the iterate of
// A_q z = X[targets[q][t]] from z = 0 into Z [h.nseg * n_targets][k], by the recurrence, the operator, the preconditioner and
// the stop rule of foldcg_launch for row q (cold start).  Z must be zero.  A padding target, a row without counting entries and
// a zero target row stay zero and count 0 steps.  targets: device, checked (< x_rows or the padding); counts: device
// [h.nseg * n_targets] (steps applied) or NULL.  The pairs must number less than 2^31.
int explaincg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, const FoldCg& m, const uint32_t* targets,
                     uint32_t n_targets, float* Z, int32_t* counts, hipStream_t st);

}  // namespace mfx
