// rec_foldin_cg.hpp -- the conjugate-gradient method that fold-in, training (rec_foldin_cg.hip, foldcg_launch) and explanation
// (rec_explain_cg.hip, explaincg_launch) share.  The method runs over SYSTEMS: system s belongs to row s / T of
// the CSR side, its vectors are rows s of [nsys][k] arrays, its |b|^2, gamma, step count and frozen flag live at s.  Fold-in
// and training are T = 1 (a system is a row); explanation has one system per (row, target) pair, T targets per row.
// Here: the lane helpers, the gather kernel and the end of the start kernels (device code both units compile), and the
// launches rec_foldin_cg.hip defines for both: the dense product, the sum of a split row's slots, the step loop.
#pragma once

#include <functional>

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

// Rows of k floats that a partial slot takes in the gathers' workspace: S of target t at row slot * stride + t, B (T = 1
// only) at row 2 slot + 1.  FoldCgWs::part (nslots * 2 * k floats) holds every mode of T = 1.
__host__ __device__ constexpr uint32_t cg_ws_stride(uint32_t T, int mode) { return mode & 2 ? 2u : T; }

namespace {

// One wavefront per work item of AlsHalf (a whole row, or a chunk of 2048 entries into a partial slot) and per group
// blockIdx.y of TG systems of its row; C = columns per lane: lane l holds coordinates l + 64 i.
// MODE bit 0: S[s] = sum_e c_e <h_e, v_s> h_e with v_s = V[s], for the systems s = seg T + t of the group that exist and are
// not frozen (frozen NULL: none is); bit 1 (TG = 1): B[s] = sum_e d_e h_e.  implicit: an entry counts when r_e > 0,
// c_e = w_e = fp32(alpha r_e), d_e = fp32(1 + w_e); explicit: every entry counts, c_e = 1, d_e = r_e.
// An entry's row of H is loaded ONCE for the group, four rows in flight before their reductions; per system <h_e, v_s> by the
// fma chain over i and the butterfly over the lanes, then (c_e <h_e, v_s>) h_e from the registers that still hold the row: a
// system's bits depend neither on TG nor on the other systems of its group.
// A whole row (slot < 0) writes rows s of S / B; a chunk writes its slot of ws (cg_ws_stride).
template <int C, int TG, int MODE>
__global__ __launch_bounds__(64) void k_cg_gather(const AlsItem* __restrict__ items, uint32_t nitems, const uint32_t* __restrict__ idx,
                                                  const float* __restrict__ val, const float* __restrict__ X, uint32_t x_rows, uint32_t k,
                                                  int32_t implicit, float alpha, uint32_t T, const float* __restrict__ V,
                                                  const uint32_t* __restrict__ frozen, float* __restrict__ S, float* __restrict__ B,
                                                  float* __restrict__ ws) {
    static_assert(TG == 1 || MODE == 1, "B is formed one system per wavefront");
    constexpr int U = kGatherRows;
    const uint32_t lane = threadIdx.x & 63;
    if (blockIdx.x >= nitems) return;
    const AlsItem it = items[blockIdx.x];
    if (it.hi == it.lo) return;  // (the start kernels zero and freeze the systems of an empty row)
    const uint32_t t0 = blockIdx.y * TG;
    const size_t sys0 = (size_t) it.seg * T + t0;
    uint32_t live = 0;  // bit j: system sys0 + j exists and is not frozen (wave-uniform); TG = 1: the one test of the wavefront
#pragma unroll
    for (int j = 0; j < TG; ++j)
        if (t0 + j < T && !(frozen && frozen[sys0 + j])) live |= 1u << j;
    live = __builtin_amdgcn_readfirstlane(live);
    if (!live) return;
    float pv[TG][C], acc[TG][C], accb[C];
#pragma unroll
    for (int j = 0; j < TG; ++j)
#pragma unroll
        for (int i = 0; i < C; ++i) {
            pv[j][i] = (MODE & 1) && (TG == 1 || (live >> j & 1)) && 64 * i + lane < k ? V[(sys0 + j) * k + 64 * i + lane] : 0.f;
            acc[j][i] = 0.f;
        }
#pragma unroll
    for (int i = 0; i < C; ++i) accb[i] = 0.f;
    for (uint32_t q0 = it.lo; q0 < it.hi; q0 += U) {
        float hv[U][C], cw[U], cb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + u;
            const bool ok = q < it.hi;  // wave-uniform; past the end: the zero row of X, weight 0
            const float r = ok ? val[q] : 0.f;
            const float* x = X + (size_t) (ok ? idx[q] : x_rows) * k;
            if (implicit) {
                const float w = alpha * r;
                cw[u] = r > 0.f ? w : 0.f;
                cb[u] = r > 0.f ? 1.f + w : 0.f;
            } else {
                cw[u] = ok ? 1.f : 0.f;
                cb[u] = r;
            }
#pragma unroll
            for (int i = 0; i < C; ++i) hv[u][i] = 64 * i + lane < k ? x[64 * i + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q0 + u < it.hi) {  // wave-uniform
                if (MODE & 1) {
#pragma unroll
                    for (int j = 0; j < TG; ++j) {
                        if (TG == 1 || (live >> j & 1)) {  // wave-uniform
                            float t = 0.f;
#pragma unroll
                            for (int i = 0; i < C; ++i) t = __builtin_fmaf(hv[u][i], pv[j][i], t);
                            const float ct = cw[u] * wave_sum(t);
#pragma unroll
                            for (int i = 0; i < C; ++i) acc[j][i] = __builtin_fmaf(ct, hv[u][i], acc[j][i]);
                        }
                    }
                }
                if (MODE & 2) {
#pragma unroll
                    for (int i = 0; i < C; ++i) accb[i] = __builtin_fmaf(cb[u], hv[u][i], accb[i]);
                }
            }
        }
    }
    if (MODE & 1) {
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            if (TG > 1 && !(live >> j & 1)) continue;
            float* s = it.slot < 0 ? S + (sys0 + j) * k : ws + ((size_t) it.slot * cg_ws_stride(T, MODE) + t0 + j) * k;
#pragma unroll
            for (int i = 0; i < C; ++i)
                if (64 * i + lane < k) s[64 * i + lane] = acc[j][i];
        }
    }
    if (MODE & 2) {
        float* b = it.slot < 0 ? B + sys0 * k : ws + (size_t) (2 * it.slot + 1) * k;
#pragma unroll
        for (int i = 0; i < C; ++i)
            if (64 * i + lane < k) b[64 * i + lane] = accb[i];
    }
}

// The end of both start kernels, one wavefront per system s at offset o = s k, after R[s] = b: b2 = |b|^2 (0 as well where
// the system has no right-hand side), r2 = |b - A y0|^2.  b2 = 0: y = 0, frozen, 0 steps, whatever the start held.  Any other
// system: |b|^2 kept, frozen at once if tol > 0 and |r| <= tol |b|.  r, z and p of a frozen system are zeroed so that nothing
// unwritten is ever read.  (explicit: Z is R)
__device__ __forceinline__ void cg_start_tail(size_t s, size_t o, uint32_t k, uint32_t lane, float b2, float r2, float tol,
                                              float* __restrict__ Y, float* R, float* Z, float* __restrict__ P, float* __restrict__ bb,
                                              uint32_t* __restrict__ frozen, int32_t* __restrict__ counts) {
    if (b2 == 0.f) {
        for (uint32_t c = lane; c < k; c += 64) Y[o + c] = R[o + c] = Z[o + c] = P[o + c] = 0.f;
        if (lane == 0) { frozen[s] = 1; counts[s] = 0; bb[s] = 0.f; }
        return;
    }
    const bool stop = tol > 0.f && sqrtf(r2) <= tol * sqrtf(b2);
    if (stop)
        for (uint32_t c = lane; c < k; c += 64) Z[o + c] = P[o + c] = 0.f;
    if (lane == 0) { frozen[s] = stop; counts[s] = 0; bb[s] = b2; }
}

}  // namespace

// out = V M (+ add) over the rows of V [nseg][k] that are not frozen, M [k][k] symmetric (k_foldcg_dense): an output row
// depends on its own input row and the k order alone, so the rows may as well be systems
int foldcg_dense(const float* V, uint32_t nseg, uint32_t k, const float* M, const uint32_t* frozen, const float* add, float* out,
                 hipStream_t st);

// After a gather in `mode` over T systems per row: the partial slots of every split row of h into S / B (k_cg_reduce)
int cg_reduce(const AlsHalf& h, uint32_t k, uint32_t T, int mode, const uint32_t* frozen, const float* ws, float* S, float* B,
              hipStream_t st);

// The method after the start kernel of either entry function, on nsys = h.nseg T systems: w.R holds r (frozen systems zeroed),
// w.bb, w.frozen and counts are set, Y [nsys][k] is the iterate.  gather() must leave in w.Q the gathered part of A p for
// p = w.P, over the systems that are not frozen.  The first direction counts into first_active (or NULL); with m.tol > 0 the
// later ones count into w.active + s + 1 and the host reads each counter to stop when every system is frozen.  fail may be
// NULL.  Returns after a stream synchronisation.  (The sequence of launches: DESIGN 5.21.)
int cg_iterate(const AlsHalf& h, uint32_t T, uint32_t k, const FoldCg& m, float* Y, FoldCgWs& w, int32_t* counts, uint32_t* fail,
               uint32_t* first_active, const std::function<int()>& gather, hipStream_t st);

// The target solves of mfx_rec_explain_cg (rec_explain_cg.hip): for every row q of h and every t < n_targets the iterate of
// A_q z = X[targets[q][t]] from z = 0 into Z [h.nseg * n_targets][k], by the recurrence, the operator, the preconditioner and
// the stop rule of foldcg_launch for row q (cold start).  Z must be zero.  A padding target, a row without counting entries and
// a zero target row stay zero and count 0 steps.  targets: device, checked (< x_rows or the padding); counts: device
// [h.nseg * n_targets] (steps applied) or NULL.  The pairs must number less than 2^31.
int explaincg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, const FoldCg& m, const uint32_t* targets,
                     uint32_t n_targets, float* Z, int32_t* counts, hipStream_t st);

}  // namespace mfx
