// rec_explain_cg.hip -- the target solves of mfx_rec_explain_cg on gfx950: A_q z = h_t for every query row q and every target
// t of its slot, by the preconditioned conjugate gradients of rec_foldin_cg.hip (the operator, the preconditioner, the
// recurrence and the stop rule of row q), ranks up to 1024.
// The systems are the pairs (q, t), rows q T + t of [nu T][k] arrays: z (the caller's Z), r, the preconditioned residual
// (implicit), p and A p; |h_t|^2, gamma, the step count and the frozen flag live per pair.  The method is step-synchronous
// over all pairs.  The kernels, in the order of a step:
//   k_explcg_gather<C, TG>  one wavefront per work item of AlsHalf (a whole row, or a chunk of 2048 entries into a partial
//                           slot) and per group of TG targets: lane l holds coordinates l + 64 i of p_t and of the sum of
//                           every target of the group.  An entry's row of H is loaded ONCE for the group, four rows in flight;
//                           per target <h_e, p_t> by the fma chain over i and the butterfly over the lanes, then
//                           (c_e <h_e, p_t>) h_e from the registers that hold the row: per target the very operation order of
//                           k_foldcg_gather<C, 1>, so a pair's bits depend neither on TG nor on the other targets of its slot
//   k_explcg_reduce         the partial slots of a split row summed in slot order, per target
//   k_foldcg_dense          (implicit; rec_foldin_cg.hip) G p on top of the gathered part, and Minv r: row by row
//   k_explcg_start          r = h_t, |h_t|^2; a padding target, a row without counting entries, h_t = 0: zero, frozen, 0 steps
//   k_explcg_step           <p, q>, a, z += a p, r -= a q, the count, the stop test |r| <= tol |h_t|
//   k_explcg_dir            gamma' = <r, M^-1 r>, p = M^-1 r + (gamma' / gamma) p; the pairs still active counted for the host
// A frozen pair is skipped by every kernel, a group of frozen targets does no gathering.  No float atomics; every sum has a
// fixed order that depends on the pair alone.
#include <algorithm>

#include "rec_foldin_cg.hpp"

namespace mfx {
namespace {

constexpr uint32_t kPadTarget = 0xFFFFFFFFu;

// S[seg T + t] = sum_e c_e <h_e, p_t> h_e for the targets t of group blockIdx.y that are not frozen, p_t = P[seg T + t].
// implicit: an entry counts when r_e > 0, c_e = fp32(alpha r_e); explicit: every entry counts, c_e = 1.  C = columns per lane.
// A whole row (slot < 0) writes S [seg T + t][k]; a chunk writes row (slot T + t) of ws.
template <int C, int TG>
__global__ __launch_bounds__(64) void k_explcg_gather(const AlsItem* __restrict__ items, uint32_t nitems, const uint32_t* __restrict__ idx,
                                                      const float* __restrict__ val, const float* __restrict__ X, uint32_t x_rows, uint32_t k,
                                                      int32_t implicit, float alpha, uint32_t T, const float* __restrict__ P,
                                                      const uint32_t* __restrict__ frozen, float* __restrict__ S, float* __restrict__ ws) {
    constexpr int U = kGatherRows;
    const uint32_t lane = threadIdx.x & 63;
    if (blockIdx.x >= nitems) return;
    const AlsItem it = items[blockIdx.x];
    if (it.hi == it.lo) return;  // (k_explcg_start froze the pairs of an empty row)
    const uint32_t t0 = blockIdx.y * TG;
    const size_t pair0 = (size_t) it.seg * T + t0;
    uint32_t live = 0;  // bit j: target t0 + j exists and is not frozen (wave-uniform)
#pragma unroll
    for (int j = 0; j < TG; ++j)
        if (t0 + j < T && !frozen[pair0 + j]) live |= 1u << j;
    live = __builtin_amdgcn_readfirstlane(live);
    if (!live) return;
    float pv[TG][C], acc[TG][C];
#pragma unroll
    for (int j = 0; j < TG; ++j)
#pragma unroll
        for (int i = 0; i < C; ++i) {
            pv[j][i] = (live >> j & 1) && 64 * i + lane < k ? P[(pair0 + j) * k + 64 * i + lane] : 0.f;
            acc[j][i] = 0.f;
        }
    for (uint32_t q0 = it.lo; q0 < it.hi; q0 += U) {
        float hv[U][C], cw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + u;
            const bool ok = q < it.hi;  // wave-uniform; past the end: the zero row of X, weight 0
            const float r = ok ? val[q] : 0.f;
            const float* x = X + (size_t) (ok ? idx[q] : x_rows) * k;
            if (implicit) {
                const float w = alpha * r;
                cw[u] = r > 0.f ? w : 0.f;
            } else {
                cw[u] = ok ? 1.f : 0.f;
            }
#pragma unroll
            for (int i = 0; i < C; ++i) hv[u][i] = 64 * i + lane < k ? x[64 * i + lane] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q0 + u < it.hi) {  // wave-uniform
#pragma unroll
                for (int j = 0; j < TG; ++j) {
                    if (live >> j & 1) {  // wave-uniform
                        float t = 0.f;
#pragma unroll
                        for (int i = 0; i < C; ++i) t = __builtin_fmaf(hv[u][i], pv[j][i], t);
                        const float ct = cw[u] * wave_sum(t);
#pragma unroll
                        for (int i = 0; i < C; ++i) acc[j][i] = __builtin_fmaf(ct, hv[u][i], acc[j][i]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TG; ++j) {
        if (!(live >> j & 1)) continue;
        float* s = it.slot < 0 ? S + (pair0 + j) * k : ws + ((size_t) it.slot * T + t0 + j) * k;
#pragma unroll
        for (int i = 0; i < C; ++i)
            if (64 * i + lane < k) s[64 * i + lane] = acc[j][i];
    }
}

// the partial slots of a split row into S [seg T + t][k], in slot order; one wavefront per (split row, target)
__global__ __launch_bounds__(64) void k_explcg_reduce(const AlsReduce* __restrict__ reduces, uint32_t nreduces, uint32_t k, uint32_t T,
                                                      const uint32_t* __restrict__ frozen, const float* __restrict__ ws, float* __restrict__ S) {
    if (blockIdx.x >= nreduces) return;
    const AlsReduce rd = reduces[blockIdx.x];
    const uint32_t t = blockIdx.y;
    const size_t pair = (size_t) rd.seg * T + t;
    if (frozen[pair]) return;
    for (uint32_t c = threadIdx.x & 63; c < k; c += 64) {
        float s = 0.f;
        for (uint32_t p = 0; p < rd.nslots; ++p) s += ws[((size_t) (rd.slot0 + p) * T + t) * k + c];
        S[pair * k + c] = s;
    }
}

// One wavefront per pair, lane l the columns l + 64 i.  A padding target, a row without counting entries (implicit: no r > 0;
// explicit: no entry) or h_t = 0: z = 0, frozen, 0 steps.  Any other pair: r = h_t (z is zero), |h_t|^2 kept, frozen at once if
// tol > 0 and |r| <= tol |h_t|.  r, the preconditioned residual and p of a frozen pair are zeroed so that nothing unwritten is
// ever read.  (explicit: Zp is R)
__global__ __launch_bounds__(256) void k_explcg_start(const uint32_t* __restrict__ ptr, const float* __restrict__ val, size_t npair, uint32_t T,
                                                      uint32_t k, const uint32_t* __restrict__ targets, const float* __restrict__ X,
                                                      int32_t implicit, float* __restrict__ Z, float* R, float* Zp, float* __restrict__ P,
                                                      float tol, float* __restrict__ bb, uint32_t* __restrict__ frozen,
                                                      int32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t pair = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npair) return;
    const uint32_t seg = (uint32_t) (pair / T), tg = targets[pair];
    const size_t o = pair * k;
    const uint32_t lo = ptr[seg], hi = ptr[seg + 1];
    bool counting = hi > lo;
    if (implicit) {
        bool any = false;
        for (uint32_t e = lo + lane; e < hi; e += 64) any = any || val[e] > 0.f;
        counting = __any(any);
    }
    float b2 = 0.f;
    if (counting && tg != kPadTarget) {
        const float* h = X + (size_t) tg * k;
        for (uint32_t c = lane; c < k; c += 64) {
            const float v = h[c];
            R[o + c] = v;
            b2 = __builtin_fmaf(v, v, b2);
        }
        b2 = wave_sum(b2);
    }
    if (b2 == 0.f) {
        for (uint32_t c = lane; c < k; c += 64) Z[o + c] = R[o + c] = Zp[o + c] = P[o + c] = 0.f;
        if (lane == 0) { frozen[pair] = 1; counts[pair] = 0; bb[pair] = 0.f; }
        return;
    }
    const bool stop = tol > 0.f && sqrtf(b2) <= tol * sqrtf(b2);
    if (stop)
        for (uint32_t c = lane; c < k; c += 64) Zp[o + c] = P[o + c] = 0.f;
    if (lane == 0) { frozen[pair] = stop; counts[pair] = 0; bb[pair] = b2; }
}

// k_foldcg_step over the pairs: rho is that of the pair's row.  <p, q> < 0 or not finite: the pair's z becomes NaN and is
// frozen, the step counted; <p, q> exactly 0: frozen as it is, the step not counted.
__global__ __launch_bounds__(256) void k_explcg_step(const uint32_t* __restrict__ ptr, size_t npair, uint32_t T, uint32_t k,
                                                     float* __restrict__ Z, float* __restrict__ R, const float* __restrict__ P,
                                                     const float* __restrict__ Q, int32_t reg, float lambda, float tol,
                                                     const float* __restrict__ gamma, const float* __restrict__ bb,
                                                     uint32_t* __restrict__ frozen, int32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t pair = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npair || frozen[pair]) return;  // wave-uniform
    const size_t o = pair * k;
    const float rho = reg ? row_rho(reg, lambda, ptr, (uint32_t) (pair / T)) : 0.f;
    float pq = 0.f;
    for (uint32_t c = lane; c < k; c += 64) {
        const float q = reg ? __builtin_fmaf(rho, P[o + c], Q[o + c]) : Q[o + c];
        pq = __builtin_fmaf(P[o + c], q, pq);
    }
    pq = wave_sum(pq);
    if (!(pq >= 0.f) || !(pq <= 3.402823466e38f)) {
        for (uint32_t c = lane; c < k; c += 64) Z[o + c] = __builtin_nanf("");
        if (lane == 0) { frozen[pair] = 1; counts[pair] += 1; }
        return;
    }
    if (pq == 0.f) {
        if (lane == 0) frozen[pair] = 1;
        return;
    }
    const float a = gamma[pair] / pq;
    float r2 = 0.f;
    for (uint32_t c = lane; c < k; c += 64) {
        const float p = P[o + c];
        const float q = reg ? __builtin_fmaf(rho, p, Q[o + c]) : Q[o + c];
        Z[o + c] = __builtin_fmaf(a, p, Z[o + c]);
        const float r = __builtin_fmaf(-a, q, R[o + c]);
        R[o + c] = r;
        r2 = __builtin_fmaf(r, r, r2);
    }
    r2 = wave_sum(r2);
    if (lane == 0) {
        counts[pair] += 1;
        if (tol > 0.f && sqrtf(r2) <= tol * sqrtf(bb[pair])) frozen[pair] = 1;
    }
}

// k_foldcg_dir over the pairs (explicit: Zp is R): gamma' = <r, zp>; first: p = zp, else p = zp + (gamma' / gamma) p.
// gamma' exactly 0 freezes the pair.  The pairs still active are counted into *active (NULL: no count; an integer atomic).
__global__ __launch_bounds__(256) void k_explcg_dir(size_t npair, uint32_t k, const float* __restrict__ R, const float* __restrict__ Zp,
                                                    float* __restrict__ P, int32_t first, float* __restrict__ gamma,
                                                    uint32_t* __restrict__ frozen, uint32_t* __restrict__ active) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t pair = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npair || frozen[pair]) return;  // wave-uniform
    const size_t o = pair * k;
    float g = 0.f;
    for (uint32_t c = lane; c < k; c += 64) g = __builtin_fmaf(R[o + c], Zp[o + c], g);
    g = wave_sum(g);
    if (g == 0.f) {
        if (lane == 0) frozen[pair] = 1;
        return;
    }
    if (first) {
        for (uint32_t c = lane; c < k; c += 64) P[o + c] = Zp[o + c];
    } else {
        const float beta = g / gamma[pair];
        for (uint32_t c = lane; c < k; c += 64) P[o + c] = __builtin_fmaf(beta, P[o + c], Zp[o + c]);
    }
    if (lane == 0) {
        gamma[pair] = g;
        if (active) atomicAdd(active, 1u);
    }
}

// Targets per wavefront for C = ceil(k / 64) columns per lane: four rows of H (4 C registers) plus 2 C per target stay within
// 128 VGPRs without scratch (the compiler's report: profiles/).  At C = 16 the four rows and one target fill the budget.
template <int C, int TG>
void launch_gather(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, int32_t implicit, float alpha, uint32_t T, const float* P,
                   const uint32_t* frozen, float* S, float* ws, hipStream_t st) {
    hipLaunchKernelGGL((k_explcg_gather<C, TG>), dim3(h.nitems, (T + TG - 1) / TG), dim3(64), 0, st, h.items.get(), h.nitems, h.idx.get(),
                       h.val.get(), X, x_rows, k, implicit, alpha, T, P, frozen, S, ws);
}

// the gather pass and, where a row was split, the sum of its slots
int gather(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, int32_t implicit, float alpha, uint32_t T, const float* P,
           const uint32_t* frozen, float* S, float* ws, hipStream_t st) {
    const uint32_t c = (k + 63) / 64;
    if (c <= 1) launch_gather<1, 16>(h, X, x_rows, k, implicit, alpha, T, P, frozen, S, ws, st);
    else if (c <= 2) launch_gather<2, 16>(h, X, x_rows, k, implicit, alpha, T, P, frozen, S, ws, st);
    else if (c <= 4) launch_gather<4, 8>(h, X, x_rows, k, implicit, alpha, T, P, frozen, S, ws, st);
    else if (c <= 8) launch_gather<8, 4>(h, X, x_rows, k, implicit, alpha, T, P, frozen, S, ws, st);
    else launch_gather<16, 1>(h, X, x_rows, k, implicit, alpha, T, P, frozen, S, ws, st);
    MFX_HIP(hipGetLastError());
    if (h.nreduces) {
        hipLaunchKernelGGL(k_explcg_reduce, dim3(h.nreduces, T), dim3(64), 0, st, h.reduces.get(), h.nreduces, k, T, frozen, ws, S);
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

}  // namespace

int explaincg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, const FoldCg& m, const uint32_t* targets,
                     uint32_t n_targets, float* Z, int32_t* counts, hipStream_t st) {
    const uint32_t T = n_targets;
    const size_t npair = (size_t) h.nseg * T;
    if (npair == 0) return MFX_OK;
    MFX_REQUIRE(npair < ((size_t) 1 << 31), "explanations by conjugate gradients: %zu (row, target) pairs in one call (fewer than 2^31)", npair);
    const bool implicit = m.reg == 0;
    MFX_REQUIRE(!implicit || (m.G && m.Minv), "explanations by conjugate gradients: the implicit model needs G and Minv");
    const size_t nk = npair * k;
    const uint32_t np32 = (uint32_t) npair;
    DevBuf<float> R, Zb, P, Q, ws, bb, gamma;
    DevBuf<uint32_t> frozen, active;  // active [1 + steps]: the pairs still active after the start and after each step
    DevBuf<int32_t> own_counts;
    MFX_TRY(R.alloc(nk));
    MFX_TRY(P.alloc(nk));
    MFX_TRY(Q.alloc(nk));
    if (implicit) MFX_TRY(Zb.alloc(nk));
    MFX_TRY(ws.alloc(std::max<size_t>(1, (size_t) h.nslots * T * k)));
    MFX_TRY(bb.alloc(npair));
    MFX_TRY(gamma.alloc(npair));
    MFX_TRY(frozen.alloc(npair));
    const bool stop = m.tol > 0.f;
    if (stop) MFX_TRY(active.alloc_zero((size_t) m.steps + 1, st));
    if (!counts) {
        MFX_TRY(own_counts.alloc(npair));
        counts = own_counts.get();
    }
    float* Zp = implicit ? Zb.get() : R.get();  // the explicit models' preconditioner is the identity
    const dim3 grid((np32 + 3) / 4), block(256);
    auto all_frozen = [&](uint32_t slot, bool& done) -> int {
        uint32_t left = 0;
        MFX_HIP(hipMemcpyAsync(&left, active.get() + slot, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        done = left == 0;
        return MFX_OK;
    };

    hipLaunchKernelGGL(k_explcg_start, grid, block, 0, st, h.ptr.get(), h.val.get(), npair, T, k, targets, X, (int32_t) implicit, Z, R.get(), Zp,
                       P.get(), m.tol, bb.get(), frozen.get(), counts);
    MFX_HIP(hipGetLastError());
    if (implicit) MFX_TRY(foldcg_dense(R.get(), np32, k, m.Minv, frozen.get(), nullptr, Zp, st));
    hipLaunchKernelGGL(k_explcg_dir, grid, block, 0, st, npair, k, R.get(), Zp, P.get(), 1, gamma.get(), frozen.get(), active.get());
    MFX_HIP(hipGetLastError());
    bool done = false;
    if (stop) MFX_TRY(all_frozen(0, done));
    for (int32_t s = 0; s < m.steps && !done; ++s) {
        MFX_TRY(gather(h, X, x_rows, k, implicit, m.alpha, T, P.get(), frozen.get(), Q.get(), ws.get(), st));
        if (implicit) MFX_TRY(foldcg_dense(P.get(), np32, k, m.G, frozen.get(), Q.get(), Q.get(), st));
        hipLaunchKernelGGL(k_explcg_step, grid, block, 0, st, h.ptr.get(), npair, T, k, Z, R.get(), P.get(), Q.get(), m.reg, m.lambda, m.tol,
                           gamma.get(), bb.get(), frozen.get(), counts);
        MFX_HIP(hipGetLastError());
        if (s + 1 == m.steps) break;  // (the direction of a step that never comes)
        if (implicit) MFX_TRY(foldcg_dense(R.get(), np32, k, m.Minv, frozen.get(), nullptr, Zp, st));
        hipLaunchKernelGGL(k_explcg_dir, grid, block, 0, st, npair, k, R.get(), Zp, P.get(), 0, gamma.get(), frozen.get(),
                           stop ? active.get() + s + 1 : nullptr);
        MFX_HIP(hipGetLastError());
        if (stop) MFX_TRY(all_frozen((uint32_t) s + 1, done));
    }
    MFX_HIP(hipStreamSynchronize(st));  // (the workspace goes with this call)
    return MFX_OK;
}

}  // namespace mfx
