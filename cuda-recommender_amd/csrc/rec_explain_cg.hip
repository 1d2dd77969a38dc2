// rec_explain_cg.hip -- the target solves of mfx_rec_explain_cg on gfx950: A_q z = h_t for every query row q and every target
// t of its slot, by the preconditioned conjugate gradients of rec_foldin_cg.hip (the operator, the preconditioner, the
// recurrence and the stop rule of row q), ranks up to 1024.
// The systems are the pairs (q, t), rows q T + t of [nu T][k] arrays: z (the caller's Z), r, the preconditioned residual
// (implicit), p and A p; |h_t|^2, gamma, the step count and the frozen flag live per pair.  The method is the shared one of
// rec_foldin_cg.hpp with T systems per row: k_cg_reduce, k_foldcg_dense, k_cg_step, k_cg_dir and the step loop
// cg_iterate are those of fold-in.  What is this unit's own:
//   k_explcg_start          r = h_t, |h_t|^2; a padding target, a row without counting entries, h_t = 0: zero, frozen, 0 steps
//   k_cg_gather<C, TG, 1>   with TG targets per wavefront: an entry's row of H is loaded ONCE for the group; per target the
//                           very operation order of fold-in's <C, 1, 1>, so a pair's bits depend neither on TG nor on the
//                           other targets of its slot.  A group of frozen targets does no gathering.
#include <algorithm>

#include "rec_foldin_cg.hpp"

namespace mfx {
namespace {

constexpr uint32_t kPadTarget = 0xFFFFFFFFu;

// One wavefront per pair, lane l the columns l + 64 i.  A pair with a target and a row with counting entries (implicit: some
// r > 0; explicit: any entry): r = h_t (z is zero); then cg_start_tail (every other pair has b2 = 0 there).  (explicit: Zp is R)
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
    cg_start_tail(pair, o, k, lane, b2, b2, tol, Z, R, Zp, P, bb, frozen, counts);
}

// Targets per wavefront for C = ceil(k / 64) columns per lane: four rows of H (4 C registers) plus 2 C per target stay within
// 128 VGPRs without scratch (the compiler's report: profiles/).  At C = 16 the four rows and one target fill the budget.
template <int C, int TG>
void launch_gather(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, int32_t implicit, float alpha, uint32_t T, const float* P,
                   const uint32_t* frozen, float* S, float* ws, hipStream_t st) {
    hipLaunchKernelGGL((k_cg_gather<C, TG, 1>), dim3(h.nitems, (T + TG - 1) / TG), dim3(64), 0, st, h.items.get(), h.nitems, h.idx.get(),
                       h.val.get(), X, x_rows, k, implicit, alpha, T, P, frozen, S, nullptr, ws);
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
    return cg_reduce(h, k, T, 1, frozen, ws, S, nullptr, st);
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
    FoldCgWs w;  // the call's own vectors, one row per pair
    DevBuf<int32_t> own_counts;
    MFX_TRY(w.R.alloc(nk));
    MFX_TRY(w.P.alloc(nk));
    MFX_TRY(w.Q.alloc(nk));
    if (implicit) MFX_TRY(w.Z.alloc(nk));
    MFX_TRY(w.part.alloc(std::max<size_t>(1, (size_t) h.nslots * T * k)));
    MFX_TRY(w.bb.alloc(npair));
    MFX_TRY(w.gamma.alloc(npair));
    MFX_TRY(w.frozen.alloc(npair));
    if (m.tol > 0.f) MFX_TRY(w.active.alloc_zero((size_t) m.steps + 1, st));
    if (!counts) {
        MFX_TRY(own_counts.alloc(npair));
        counts = own_counts.get();
    }
    float* Zp = implicit ? w.Z.get() : w.R.get();  // the explicit models' preconditioner is the identity
    hipLaunchKernelGGL(k_explcg_start, dim3(((uint32_t) npair + 3) / 4), dim3(256), 0, st, h.ptr.get(), h.val.get(), npair, T, k, targets, X,
                       (int32_t) implicit, Z, w.R.get(), Zp, w.P.get(), m.tol, w.bb.get(), w.frozen.get(), counts);
    MFX_HIP(hipGetLastError());
    // (the first direction is handed w.active as it is: NULL when tol = 0, where it was never allocated)
    return cg_iterate(h, T, k, m, Z, w, counts, nullptr, w.active.get(), [&] {
        return gather(h, X, x_rows, k, implicit, m.alpha, T, w.P.get(), w.frozen.get(), w.Q.get(), w.part.get(), st);
    }, st);
}

}  // namespace mfx
