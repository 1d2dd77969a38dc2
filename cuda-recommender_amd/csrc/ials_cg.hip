// ials_cg.hip -- implicit ALS by preconditioned conjugate gradients (mfx_ials_cg_create, mfx_ials_cg_half), any
// rank up to 1024.  A half-sweep over the fixed side X is three things on one stream: G = X^T X + lambda I (ialsb_gramian),
// Minv ~ G^-1 on the device (spd_inverse_launch), and the method of rec_foldin_cg.hip (foldcg_launch) in place on the side
// being solved, every row from its current value: each row's system is G plus a matrix of the rank of the row, so CG
// preconditioned by Minv ends after n + 1 steps on a row of n entries, and a warm row after fewer.  The kernels are those of
// rec_foldin_cg.hip and spd_inverse.hip; this file adds the count of what the half did.
#include <algorithm>

#include "als_solver.hpp"

namespace mfx {
namespace {

// stats[0] += the steps of every row, stats[1] = the most steps of a row, stats[2] += the rows still active at the end (they
// used every step without meeting tol; count_open = tol > 0).  Integer atomics: the sums have no order.
__global__ __launch_bounds__(256) void k_ialscg_stats(const int32_t* __restrict__ counts, const uint32_t* __restrict__ frozen, uint32_t nseg,
                                                      int32_t count_open, unsigned long long* __restrict__ stats) {
    const uint32_t seg = blockIdx.x * 256 + threadIdx.x;
    unsigned long long c = 0, open = 0;
    if (seg < nseg) {
        c = (unsigned long long) counts[seg];
        open = count_open && !frozen[seg];
    }
    unsigned long long sum = c, mx = c, op = open;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        op += __shfl_xor(op, o, 64);
        const unsigned long long other = __shfl_xor(mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        if (sum) atomicAdd(stats, sum);
        if (mx) atomicMax(stats + 1, mx);
        if (op) atomicAdd(stats + 2, op);
    }
}

}  // namespace

int IalsCg::alloc(uint32_t k_, uint32_t max_rows_x, uint32_t max_seg, uint32_t nslots, int32_t steps) {
    k = k_;
    MFX_TRY(gb.alloc_gramian(k, max_rows_x));
    MFX_TRY(Minv.alloc((size_t) k * k));
    MFX_TRY(inv_ws.alloc(spd_inverse_ws_floats(k)));
    MFX_TRY(ws.alloc(max_seg, k, nslots, steps));
    return counts.alloc(std::max<uint32_t>(1, max_seg));
}

int ialscg_half_launch(IalsCg& c, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, bool warm, float lambda, float alpha,
                       int32_t steps, float tol, uint32_t* fails, unsigned long long* stats, hipEvent_t ev_gram, hipEvent_t ev_inv,
                       hipStream_t st) {
    MFX_HIP(hipMemsetAsync(stats, 0, sizeof(unsigned long long) * 3, st));
    MFX_TRY(ialsb_gramian(c.gb, X, x_rows, lambda, st));
    if (ev_gram) MFX_HIP(hipEventRecord(ev_gram, st));
    MFX_TRY(spd_inverse_launch(c.gb.G.get(), c.k, c.Minv.get(), c.inv_ws.get(), fails, st));
    if (ev_inv) MFX_HIP(hipEventRecord(ev_inv, st));
    if (h.nseg == 0) return MFX_OK;
    MFX_REQUIRE(c.counts.size() >= h.nseg, "implicit ALS by conjugate gradients: workspace too small for this half");
    FoldCg m;
    m.reg = 0;
    m.lambda = lambda;
    m.alpha = alpha;
    m.G = c.gb.G.get();
    m.Minv = c.Minv.get();
    m.steps = steps;
    m.tol = tol;
    MFX_TRY(foldcg_launch(h, X, x_rows, c.k, m, Y, warm, c.counts.get(), fails + 1, st, &c.ws));
    hipLaunchKernelGGL(k_ialscg_stats, dim3((h.nseg + 255) / 256), dim3(256), 0, st, c.counts.get(), c.ws.frozen.get(), h.nseg,
                       (int32_t) (tol > 0.f), stats);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

}  // namespace mfx
