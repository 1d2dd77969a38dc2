// ease_inverse.hip -- mfx_ease_inverse: the blocked SPD inverse of spd_inverse.hip for 1 <= n <= 32768 (nb = ceil(n / 32) <=
// 1024 blocks), on gfx950.  The algorithm, its padded copy and its three workspaces A, T, M are those stated at the top of
// spd_inverse.hip; every block product is the same chain of v_mfma_f32_32x32x2_f32 over the summed index, ascending, so the
// bits of the result are fixed by (G, n).  Two schedules of the same chains:
//   simple   (MFX_EASE_INV_SIMPLE) the kernels of spd_device.hpp as spd_inverse_launch queues them: one wavefront per block,
//            operands from global memory.  4 nb launches.
//   grouped  (default) a workgroup of 4 waves owns 4 x 4 blocks of output; wave w owns block row w of the group and keeps
//            its four accumulators in registers across the summed index.  Per step of the summed index the four operand
//            blocks of the rows and the four of the columns are staged in LDS once (row stride 33: no bank conflicts in
//            either orientation) and every wave multiplies from there.
//     Cholesky  left-looking by groups of four block columns: k_ease_trail_g applies the steps j < p0 to the columns
//               p0 .. p0 + 3 in one pass (j ascending, the accumulator carried in registers: storing and reloading fp32
//               between steps is lossless), then the four columns are finished by k_spd_diag, k_spd_panel and
//               k_ease_trail_cols, the one-wave trailing update restricted to the columns of the group.  Every element of A
//               still sees j = 0, 1, 2, ... in order, each step the same 16 MFMAs.
//     T = L^-1  by groups of four block rows, ascending: k_ease_tinv_g sums t from the group's first column to the row
//               group's start from LDS stages, then the four rows of the group in order: the wave of row t is complete when
//               step t begins, stores T_tj and hands it to the rows below through LDS.
//     T^T T     k_ease_prod_g, one launch.
//   k_spd_diag, k_spd_panel and k_spd_scale stay one wave per block.  Stream order only; no float atomics.
#include "als_solver.hpp"
#include "ease.hpp"

namespace mfx {
namespace {
constexpr uint32_t kSpdB = 32;
}  // namespace
}  // namespace mfx

#include "spd_device.hpp"

namespace mfx {
namespace {

constexpr uint32_t kGrp = 4;                 // blocks per side of a group, and waves of its workgroup
constexpr uint32_t kGrpThreads = 64 * kGrp;
constexpr uint32_t kGrpLd = 33;              // floats per row of a staged block
constexpr uint32_t kGrpBlk = 32 * kGrpLd;

// One 32 x 32 block of a matrix with row stride kp into LDS, by the whole workgroup (a float4 per thread).
__device__ __forceinline__ void stage_block(float* __restrict__ dst, const float* __restrict__ src, uint32_t kp) {
    const uint32_t r = threadIdx.x >> 3, c = (threadIdx.x & 7) * 4;
    const float4 v = *reinterpret_cast<const float4*>(src + (size_t) r * kp + c);
    float* d = dst + r * kGrpLd + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
}

__device__ __forceinline__ const float* block_of(const float* m, uint32_t kp, uint32_t bi, uint32_t bj) {
    return m + (size_t) (bi * kSpdB) * kp + bj * kSpdB;
}
__device__ __forceinline__ float* block_of(float* m, uint32_t kp, uint32_t bi, uint32_t bj) {
    return m + (size_t) (bi * kSpdB) * kp + bj * kSpdB;
}

// A_ip -= sum_{j < p0} L_ij L_pj^T (j ascending) for the columns p = p0 + c of column group pg and the rows i >= p of row
// group pg + blockIdx.x.
__global__ __launch_bounds__(kGrpThreads) void k_ease_trail_g(float* __restrict__ A, uint32_t kp, uint32_t nb, uint32_t pg) {
    __shared__ float P[kGrp][kGrpBlk], Q[kGrp][kGrpBlk];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, c31 = lane & 31, h = lane >> 5;
    const uint32_t p0 = pg * kGrp, i0 = (pg + blockIdx.x) * kGrp, i = i0 + w;
    f32x16 acc[kGrp];
    bool on[kGrp];
#pragma unroll
    for (uint32_t c = 0; c < kGrp; ++c) {
        const uint32_t p = p0 + c;
        on[c] = i < nb && p < nb && p <= i;
        if (on[c]) {
            const float* Aip = block_of(A, kp, i, p);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][r] = Aip[(size_t) acc_row(r, h) * kp + c31];
        }
    }
    for (uint32_t j = 0; j < p0; ++j) {
        __syncthreads();  // (the stages of the step before have been read)
#pragma unroll
        for (uint32_t g = 0; g < kGrp; ++g) {
            if (i0 + g < nb) stage_block(P[g], block_of(A, kp, i0 + g, j), kp);
            if (p0 + g < nb) stage_block(Q[g], block_of(A, kp, p0 + g, j), kp);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t c = 0; c < kGrp; ++c)
            if (on[c]) tile_mac<false, false>(acc[c], P[w], Q[c], kGrpLd, -1.f, c31, h);
    }
#pragma unroll
    for (uint32_t c = 0; c < kGrp; ++c)
        if (on[c]) tile_store(acc[c], block_of(A, kp, i, p0 + c), kp, c31, h);
}

// A_ip -= L_ij L_pj^T for the columns j < p <= pend and the rows i >= p: k_spd_trail on the columns of j's own group.
__global__ __launch_bounds__(64) void k_ease_trail_cols(float* __restrict__ A, uint32_t kp, uint32_t nb, uint32_t j, uint32_t pend) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    uint32_t p = j + 1, t = blockIdx.x;
    while (p <= pend && t >= nb - p) { t -= nb - p; ++p; }
    if (p > pend) return;
    const uint32_t i = p + t;
    float* Aip = block_of(A, kp, i, p);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = Aip[(size_t) acc_row(r, h) * kp + c31];
    tile_mac<false, false>(acc, block_of(A, kp, i, j), block_of(A, kp, p, j), kp, -1.f, c31, h);
    tile_store(acc, Aip, kp, c31, h);
}

// T_ij = -sum_{t = j .. i - 1} M_it T_tj (t ascending) for the rows i = 4 ig + w and the columns j = 4 blockIdx.x + c, j < i.
// The rows above the group are done (earlier launches); the group's own rows follow one another inside the workgroup.
__global__ __launch_bounds__(kGrpThreads) void k_ease_tinv_g(const float* __restrict__ M, float* T, uint32_t kp, uint32_t nb, uint32_t ig) {
    __shared__ float P[kGrp][kGrpBlk], Q[kGrp][kGrpBlk];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, c31 = lane & 31, h = lane >> 5;
    const uint32_t jg = blockIdx.x, i0 = ig * kGrp, j0 = jg * kGrp, i = i0 + w;
    f32x16 acc[kGrp];
#pragma unroll
    for (uint32_t c = 0; c < kGrp; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    for (uint32_t t = j0; t < i0; ++t) {  // (t < i0 <= i: M_it is a block of the strict lower triangle)
        __syncthreads();
#pragma unroll
        for (uint32_t g = 0; g < kGrp; ++g) {
            if (i0 + g < nb) stage_block(P[g], block_of(M, kp, i0 + g, t), kp);
            if (j0 + g <= t) stage_block(Q[g], block_of(T, kp, t, j0 + g), kp);
        }
        __syncthreads();
        if (i < nb) {
#pragma unroll
            for (uint32_t c = 0; c < kGrp; ++c)
                if (j0 + c <= t) tile_mac<false, true>(acc[c], P[w], Q[c], kGrpLd, -1.f, c31, h);
        }
    }
    for (uint32_t tt = 0; tt < kGrp; ++tt) {
        const uint32_t t = i0 + tt;
        if (t >= nb) break;
        __syncthreads();
        if (w == tt) {  // row t has seen every step below t: its blocks left of the diagonal are final
#pragma unroll
            for (uint32_t c = 0; c < kGrp; ++c)
                if (j0 + c < t) {
                    tile_store(acc[c], block_of(T, kp, t, j0 + c), kp, c31, h);
                    tile_store(acc[c], Q[c], kGrpLd, c31, h);
                }
        }
        if (jg == ig) stage_block(Q[tt], block_of(T, kp, t, t), kp);  // (the diagonal block, from k_spd_diag)
#pragma unroll
        for (uint32_t g = 0; g < kGrp; ++g)
            if (g > tt && i0 + g < nb) stage_block(P[g], block_of(M, kp, i0 + g, t), kp);
        __syncthreads();
        if (w > tt && i < nb) {
#pragma unroll
            for (uint32_t c = 0; c < kGrp; ++c)
                if (j0 + c <= t) tile_mac<false, true>(acc[c], P[w], Q[c], kGrpLd, -1.f, c31, h);
        }
    }
}

// Minv blocks (a, b) = (4 ag + w, 4 bg + c), a <= b (blockIdx.x: the pair (bg, ag) of lower_of): sum_{t >= b} T_ta^T T_tb,
// t ascending, written as k_spd_prod writes it.
__global__ __launch_bounds__(kGrpThreads) void k_ease_prod_g(const float* __restrict__ T, uint32_t kp, uint32_t nb, uint32_t k,
                                                             float* __restrict__ Minv) {
    __shared__ float P[kGrp][kGrpBlk], Q[kGrp][kGrpBlk];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, c31 = lane & 31, h = lane >> 5;
    uint32_t ag, bg;
    lower_of(blockIdx.x, bg, ag);
    const uint32_t a0 = ag * kGrp, b0 = bg * kGrp, a = a0 + w;
    f32x16 acc[kGrp];
#pragma unroll
    for (uint32_t c = 0; c < kGrp; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    for (uint32_t t = b0; t < nb; ++t) {
        __syncthreads();
#pragma unroll
        for (uint32_t g = 0; g < kGrp; ++g) {  // (only blocks of the lower triangle of T hold anything)
            if (a0 + g <= t) stage_block(P[g], block_of(T, kp, t, a0 + g), kp);
            if (b0 + g <= t) stage_block(Q[g], block_of(T, kp, t, b0 + g), kp);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t c = 0; c < kGrp; ++c) {
            const uint32_t b = b0 + c;
            if (a <= b && b <= t) tile_mac<true, true>(acc[c], P[w], Q[c], kGrpLd, 1.f, c31, h);
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < kGrp; ++c) {
        const uint32_t b = b0 + c, col = b * kSpdB + c31;
        if (a > b || b >= nb) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row = a * kSpdB + acc_row(r, h);
            if (row >= k || col >= k || row > col) continue;
            Minv[(size_t) row * k + col] = acc[c][r];
            Minv[(size_t) col * k + row] = acc[c][r];
        }
    }
}

int launch_simple(float* A, float* T, float* M, uint32_t k, uint32_t kp, uint32_t nb, float* Minv, uint32_t* fail, hipStream_t st) {
    for (uint32_t j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(k_spd_diag, dim3(1), dim3(64), 0, st, A, T, kp, j, fail, nb == 1 ? Minv : nullptr, k);
        MFX_HIP(hipGetLastError());
        const uint32_t left = nb - j - 1;
        if (!left) break;
        hipLaunchKernelGGL(k_spd_panel, dim3(left), dim3(64), 0, st, A, T, kp, j);
        MFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_spd_trail, dim3(left * (left + 1) / 2), dim3(64), 0, st, A, kp, j);
        MFX_HIP(hipGetLastError());
    }
    if (nb == 1) return MFX_OK;
    hipLaunchKernelGGL(k_spd_scale, dim3(nb * (nb - 1) / 2), dim3(64), 0, st, A, T, kp, M);
    MFX_HIP(hipGetLastError());
    for (uint32_t s = 1; s < nb; ++s) {
        hipLaunchKernelGGL(k_spd_tinv, dim3(nb - s), dim3(64), 0, st, M, T, kp, s);
        MFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_spd_prod, dim3(nb * (nb + 1) / 2), dim3(64), 0, st, T, kp, nb, k, Minv);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int launch_grouped(float* A, float* T, float* M, uint32_t k, uint32_t kp, uint32_t nb, float* Minv, uint32_t* fail, hipStream_t st) {
    const uint32_t ng = (nb + kGrp - 1) / kGrp;
    for (uint32_t pg = 0; pg < ng; ++pg) {
        const uint32_t p0 = pg * kGrp, pend = std::min(p0 + kGrp, nb) - 1;
        if (pg > 0) {
            hipLaunchKernelGGL(k_ease_trail_g, dim3(ng - pg), dim3(kGrpThreads), 0, st, A, kp, nb, pg);
            MFX_HIP(hipGetLastError());
        }
        for (uint32_t j = p0; j <= pend; ++j) {
            hipLaunchKernelGGL(k_spd_diag, dim3(1), dim3(64), 0, st, A, T, kp, j, fail, nb == 1 ? Minv : nullptr, k);
            MFX_HIP(hipGetLastError());
            const uint32_t left = nb - j - 1;
            if (!left) break;
            hipLaunchKernelGGL(k_spd_panel, dim3(left), dim3(64), 0, st, A, T, kp, j);
            MFX_HIP(hipGetLastError());
            uint32_t blocks = 0;
            for (uint32_t p = j + 1; p <= pend; ++p) blocks += nb - p;
            if (blocks) {
                hipLaunchKernelGGL(k_ease_trail_cols, dim3(blocks), dim3(64), 0, st, A, kp, nb, j, pend);
                MFX_HIP(hipGetLastError());
            }
        }
    }
    if (nb == 1) return MFX_OK;
    hipLaunchKernelGGL(k_spd_scale, dim3(nb * (nb - 1) / 2), dim3(64), 0, st, A, T, kp, M);
    MFX_HIP(hipGetLastError());
    for (uint32_t ig = 0; ig < ng; ++ig) {
        hipLaunchKernelGGL(k_ease_tinv_g, dim3(ig + 1), dim3(kGrpThreads), 0, st, M, T, kp, nb, ig);
        MFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ease_prod_g, dim3(ng * (ng + 1) / 2), dim3(kGrpThreads), 0, st, T, kp, nb, k, Minv);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

}  // namespace

size_t ease_inverse_ws_floats(uint32_t n) { return (size_t) 3 * spd_kp(n) * spd_kp(n); }

int ease_inverse_launch(const float* G, uint32_t n, float* Minv, float* ws, uint32_t* fail, int flags, hipStream_t st) {
    MFX_REQUIRE(n >= 1 && n <= kEaseMaxCols, "EASE inverse: n = %u not supported (1 <= n <= %u)", n, kEaseMaxCols);
    const uint32_t kp = spd_kp(n), nb = kp / kSpdB;
    float *A = ws, *T = ws + (size_t) kp * kp, *M = ws + (size_t) 2 * kp * kp;
    hipLaunchKernelGGL(k_spd_copy, dim3((kp * kp + 255) / 256), dim3(256), 0, st, G, n, kp, A);
    MFX_HIP(hipGetLastError());
    return (flags & MFX_EASE_INV_SIMPLE) ? launch_simple(A, T, M, n, kp, nb, Minv, fail, st) : launch_grouped(A, T, M, n, kp, nb, Minv, fail, st);
}

}  // namespace mfx
