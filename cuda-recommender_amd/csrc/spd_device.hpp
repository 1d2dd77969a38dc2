// spd_device.hpp -- the device side of the blocked SPD inverse (the algorithm is stated at the top of spd_inverse.hip): the
// 32 x 32 MFMA tile product and the one-wavefront-per-block kernels.  Everything here sits in an anonymous namespace: each
// unit compiles its own copy, as spd_inverse.hip did while this text was part of it.  spd_inverse.hip (k <= 1024) and
// ease_inverse.hip (the same kernels with the cap lifted, and their grouped siblings) include it, each after defining the
// block width kSpdB in mfx's anonymous namespace.
#pragma once

#include "common.hpp"

namespace mfx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

static_assert(kSpdB == 32, "the including unit defines kSpdB, the block width, before this header: the MFMA tiles are 32 x 32");

// A = G on [k][k], the identity on the tail up to kp
__global__ __launch_bounds__(256) void k_spd_copy(const float* __restrict__ G, uint32_t k, uint32_t kp, float* __restrict__ A) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kp * kp) return;
    const uint32_t r = e / kp, c = e - r * kp;
    A[e] = r < k && c < k ? G[(size_t) r * k + c] : r == c ? 1.f : 0.f;
}

// row of the accumulator register r of lane half h (the column is the lane's c31)
__device__ __forceinline__ uint32_t acc_row(int r, uint32_t h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// acc[i][j] += sum_{t < 32} sa * P(i, t) * Q(j, t) with t ascending (lane half h takes t = 2 u + h in step u).  PT: P(i, t)
// is p[t * ld + i] (the summed index is the row of the stored block), else p[i * ld + t]; QT likewise for Q.
template <bool PT, bool QT>
__device__ __forceinline__ void tile_mac(f32x16& acc, const float* __restrict__ p, const float* __restrict__ q, uint32_t ld, float sa,
                                         uint32_t c31, uint32_t h) {
    float a[16], b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const uint32_t t = 2 * u + h;
        a[u] = sa * (PT ? p[(size_t) t * ld + c31] : p[(size_t) c31 * ld + t]);
        b[u] = QT ? q[(size_t) t * ld + c31] : q[(size_t) c31 * ld + t];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
}

__device__ __forceinline__ void tile_store(const f32x16& acc, float* __restrict__ o, uint32_t ld, uint32_t c31, uint32_t h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(size_t) acc_row(r, h) * ld + c31] = acc[r];
}

// pair t of the lower block triangle of n block rows in the order (0,0), (1,0), (1,1), (2,0), ...: i >= p
__device__ __forceinline__ void lower_of(uint32_t t, uint32_t& i, uint32_t& p) {
    uint32_t r = 0;
    while (t > r) { t -= r + 1; ++r; }
    i = r; p = t;
}

// The diagonal block j of A: L_jj by Cholesky and T_jj = L_jj^-1, both in fp64, rounded into A (upper part zero) and T.
// One wavefront; thread (r, half) updates row r of the trailing part of the block, every other column each; thread c < 32
// then inverts column c of L from registers.  single (kp == 32): Minv = T^T T in fp64 on [k][k], nothing else follows.
__global__ __launch_bounds__(64) void k_spd_diag(float* __restrict__ A, float* __restrict__ T, uint32_t kp, uint32_t j, uint32_t* __restrict__ fail,
                                                 float* __restrict__ Minv, uint32_t k) {
    __shared__ double a[32][33], t[32][33];
    const uint32_t tid = threadIdx.x, row = tid & 31, half = tid >> 5;
    float* Ab = A + (size_t) (j * kSpdB) * kp + j * kSpdB;
    float* Tb = T + (size_t) (j * kSpdB) * kp + j * kSpdB;
    for (uint32_t e = tid; e < 1024; e += 64) a[e >> 5][e & 31] = (double) Ab[(size_t) (e >> 5) * kp + (e & 31)];
    __syncthreads();
    for (uint32_t c = 0; c < 32; ++c) {
        double p = a[c][c];
        const bool bad = !(p > 0.0) || !(p <= 1.7976931348623157e308);
        if (bad) {
            if (tid == 0) atomicAdd(fail, 1u);
            p = 1.0;
        }
        const double d = sqrt(p);
        __syncthreads();  // (every thread has read the pivot)
        if (half == 0) {
            if (row == c) a[c][c] = d;
            else if (row > c) a[row][c] /= d;
        }
        __syncthreads();
        if (row > c) {
            const double lrc = a[row][c];
            for (uint32_t c2 = c + 1 + half; c2 <= row; c2 += 2) a[row][c2] -= lrc * a[c2][c];
        }
        __syncthreads();
    }
    if (tid < 32) {  // column tid of T: t[r] = (delta - sum_{u < r} L[r][u] t[u]) / L[r][r], zero above the diagonal
        double tc[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            double s = r == (int) tid ? 1.0 : 0.0;
#pragma unroll
            for (int u = 0; u < r; ++u) s -= a[r][u] * tc[u];
            tc[r] = r < (int) tid ? 0.0 : s / a[r][r];
        }
#pragma unroll
        for (int r = 0; r < 32; ++r) t[r][tid] = tc[r];
    }
    __syncthreads();
    for (uint32_t e = tid; e < 1024; e += 64) {
        const uint32_t r = e >> 5, c = e & 31;
        Ab[(size_t) r * kp + c] = c <= r ? (float) a[r][c] : 0.f;
        Tb[(size_t) r * kp + c] = c <= r ? (float) t[r][c] : 0.f;
    }
    if (Minv) {
        for (uint32_t e = tid; e < 1024; e += 64) {
            const uint32_t r = e >> 5, c = e & 31;
            if (r > c || c >= k) continue;
            double s = 0.0;
            for (uint32_t u = c; u < 32; ++u) s += t[u][r] * t[u][c];
            Minv[(size_t) r * k + c] = (float) s;
            Minv[(size_t) c * k + r] = (float) s;
        }
    }
}

// L_ij = A_ij T_jj^T in place, i = j + 1 + blockIdx.x
__global__ __launch_bounds__(64) void k_spd_panel(float* __restrict__ A, const float* __restrict__ T, uint32_t kp, uint32_t j) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5, i = j + 1 + blockIdx.x;
    float* Aij = A + (size_t) (i * kSpdB) * kp + j * kSpdB;
    const float* Tjj = T + (size_t) (j * kSpdB) * kp + j * kSpdB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    tile_mac<false, false>(acc, Aij, Tjj, kp, 1.f, c31, h);  // (every load of A_ij is issued before the first store below)
    tile_store(acc, Aij, kp, c31, h);
}

// A_ip -= L_ij L_pj^T over the blocks j < p <= i of the lower triangle
__global__ __launch_bounds__(64) void k_spd_trail(float* __restrict__ A, uint32_t kp, uint32_t j) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    uint32_t i, p;
    lower_of(blockIdx.x, i, p);
    i += j + 1; p += j + 1;
    float* Aip = A + (size_t) (i * kSpdB) * kp + p * kSpdB;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = Aip[(size_t) acc_row(r, h) * kp + c31];
    tile_mac<false, false>(acc, A + (size_t) (i * kSpdB) * kp + j * kSpdB, A + (size_t) (p * kSpdB) * kp + j * kSpdB, kp, -1.f, c31, h);
    tile_store(acc, Aip, kp, c31, h);
}

// M_it = T_ii L_it over the blocks t < i of the strictly lower triangle (blockIdx.x: the pairs (i - 1, t) of lower_of)
__global__ __launch_bounds__(64) void k_spd_scale(const float* __restrict__ A, const float* __restrict__ T, uint32_t kp, float* __restrict__ M) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    uint32_t i, t;
    lower_of(blockIdx.x, i, t);
    i += 1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // M[r][c] = sum_v T_ii[r][v] L_it[v][c]
    tile_mac<false, true>(acc, T + (size_t) (i * kSpdB) * kp + i * kSpdB, A + (size_t) (i * kSpdB) * kp + t * kSpdB, kp, 1.f, c31, h);
    tile_store(acc, M + (size_t) (i * kSpdB) * kp + t * kSpdB, kp, c31, h);
}

// T_ij = -sum_{t = j .. i - 1} M_it T_tj for i = j + s, j = blockIdx.x: the blocks T_tj are at distances below s, done before
__global__ __launch_bounds__(64) void k_spd_tinv(const float* __restrict__ M, float* __restrict__ T, uint32_t kp, uint32_t s) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5, j = blockIdx.x, i = j + s;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (uint32_t t = j; t < i; ++t)  // T_ij[r][c] -= sum_u M_it[r][u] T_tj[u][c]
        tile_mac<false, true>(acc, M + (size_t) (i * kSpdB) * kp + t * kSpdB, T + (size_t) (t * kSpdB) * kp + j * kSpdB, kp, -1.f, c31, h);
    tile_store(acc, T + (size_t) (i * kSpdB) * kp + j * kSpdB, kp, c31, h);
}

// Minv block (a, b), a <= b (blockIdx.x: the pair (b, a) of lower_of): sum_{t >= b} T_ta^T T_tb, the part inside [k][k] and
// its mirror.  On a diagonal block entry (r, c) and entry (c, r) are the same products in the same order: one of them writes.
__global__ __launch_bounds__(64) void k_spd_prod(const float* __restrict__ T, uint32_t kp, uint32_t nb, uint32_t k, float* __restrict__ Minv) {
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    uint32_t a, b;
    lower_of(blockIdx.x, b, a);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (uint32_t t = b; t < nb; ++t)  // out[r][c] += sum_u T_ta[u][r] T_tb[u][c]
        tile_mac<true, true>(acc, T + (size_t) (t * kSpdB) * kp + a * kSpdB, T + (size_t) (t * kSpdB) * kp + b * kSpdB, kp, 1.f, c31, h);
    const uint32_t col = b * kSpdB + c31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t row = a * kSpdB + acc_row(r, h);
        if (row >= k || col >= k || row > col) continue;
        Minv[(size_t) row * k + col] = acc[r];
        Minv[(size_t) col * k + row] = acc[r];
    }
}

uint32_t spd_kp(uint32_t k) { return (k + kSpdB - 1) / kSpdB * kSpdB; }

}  // namespace
}  // namespace mfx
