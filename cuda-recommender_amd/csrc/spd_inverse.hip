// spd_inverse.hip -- Minv ~ G^-1 of one symmetric positive definite matrix G [k][k] on the device, 1 <= k <= 1024, gfx950
// (mfx_spd_inverse; the preconditioner of mfx_ials_cg_create).  Blocked with blocks of kSpdB = 32 coordinates on
// a padded copy A [kp][kp], kp = k rounded up to 32, whose tail is the identity (nothing outside [k][k] of G or Minv is ever
// touched, and the tail contributes exact zeros):
//   G = L L^T      for j = 0 .. nb - 1:  k_spd_diag   L_jj and T_jj = L_jj^-1 of the diagonal block, one workgroup, fp64 in LDS
//                                        k_spd_panel  L_ij = A_ij T_jj^T for i > j, one wavefront per block
//                                        k_spd_trail  A_ip -= L_ij L_pj^T for j < p <= i, one wavefront per block
//   T = L^-1       k_spd_scale   M_it = T_ii L_it for t < i (every block at once); then for s = 1 .. nb - 1
//                  k_spd_tinv    T_ij = -sum_{t = j .. i - 1} M_it T_tj for i = j + s, one wavefront per block, t ascending
//   Minv = T^T T   k_spd_prod    block (a, b), a <= b: sum_{t = b .. nb - 1} T_ta^T T_tb, t ascending, written with its mirror
// kp = 32 (k <= 32) is the diagonal kernel alone, which then forms T^T T in fp64 too.  Every block product is a chain of
// v_mfma_f32_32x32x2_f32 over the summed index in ascending order, so every sum's order is fixed by k: the bits of Minv depend
// on (G, k) alone.  The stages depend on each other by stream order only: no kernel waits for another workgroup, no float
// atomics.  A pivot that is <= 0 or not finite counts into *fail (an integer atomic) and is replaced by 1: every later stage
// runs to its end, Minv is then unspecified.  4 nb launches for nb = kp / 32 > 1 blocks: 128 at k = 1024.
#include "als_solver.hpp"

namespace mfx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr uint32_t kSpdB = 32;

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

size_t spd_inverse_ws_floats(uint32_t k) { return (size_t) 3 * spd_kp(k) * spd_kp(k); }

int spd_inverse_launch(const float* G, uint32_t k, float* Minv, float* ws, uint32_t* fail, hipStream_t st) {
    MFX_REQUIRE(k >= 1 && k <= kIalsBlockMaxRank, "SPD inverse: k = %u not supported (1 <= k <= %u)", k, kIalsBlockMaxRank);
    const uint32_t kp = spd_kp(k), nb = kp / kSpdB;
    float *A = ws, *T = ws + (size_t) kp * kp, *M = ws + (size_t) 2 * kp * kp;
    hipLaunchKernelGGL(k_spd_copy, dim3((kp * kp + 255) / 256), dim3(256), 0, st, G, k, kp, A);
    MFX_HIP(hipGetLastError());
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

int spd_inverse_op(int64_t k, const float* A, float* Ainv, int device) {
    MFX_REQUIRE(k >= 1 && k <= (int64_t) kIalsBlockMaxRank, "mfx_spd_inverse: k = %lld not supported (1 <= k <= %u)", (long long) k, kIalsBlockMaxRank);
    MFX_TRY(use_device(device));
    OpStream os;
    MFX_HIP(hipStreamCreateWithFlags(&os.st, hipStreamNonBlocking));
    const size_t kk = (size_t) k * k;
    DevBuf<float> G, Minv, ws;
    DevBuf<uint32_t> fail;
    MFX_TRY(G.alloc(kk));
    MFX_TRY(G.upload(A, kk, MFX_HOST, os.st));
    MFX_TRY(Minv.alloc_zero(kk, os.st));
    MFX_TRY(ws.alloc(spd_inverse_ws_floats((uint32_t) k)));
    MFX_TRY(fail.alloc_zero(1, os.st));
    MFX_TRY(spd_inverse_launch(G.get(), (uint32_t) k, Minv.get(), ws.get(), fail.get(), os.st));
    uint32_t bad = 0;
    MFX_HIP(hipMemcpyAsync(&bad, fail.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipMemcpyAsync(Ainv, Minv.get(), sizeof(float) * kk, hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipStreamSynchronize(os.st));
    MFX_REQUIRE(bad == 0, "mfx_spd_inverse: A is not positive definite (%u pivots <= 0 or not finite): it must be symmetric, positive definite and finite",
                bad);
    return MFX_OK;
}

}  // namespace mfx
