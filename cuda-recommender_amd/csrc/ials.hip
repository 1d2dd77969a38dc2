// ials.hip -- implicit-feedback ALS (Hu, Koren, Volinsky 2008) on gfx950: the dense base Gramian, the check of the
// interaction strengths and the objective.  The per-segment systems are the k_ials_* kernels of als_solver.hip.
//
// Base Gramian G = X^T X + lambda I over ALL rows of X [rows][k] (formed once per half-sweep): a tall-skinny
// reduction on the matrix cores.  Partition p (one wavefront) takes rows [p per, (p + 1) per) and accumulates the
// upper block triangle with v_mfma_f32_32x32x2_f32 exactly as k_als_gram<NT> does (lane l supplies X[row q0 + (l >> 5)]
// [32 I + (l & 31)] as the A operand of tile (I, J) and the B operand of tile (J', I)), from contiguous rows instead of
// gathered ones; the partials are then summed in partition order -- no float atomics, bitwise reproducible.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "als_solver.hpp"

namespace mfx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr uint32_t kBaseParts = 1024;  // partitions (wavefronts) of the base Gramian at most
constexpr uint32_t kBaseMinRows = 64;  // rows per partition at least
constexpr uint32_t kGramF64Parts = 64; // row partitions of the fp64 Gramians of the objective
constexpr uint32_t kLossBlocks = 1024; // workgroups of the per-entry objective terms
constexpr int kLossBlock = 256;

constexpr int tiles_of(int NT) { return NT * (NT + 1) / 2; }

template <int NT>
__global__ __launch_bounds__(64) void k_ials_base_gram(const float* __restrict__ X, uint32_t rows, uint32_t k, uint32_t per,
                                                       float* __restrict__ part) {
    constexpr int T = tiles_of(NT);
    constexpr int U = NT >= 3 ? 4 : 8;  // row pairs per step: all loads of a step go out before its MFMAs
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    const uint32_t lo = blockIdx.x * per, hi = min(rows, lo + per);
    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    for (uint32_t q0 = lo; q0 < hi; q0 += 2 * U) {
        float av[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = q0 + 2 * u + h;
#pragma unroll
            for (int I = 0; I < NT; ++I) {
                const uint32_t col = 32 * I + c31;
                av[u][I] = row < hi && col < k ? X[(size_t) row * k + col] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int ti = 0;
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int J = I; J < NT; ++J, ++ti)
                    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][I], av[u][J], acc[ti], 0, 0, 0);
        }
    }
    float* w = part + (size_t) blockIdx.x * T * 1024;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) w[t * 1024 + r * 64 + lane] = acc[t][r];
}

// 64 accumulator slots per workgroup: wave w sums partitions w, w + 4, ... in order, wave 0 adds the four sums in order;
// slot (tile (I, J), register r, lane l) is entry (32 I + (r & 3) + 8 (r >> 2) + 4 (l >> 5), 32 J + (l & 31)).
template <int NT>
__global__ __launch_bounds__(256) void k_ials_base_reduce(const float* __restrict__ part, uint32_t nparts, uint32_t k, float lambda,
                                                          float* __restrict__ G) {
    constexpr int T = tiles_of(NT);
    __shared__ float sums[4][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t slot = blockIdx.x * 64 + lane;  // < T * 1024
    float s = 0.f;
    for (uint32_t p = wv; p < nparts; p += 4) s += part[(size_t) p * T * 1024 + slot];
    sums[wv][lane] = s;
    __syncthreads();
    if (wv != 0) return;
    s = ((sums[0][lane] + sums[1][lane]) + sums[2][lane]) + sums[3][lane];
    uint32_t t = slot >> 10, I = 0, J = 0;
    for (uint32_t ti = 0, i = 0; i < (uint32_t) NT; ++i)
        for (uint32_t j = i; j < (uint32_t) NT; ++j, ++ti)
            if (ti == t) { I = i; J = j; }
    const uint32_t r = (slot >> 6) & 15;
    const uint32_t row = 32 * I + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = 32 * J + (lane & 31);
    if (row < k && col < k && row <= col) {  // (a diagonal tile holds (row, col) and (col, row) alike: same sums)
        G[(size_t) row * k + col] = row == col ? s + lambda : s;
        G[(size_t) col * k + row] = row == col ? s + lambda : s;
    }
}

template <int NT>
int base_gram_nt(const float* X, uint32_t rows, uint32_t k, float lambda, float* part, float* G, hipStream_t st) {
    const uint32_t nparts = ials_base_parts(rows);
    const uint32_t per = (rows + nparts - 1) / nparts;
    hipLaunchKernelGGL(k_ials_base_gram<NT>, dim3(nparts), dim3(64), 0, st, X, rows, k, per, part);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ials_base_reduce<NT>, dim3(tiles_of(NT) * 1024 / 64), dim3(256), 0, st, part, nparts, k, lambda, G);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

// ---- objective -----------------------------------------------------------------------------------------------------
// L = sum_{(u,i) in Omega} [c_ui (p_ui - s_ui)^2 - s_ui^2] + <W^T W, H^T H>_F + lambda (|W|^2 + |H|^2), the dense
// sum over all m n pairs rewritten.  s_ui is the fp32 FMA chain in ascending t (the score of mfx_rec_query); the
// entry terms and both Gramians are formed in fp64 (an fp32 product is exact in fp64), every sum in a fixed order.

// fp64 X^T X in 4 x 4 blocks: thread (bi, bj) of the (k/4)^2 grid, row partition blockIdx.y
__global__ __launch_bounds__(256) void k_gram_f64(const float* __restrict__ X, uint32_t rows, uint32_t k, uint32_t nb, uint32_t per,
                                                  double* __restrict__ part) {
    const uint32_t pi = blockIdx.x * 256 + threadIdx.x;
    if (pi >= nb * nb) return;
    const uint32_t bi = pi / nb, bj = pi % nb;
    const uint32_t lo = blockIdx.y * per, hi = min(rows, lo + per);
    double acc[4][4] = {};
    for (uint32_t r = lo; r < hi; ++r) {
        const float* x = X + (size_t) r * k;
        double xi[4], xj[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            xi[e] = 4 * bi + e < k ? (double) x[4 * bi + e] : 0.0;
            xj[e] = 4 * bj + e < k ? (double) x[4 * bj + e] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_fma(xi[a], xj[b], acc[a][b]);
    }
    double* w = part + ((size_t) blockIdx.y * nb * nb + pi) * 16;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) w[4 * a + b] = acc[a][b];
}

__device__ __forceinline__ double block_sum(double v, double* sh) {  // fixed-order tree over kLossBlock threads
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = kLossBlock / 2; o > 0; o >>= 1) {
        if ((int) threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(kLossBlock) void k_ials_loss_entries(uint32_t nseg, uint64_t nnz, const uint32_t* __restrict__ ptr,
                                                                  const uint32_t* __restrict__ idx, const float* __restrict__ val,
                                                                  const float* __restrict__ W, const float* __restrict__ H, uint32_t k,
                                                                  float alpha, double* __restrict__ partials) {
    __shared__ double sh[kLossBlock];
    double acc = 0.0;
    for (uint64_t q = (uint64_t) blockIdx.x * kLossBlock + threadIdx.x; q < nnz; q += (uint64_t) gridDim.x * kLossBlock) {
        const float r = val[q];
        if (!(r > 0.f)) continue;  // an explicit zero: c = 1, p = 0, the term is 0
        uint32_t a = 0, b = nseg;  // the row: last u with ptr[u] <= q
        while (b - a > 1) {
            const uint32_t m = (a + b) / 2;
            if (ptr[m] <= q) a = m; else b = m;
        }
        const float* wu = W + (size_t) a * k;
        const float* hi = H + (size_t) idx[q] * k;
        float s = 0.f;
        for (uint32_t t = 0; t < k; ++t) s = __builtin_fmaf(wu[t], hi[t], s);
        const float w = alpha * r;
        const double c = 1.0 + (double) w, d = 1.0 - (double) s;
        acc += c * d * d - (double) s * (double) s;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(kLossBlock) void k_ials_loss_final(const double* __restrict__ gw, const double* __restrict__ gh, uint32_t nparts,
                                                                uint32_t nb, uint32_t k, double lambda, const double* __restrict__ entry_partials,
                                                                uint32_t nentry, double* __restrict__ out) {
    __shared__ double sh[kLossBlock];
    double acc = 0.0;
    for (uint32_t pi = threadIdx.x; pi < nb * nb; pi += kLossBlock) {
        const uint32_t bi = pi / nb, bj = pi % nb;
        for (int e = 0; e < 16; ++e) {
            const uint32_t i = 4 * bi + e / 4, j = 4 * bj + e % 4;
            if (i >= k || j >= k) continue;
            double sw = 0.0, sv = 0.0;
            for (uint32_t p = 0; p < nparts; ++p) {
                sw += gw[((size_t) p * nb * nb + pi) * 16 + e];
                sv += gh[((size_t) p * nb * nb + pi) * 16 + e];
            }
            acc += sw * sv;
            if (i == j) acc += lambda * (sw + sv);
        }
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        double s = t;
        for (uint32_t b = 0; b < nentry; ++b) s += entry_partials[b];
        *out = s;
    }
}

__global__ __launch_bounds__(256) void k_ials_check(uint64_t n, const float* __restrict__ val, float alpha,
                                                    unsigned long long* __restrict__ first_bad) {
    unsigned long long bad = ~0ull;
    for (uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t) gridDim.x * 256) {
        const float v = val[q];
        const float w = alpha * v;
        if (!(v >= 0.f && v <= FLT_MAX && w <= FLT_MAX) && q < bad) bad = q;  // (NaN fails every compare)
    }
    if (bad != ~0ull) atomicMin(first_bad, bad);
}

// ---- unobserved weight alpha0 and a regulariser per segment (mfx_ials_create_reg) -----------------------
// G0 = fp32(alpha0 S) from S = X^T X as the kernels above sum it (launched with lambda = 0): one rounding on top of S
__global__ __launch_bounds__(256) void k_ialsr_scale(float* __restrict__ G, uint32_t n, float alpha0) {
#pragma clang fp contract(off)
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) G[e] = alpha0 * G[e];
}

// rho[s] = fp32(lambda (n_s + alpha0 N)^nu), n_s = the stored entries of segment s with r > 0; all of it in fp64, unfused.
// One wavefront per segment; the count is an integer sum (no order).
__global__ __launch_bounds__(256) void k_ialsr_rho(const uint32_t* __restrict__ ptr, const float* __restrict__ val, uint32_t nseg, double lambda,
                                                   double alpha0, double N, double nu, float* __restrict__ rho) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63, seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    uint32_t cnt = 0;
    for (uint32_t q = ptr[seg] + lane; q < ptr[seg + 1]; q += 64) cnt += val[q] > 0.f ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) {
        const double base = (double) cnt + alpha0 * N;
        rho[seg] = (float) (lambda * pow(base, nu));
    }
}

// The entry terms (alpha0 + w)(1 - s)^2 - alpha0 s^2, written as [(alpha0 + w)(1 - s)^2 - s^2] + (1 - alpha0) s^2 with the
// bracket in the operations k_ials_loss_entries compiles to (one multiply, one fused multiply-subtract): at alpha0 = 1 the
// second term adds an exact zero and the sum is that kernel's, bit for bit.
__global__ __launch_bounds__(kLossBlock) void k_ialsr_loss_entries(uint32_t nseg, uint64_t nnz, const uint32_t* __restrict__ ptr,
                                                                   const uint32_t* __restrict__ idx, const float* __restrict__ val,
                                                                   const float* __restrict__ W, const float* __restrict__ H, uint32_t k,
                                                                   float alpha, double alpha0, double* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ double sh[kLossBlock];
    double acc = 0.0;
    for (uint64_t q = (uint64_t) blockIdx.x * kLossBlock + threadIdx.x; q < nnz; q += (uint64_t) gridDim.x * kLossBlock) {
        const float r = val[q];
        if (!(r > 0.f)) continue;  // an explicit zero is no entry
        uint32_t a = 0, b = nseg;  // the row: last u with ptr[u] <= q
        while (b - a > 1) {
            const uint32_t m = (a + b) / 2;
            if (ptr[m] <= q) a = m; else b = m;
        }
        const float* wu = W + (size_t) a * k;
        const float* hi = H + (size_t) idx[q] * k;
        float s = 0.f;
        for (uint32_t t = 0; t < k; ++t) s = __builtin_fmaf(wu[t], hi[t], s);
        const float w = alpha * r;
        const double c = (double) w + alpha0, d = 1.0 - (double) s, ss = (double) s * (double) s;
        double e = __builtin_fma(d, c * d, -ss);
        e = __builtin_fma(1.0 - alpha0, ss, e);
        acc += e;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// sum_s rho[s] |y_s|^2 in fp64: thread t takes the segments t, t + (grid threads), ...; one partial per workgroup
__global__ __launch_bounds__(kLossBlock) void k_ialsr_loss_reg(const float* __restrict__ Y, uint32_t nseg, uint32_t k, const float* __restrict__ rho,
                                                               double* __restrict__ partials) {
    __shared__ double sh[kLossBlock];
    double acc = 0.0;
    for (uint64_t s = (uint64_t) blockIdx.x * kLossBlock + threadIdx.x; s < nseg; s += (uint64_t) gridDim.x * kLossBlock) {
        const float* y = Y + (size_t) s * k;
        double n2 = 0.0;
        for (uint32_t t = 0; t < k; ++t) n2 = __builtin_fma((double) y[t], (double) y[t], n2);
        acc = __builtin_fma((double) rho[s], n2, acc);
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// alpha0 <W^T W, H^T H>_F + lambda (tr W^T W + tr H^T H) + the partials.  nu = 0 (rho = lambda for every segment): lambda is
// passed and the partials are the entry terms alone, the operations of k_ials_loss_final; nu > 0: lambda = 0 and the partials
// hold the entry terms and the two sums of k_ialsr_loss_reg.
__global__ __launch_bounds__(kLossBlock) void k_ialsr_loss_final(const double* __restrict__ gw, const double* __restrict__ gh, uint32_t nparts,
                                                                 uint32_t nb, uint32_t k, double lambda, double alpha0,
                                                                 const double* __restrict__ partials, uint32_t npartials, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sh[kLossBlock];
    double acc = 0.0;
    for (uint32_t pi = threadIdx.x; pi < nb * nb; pi += kLossBlock) {
        const uint32_t bi = pi / nb, bj = pi % nb;
        for (int e = 0; e < 16; ++e) {
            const uint32_t i = 4 * bi + e / 4, j = 4 * bj + e % 4;
            if (i >= k || j >= k) continue;
            double sw = 0.0, sv = 0.0;
            for (uint32_t p = 0; p < nparts; ++p) {
                sw += gw[((size_t) p * nb * nb + pi) * 16 + e];
                sv += gh[((size_t) p * nb * nb + pi) * 16 + e];
            }
            acc = __builtin_fma(alpha0 * sw, sv, acc);
            if (i == j) acc = __builtin_fma(lambda, sw + sv, acc);
        }
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) {
        double s = t;
        for (uint32_t b = 0; b < npartials; ++b) s += partials[b];
        *out = s;
    }
}

}  // namespace

uint32_t ials_base_parts(uint32_t rows) {
    return std::max<uint32_t>(1, std::min<uint32_t>(kBaseParts, (rows + kBaseMinRows - 1) / kBaseMinRows));
}
size_t ials_base_ws_floats(uint32_t rows, uint32_t k) {
    const size_t nt = (k + 31) / 32;
    return (size_t) ials_base_parts(rows) * (nt * (nt + 1) / 2) * 1024;
}

int ials_base_gramian(const float* X, uint32_t rows, uint32_t k, float lambda, float* part, float* G, hipStream_t st) {
    switch ((k + 31) / 32) {
        case 1: return base_gram_nt<1>(X, rows, k, lambda, part, G, st);
        case 2: return base_gram_nt<2>(X, rows, k, lambda, part, G, st);
        case 3: return base_gram_nt<3>(X, rows, k, lambda, part, G, st);
        case 4: return base_gram_nt<4>(X, rows, k, lambda, part, G, st);
        default: return fail(MFX_ERR_INVALID, "implicit ALS: rank k = %u not supported (1 <= k <= 128)", k);
    }
}

int ials_check_values(const float* d_val, uint64_t n, float alpha, const char* what, hipStream_t st) {
    if (n == 0) return MFX_OK;
    DevBuf<unsigned long long> flag;
    MFX_TRY(flag.alloc(1));
    MFX_HIP(hipMemsetAsync(flag.get(), 0xFF, sizeof(unsigned long long), st));
    const uint32_t grid = (uint32_t) std::min<uint64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_ials_check, dim3(grid), dim3(256), 0, st, n, d_val, alpha, flag.get());
    MFX_HIP(hipGetLastError());
    unsigned long long bad = ~0ull;
    MFX_HIP(hipMemcpyAsync(&bad, flag.get(), sizeof(bad), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (bad == ~0ull) return MFX_OK;
    float v = 0.f;
    MFX_HIP(hipMemcpy(&v, d_val + bad, sizeof(v), hipMemcpyDeviceToHost));
    return fail(MFX_ERR_INVALID, "%s %g at position %llu: implicit ALS needs finite strengths r >= 0 with alpha * r finite",
                what, (double) v, bad);
}

size_t ials_loss_ws_doubles(uint32_t k) {
    const size_t nb = (k + 3) / 4;
    return 2 * (size_t) kGramF64Parts * nb * nb * 16 + kLossBlocks;
}

int ials_loss_launch(const AlsHalf& rows, const float* W, uint32_t m, const float* H, uint32_t n, uint32_t k, float lambda, float alpha,
                     double* ws, double* out, hipStream_t st) {
    const uint32_t nb = (k + 3) / 4;
    const size_t gsz = (size_t) kGramF64Parts * nb * nb * 16;
    double* gw = ws;
    double* gh = ws + gsz;
    double* ep = ws + 2 * gsz;
    const dim3 gg((nb * nb + 255) / 256, kGramF64Parts);
    hipLaunchKernelGGL(k_gram_f64, gg, dim3(256), 0, st, W, m, k, nb, (m + kGramF64Parts - 1) / kGramF64Parts, gw);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gram_f64, gg, dim3(256), 0, st, H, n, k, nb, (n + kGramF64Parts - 1) / kGramF64Parts, gh);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ials_loss_entries, dim3(kLossBlocks), dim3(kLossBlock), 0, st, rows.nseg, rows.nnz, rows.ptr.get(), rows.idx.get(),
                       rows.val.get(), W, H, k, alpha, ep);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ials_loss_final, dim3(1), dim3(kLossBlock), 0, st, gw, gh, kGramF64Parts, nb, k, (double) lambda, ep, kLossBlocks, out);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int ialsr_scale_launch(float* G, size_t n, float alpha0, hipStream_t st) {
    hipLaunchKernelGGL(k_ialsr_scale, dim3((uint32_t) ((n + 255) / 256)), dim3(256), 0, st, G, (uint32_t) n, alpha0);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int ialsr_base_gramian(const float* X, uint32_t rows, uint32_t k, float alpha0, float* part, float* G0, hipStream_t st) {
    MFX_TRY(ials_base_gramian(X, rows, k, 0.f, part, G0, st));  // (S + 0 = S, bit for bit)
    return ialsr_scale_launch(G0, (size_t) k * k, alpha0, st);
}

int ialsr_check_params(const char* fn, float lambda, float alpha0, float nu, int64_t rows, int64_t cols) {
    MFX_REQUIRE(std::isfinite(alpha0) && alpha0 > 0.f, "%s: alpha0 = %g (finite and > 0 required)", fn, (double) alpha0);
    MFX_REQUIRE(nu >= 0.f && nu <= 1.f, "%s: nu = %g (0 <= nu <= 1 required)", fn, (double) nu);
    const double most = (1.0 + (double) alpha0) * (double) std::max(rows, cols);
    const float top = (float) ((double) lambda * std::pow(most, (double) nu));
    MFX_REQUIRE(std::isfinite(top), "%s: the regulariser lambda ((1 + alpha0) max(rows, cols))^nu = %g is not a finite fp32 number "
                "(lambda = %g, alpha0 = %g, nu = %g)", fn, (double) top, (double) lambda, (double) alpha0, (double) nu);
    return MFX_OK;
}

int ialsr_rho_launch(const AlsHalf& h, uint32_t N, float lambda, float alpha0, float nu, float* rho, hipStream_t st) {
    if (h.nseg == 0) return MFX_OK;
    hipLaunchKernelGGL(k_ialsr_rho, dim3((h.nseg + 3) / 4), dim3(256), 0, st, h.ptr.get(), h.val.get(), h.nseg, (double) lambda,
                       (double) alpha0, (double) N, (double) nu, rho);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

size_t ialsr_loss_ws_doubles(uint32_t k) { return ials_loss_ws_doubles(k) + 2 * (size_t) kLossBlocks; }

int ialsr_loss_launch(const AlsHalf& rows, const float* W, uint32_t m, const float* H, uint32_t n, uint32_t k, float lambda, float alpha,
                      float alpha0, float nu, const float* rho_rows, const float* rho_cols, double* ws, double* out, hipStream_t st) {
    const uint32_t nb = (k + 3) / 4;
    const size_t gsz = (size_t) kGramF64Parts * nb * nb * 16;
    double* gw = ws;
    double* gh = ws + gsz;
    double* ep = ws + 2 * gsz;  // [kLossBlocks] entry terms, then (nu > 0) [kLossBlocks] each for the regularisers of W and H
    const dim3 gg((nb * nb + 255) / 256, kGramF64Parts);
    hipLaunchKernelGGL(k_gram_f64, gg, dim3(256), 0, st, W, m, k, nb, (m + kGramF64Parts - 1) / kGramF64Parts, gw);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gram_f64, gg, dim3(256), 0, st, H, n, k, nb, (n + kGramF64Parts - 1) / kGramF64Parts, gh);
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ialsr_loss_entries, dim3(kLossBlocks), dim3(kLossBlock), 0, st, rows.nseg, rows.nnz, rows.ptr.get(), rows.idx.get(),
                       rows.val.get(), W, H, k, alpha, (double) alpha0, ep);
    MFX_HIP(hipGetLastError());
    const bool uniform = nu == 0.f;  // rho = lambda everywhere: the regulariser from the traces of the Gramians already formed
    if (!uniform) {
        hipLaunchKernelGGL(k_ialsr_loss_reg, dim3(kLossBlocks), dim3(kLossBlock), 0, st, W, m, k, rho_rows, ep + kLossBlocks);
        MFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ialsr_loss_reg, dim3(kLossBlocks), dim3(kLossBlock), 0, st, H, n, k, rho_cols, ep + 2 * kLossBlocks);
        MFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ialsr_loss_final, dim3(1), dim3(kLossBlock), 0, st, gw, gh, kGramF64Parts, nb, k, uniform ? (double) lambda : 0.0,
                       (double) alpha0, ep, uniform ? kLossBlocks : 3 * kLossBlocks, out);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

}  // namespace mfx
