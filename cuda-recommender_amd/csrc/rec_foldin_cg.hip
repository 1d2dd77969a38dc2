// rec_foldin_cg.hip -- fold-in by preconditioned conjugate gradients (mfx_rec_fold_in_cg_setup) on gfx950, ranks up to 1024.
// H is fixed, so every query row's system is the fixed base G = H^T H + lambda I plus a matrix of the rank of the row:
//     implicit:  A p = G p + sum_e w_e <h_e, p> h_e,   b = sum_e fp32(1 + w_e) h_e,   w_e = fp32(alpha r_e),  M^-1 = Minv ~ G^-1
//     explicit:  A p = rho p + sum_e <h_e, p> h_e,     b = sum_e r_e h_e,             rho = lambda or fp32(lambda n),  M^-1 = I
// and CG preconditioned by G^-1 ends, in exact arithmetic, after n + 1 steps on a row of n entries.  The method is
// step-synchronous over the query batch; y (the caller's rows), r, z, p, q are [rows][k] fp32, |b|^2, gamma, the step count
// and the frozen flag live per row.
// This unit also holds what the method shares with the target solves of rec_explain_cg.hip (rec_foldin_cg.hpp):
// there a system is a (row, target) pair, T per row; here T = 1.  The kernels, in the order of a step:
//   k_cg_gather<C, 1, MODE>   (rec_foldin_cg.hpp) one wavefront per work item of AlsHalf (a whole row, or a chunk of 2048
//                             entries into a partial slot): lane l holds coordinates l + 64 i of p and of the sum; an entry's
//                             row of H is loaded once, t = <h_e, p> by a butterfly over the lanes, then (c_e t) h_e from the
//                             registers that still hold the row.  Four rows of H are in flight before their reductions.  The
//                             first pass forms b the same way (and the sum over <h_e, y0> when warm).
//   k_cg_reduce               (shared) the partial slots of a split row summed in slot order, per target
//   k_foldcg_dense<ND>        (implicit; shared) out = V M (+ add) for a symmetric M [k][k]: 32 rows x 128 columns per wavefront
//                             on v_mfma_f32_32x32x2_f32; an output row depends on its own input row and the k order alone
//   k_foldcg_start            r = b - A y0, |b|^2, the rows without a right-hand side zeroed and frozen, the stop test on y0
//   k_cg_step                 (shared) <p, q>, a, y += a p, r -= a q, the count, the stop test |r| <= tol |b|
//   k_cg_dir                  (shared) gamma' = <r, z>, p = z + (gamma' / gamma) p; the systems still active counted for the host
// cg_iterate is the step loop of both.  A frozen system is skipped by every kernel: its bits never change again.  No float
// atomics; every sum has a fixed order that depends on the system alone, so its bits and count do not depend on the batch.
#include <algorithm>
#include <cmath>

#include "rec_foldin_cg.hpp"

namespace mfx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// (kGatherRows, wave_sum, row_rho: rec_foldin_cg.hpp)

// the partial slots of a split row into S / B [seg T + t][k], in slot order; one wavefront per (split row, target)
__global__ __launch_bounds__(64) void k_cg_reduce(const AlsReduce* __restrict__ reduces, uint32_t nreduces, uint32_t k, uint32_t T, int32_t mode,
                                                  const uint32_t* __restrict__ frozen, const float* __restrict__ ws, float* __restrict__ S,
                                                  float* __restrict__ B) {
    if (blockIdx.x >= nreduces) return;
    const AlsReduce rd = reduces[blockIdx.x];
    const uint32_t t = blockIdx.y, stride = cg_ws_stride(T, mode);
    const size_t sys = (size_t) rd.seg * T + t;
    if (frozen && frozen[sys]) return;
    for (uint32_t c = threadIdx.x & 63; c < k; c += 64) {
        float s = 0.f, b = 0.f;
        for (uint32_t p = 0; p < rd.nslots; ++p) {
            const size_t row = (size_t) (rd.slot0 + p) * stride;
            if (mode & 1) s += ws[(row + t) * k + c];
            if (mode & 2) b += ws[(row + 1) * k + c];
        }
        if (mode & 1) S[sys * k + c] = s;
        if (mode & 2) B[sys * k + c] = b;
    }
}

// four consecutive floats of a row at column c (c % 4 == 0): one 16-byte load when the rows are 16-byte aligned (k % 4 == 0)
__device__ __forceinline__ f32x4 load4(const float* __restrict__ row, uint32_t c, bool ok, uint32_t k, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!ok || c >= k) return v;
    if (vec) return *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c + e < k) v[e] = row[c + e];
    return v;
}

// out[seg][b0 + j] = sum_t V[seg][t] M[b0 + j][t] (+ add[seg][b0 + j]) for a symmetric M [k][k]: 32 rows x the columns
// [b0, b0 + 32 ND) with b0 = 128 blockIdx.y per wavefront.  MFMA step e of the 8-column group at kk: lane (r31, h) supplies
// V[seg0 + r31][kk + 4 h + e] and M[b0 + 32 t + r31][kk + 4 h + e]: the sum over t in a fixed order, row by row.  A wavefront
// whose 32 rows are all frozen does nothing; a frozen row is not written.  out and add may be the same array.
template <int ND>
__global__ __launch_bounds__(256) void k_foldcg_dense(const float* __restrict__ V, uint32_t nseg, uint32_t k, const float* __restrict__ M,
                                                      const uint32_t* __restrict__ frozen, const float* add, float* out) {
    const uint32_t lane = threadIdx.x & 63, r31 = lane & 31, h = lane >> 5;
    const uint32_t seg0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (seg0 >= nseg) return;
    const bool sok = seg0 + r31 < nseg;
    if (frozen && __ballot(sok && !frozen[seg0 + r31]) == 0) return;  // wave-uniform
    const uint32_t b0 = blockIdx.y * 128, width = min(128u, k - b0);
    const bool vec = (k & 3) == 0;
    const float* vrow = V + (size_t) (sok ? seg0 + r31 : seg0) * k;
    const float* mrow[ND];
    bool mok[ND];
    f32x16 acc[ND];
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        mok[t] = 32 * t + r31 < width;
        mrow[t] = M + (size_t) (b0 + (mok[t] ? 32 * t + r31 : 0)) * k;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    }
    for (uint32_t kk = 0; kk < k; kk += 8) {
        const uint32_t c = kk + 4 * h;
        const f32x4 a = load4(vrow, c, sok, k, vec);
        f32x4 b[ND];
#pragma unroll
        for (int t = 0; t < ND; ++t) b[t] = load4(mrow[t], c, mok[t], k, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < ND; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[t][e], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t seg = seg0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (seg >= nseg || (frozen && frozen[seg])) continue;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const uint32_t col = 32 * t + r31;
            if (col < width) {
                const size_t o = (size_t) seg * k + b0 + col;
                out[o] = add ? acc[t][r] + add[o] : acc[t][r];
            }
        }
    }
}

// After the first gather (R = b; warm: Q = the gathered part of A y0, for the implicit model with G y0 added already), one
// wavefront per row, lane l the columns l + 64 i.  A row with entries and b != 0: r = b - A y0 (cold: r = b, Y is zero); then
// cg_start_tail (a row without entries has b2 = 0 there).
__global__ __launch_bounds__(256) void k_foldcg_start(const uint32_t* __restrict__ ptr, uint32_t nseg, uint32_t k, float* __restrict__ Y,
                                                      float* R, float* Z, float* __restrict__ P,  // (explicit: Z is R)
                                                      const float* __restrict__ Q, int32_t warm, int32_t reg, float lambda, float tol,
                                                      float* __restrict__ bb, uint32_t* __restrict__ frozen, int32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63, seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const size_t o = (size_t) seg * k;
    float b2 = 0.f;
    const bool empty = ptr[seg + 1] == ptr[seg];
    if (!empty) {
        for (uint32_t c = lane; c < k; c += 64) b2 = __builtin_fmaf(R[o + c], R[o + c], b2);
        b2 = wave_sum(b2);
    }
    float r2 = b2;
    if (warm && b2 != 0.f) {
        const float rho = row_rho(reg, lambda, ptr, seg);
        r2 = 0.f;
        for (uint32_t c = lane; c < k; c += 64) {
            const float ay = reg ? __builtin_fmaf(rho, Y[o + c], Q[o + c]) : Q[o + c];
            const float r = R[o + c] - ay;
            R[o + c] = r;
            r2 = __builtin_fmaf(r, r, r2);
        }
        r2 = wave_sum(r2);
    }
    cg_start_tail(seg, o, k, lane, b2, r2, tol, Y, R, Z, P, bb, frozen, counts);
}

// One step's first half, after q = A p (explicit: Q holds the gathered part, rho p is added here): a = gamma / <p, q>,
// y += a p, r -= a q, the step counted, the system frozen once |r| <= tol |b| (tol > 0).  One wavefront per system; rho is
// that of the system's row.  <p, q> < 0 or not finite (the inputs were not finite): the system becomes NaN, is frozen and
// counted into *fail (NULL: no count).  <p, q> exactly 0 is a direction that underflowed on a system long converged (tol = 0
// and more steps than it needs): frozen as it is, the step not counted.
__global__ __launch_bounds__(256) void k_cg_step(const uint32_t* __restrict__ ptr, size_t nsys, uint32_t T, uint32_t k, float* __restrict__ Y,
                                                 float* __restrict__ R, const float* __restrict__ P, const float* __restrict__ Q, int32_t reg,
                                                 float lambda, float tol, const float* __restrict__ gamma, const float* __restrict__ bb,
                                                 uint32_t* __restrict__ frozen, int32_t* __restrict__ counts, uint32_t* __restrict__ fail) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t seg = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nsys || frozen[seg]) return;  // wave-uniform
    const size_t o = seg * k;
    const float rho = reg ? row_rho(reg, lambda, ptr, (uint32_t) (seg / T)) : 0.f;
    float pq = 0.f;
    for (uint32_t c = lane; c < k; c += 64) {
        const float q = reg ? __builtin_fmaf(rho, P[o + c], Q[o + c]) : Q[o + c];
        pq = __builtin_fmaf(P[o + c], q, pq);
    }
    pq = wave_sum(pq);
    if (!(pq >= 0.f) || !(pq <= 3.402823466e38f)) {
        for (uint32_t c = lane; c < k; c += 64) Y[o + c] = __builtin_nanf("");
        if (lane == 0) {
            frozen[seg] = 1;
            counts[seg] += 1;
            if (fail) atomicAdd(fail, 1u);
        }
        return;
    }
    if (pq == 0.f) {
        if (lane == 0) frozen[seg] = 1;
        return;
    }
    const float a = gamma[seg] / pq;
    float r2 = 0.f;
    for (uint32_t c = lane; c < k; c += 64) {
        const float p = P[o + c];
        const float q = reg ? __builtin_fmaf(rho, p, Q[o + c]) : Q[o + c];
        Y[o + c] = __builtin_fmaf(a, p, Y[o + c]);
        const float r = __builtin_fmaf(-a, q, R[o + c]);
        R[o + c] = r;
        r2 = __builtin_fmaf(r, r, r2);
    }
    r2 = wave_sum(r2);
    if (lane == 0) {
        counts[seg] += 1;
        if (tol > 0.f && sqrtf(r2) <= tol * sqrtf(bb[seg])) frozen[seg] = 1;
    }
}

// After z = M^-1 r (explicit: Z is R): gamma' = <r, z>; first: p = z, else p = z + (gamma' / gamma) p; gamma = gamma'.
// gamma' exactly 0 freezes the system (nothing is left to do).  The systems still active are counted into *active (NULL: no
// count; one vector atomic per system, an integer: the sum has no order).
__global__ __launch_bounds__(256) void k_cg_dir(size_t nsys, uint32_t k, const float* __restrict__ R, const float* __restrict__ Z,
                                                float* __restrict__ P, int32_t first, float* __restrict__ gamma, uint32_t* __restrict__ frozen,
                                                uint32_t* __restrict__ active) {
    const uint32_t lane = threadIdx.x & 63;
    const size_t seg = (size_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nsys || frozen[seg]) return;  // wave-uniform
    const size_t o = seg * k;
    float g = 0.f;
    for (uint32_t c = lane; c < k; c += 64) g = __builtin_fmaf(R[o + c], Z[o + c], g);
    g = wave_sum(g);
    if (g == 0.f) {
        if (lane == 0) frozen[seg] = 1;
        return;
    }
    if (first) {
        for (uint32_t c = lane; c < k; c += 64) P[o + c] = Z[o + c];
    } else {
        const float beta = g / gamma[seg];
        for (uint32_t c = lane; c < k; c += 64) P[o + c] = __builtin_fmaf(beta, P[o + c], Z[o + c]);
    }
    if (lane == 0) {
        gamma[seg] = g;
        if (active) atomicAdd(active, 1u);
    }
}

template <int C>
void launch_gather_c(int mode, const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, int32_t implicit, float alpha, const float* V,
                     const uint32_t* frozen, float* S, float* B, float* ws, hipStream_t st) {
    const dim3 grid(h.nitems), block(64);
    switch (mode) {
        case 1:
            hipLaunchKernelGGL((k_cg_gather<C, 1, 1>), grid, block, 0, st, h.items.get(), h.nitems, h.idx.get(), h.val.get(), X, x_rows, k, implicit,
                               alpha, 1u, V, frozen, S, B, ws);
            break;
        case 2:
            hipLaunchKernelGGL((k_cg_gather<C, 1, 2>), grid, block, 0, st, h.items.get(), h.nitems, h.idx.get(), h.val.get(), X, x_rows, k, implicit,
                               alpha, 1u, V, frozen, S, B, ws);
            break;
        default:
            hipLaunchKernelGGL((k_cg_gather<C, 1, 3>), grid, block, 0, st, h.items.get(), h.nitems, h.idx.get(), h.val.get(), X, x_rows, k, implicit,
                               alpha, 1u, V, frozen, S, B, ws);
            break;
    }
}

// the gather pass and, where a row was split, the sum of its slots
int gather(int mode, const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, int32_t implicit, float alpha, const float* V,
           const uint32_t* frozen, float* S, float* B, float* ws, hipStream_t st) {
    const uint32_t c = (k + 63) / 64;
    if (c <= 1) launch_gather_c<1>(mode, h, X, x_rows, k, implicit, alpha, V, frozen, S, B, ws, st);
    else if (c <= 2) launch_gather_c<2>(mode, h, X, x_rows, k, implicit, alpha, V, frozen, S, B, ws, st);
    else if (c <= 4) launch_gather_c<4>(mode, h, X, x_rows, k, implicit, alpha, V, frozen, S, B, ws, st);
    else if (c <= 8) launch_gather_c<8>(mode, h, X, x_rows, k, implicit, alpha, V, frozen, S, B, ws, st);
    else launch_gather_c<16>(mode, h, X, x_rows, k, implicit, alpha, V, frozen, S, B, ws, st);
    MFX_HIP(hipGetLastError());
    return cg_reduce(h, k, 1, mode, frozen, ws, S, B, st);
}

// fp64 dot of two contiguous rows over [0, n): four partial sums in a fixed order
double dot4(const double* a, const double* b, size_t n) {
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    size_t t = 0;
    for (; t + 4 <= n; t += 4) {
        s0 += a[t] * b[t];
        s1 += a[t + 1] * b[t + 1];
        s2 += a[t + 2] * b[t + 2];
        s3 += a[t + 3] * b[t + 3];
    }
    for (; t < n; ++t) s0 += a[t] * b[t];
    return (s0 + s1) + (s2 + s3);
}

}  // namespace

int foldcg_dense(const float* V, uint32_t nseg, uint32_t k, const float* M, const uint32_t* frozen, const float* add, float* out, hipStream_t st) {
    const dim3 grid((nseg + 127) / 128, (k + 127) / 128), block(256);
    switch (k > 128 ? 4 : (k + 31) / 32) {
        case 1: hipLaunchKernelGGL(k_foldcg_dense<1>, grid, block, 0, st, V, nseg, k, M, frozen, add, out); break;
        case 2: hipLaunchKernelGGL(k_foldcg_dense<2>, grid, block, 0, st, V, nseg, k, M, frozen, add, out); break;
        case 3: hipLaunchKernelGGL(k_foldcg_dense<3>, grid, block, 0, st, V, nseg, k, M, frozen, add, out); break;
        default: hipLaunchKernelGGL(k_foldcg_dense<4>, grid, block, 0, st, V, nseg, k, M, frozen, add, out); break;
    }
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int cg_reduce(const AlsHalf& h, uint32_t k, uint32_t T, int mode, const uint32_t* frozen, const float* ws, float* S, float* B, hipStream_t st) {
    if (h.nreduces) {
        hipLaunchKernelGGL(k_cg_reduce, dim3(h.nreduces, T), dim3(64), 0, st, h.reduces.get(), h.nreduces, k, T, mode, frozen, ws, S, B);
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

int cg_iterate(const AlsHalf& h, uint32_t T, uint32_t k, const FoldCg& m, float* Y, FoldCgWs& w, int32_t* counts, uint32_t* fail,
               uint32_t* first_active, const std::function<int()>& gather, hipStream_t st) {
    const bool implicit = m.reg == 0, stop = m.tol > 0.f;
    const size_t nsys = (size_t) h.nseg * T;
    const uint32_t n32 = (uint32_t) nsys;
    float *R = w.R.get(), *P = w.P.get(), *Q = w.Q.get();
    float* Z = implicit ? w.Z.get() : R;  // the explicit models' preconditioner is the identity
    uint32_t *frozen = w.frozen.get(), *active = w.active.get();  // active [1 + steps]: the systems still active after the start and after each step
    const dim3 grid((n32 + 3) / 4), block(256);
    // whether every system is frozen, read from the counter that k_cg_dir filled (tol > 0 only)
    auto all_frozen = [&](uint32_t slot, bool& done) -> int {
        uint32_t left = 0;
        MFX_HIP(hipMemcpyAsync(&left, active + slot, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        done = left == 0;
        return MFX_OK;
    };

    if (implicit) MFX_TRY(foldcg_dense(R, n32, k, m.Minv, frozen, nullptr, Z, st));
    hipLaunchKernelGGL(k_cg_dir, grid, block, 0, st, nsys, k, R, Z, P, 1, w.gamma.get(), frozen, first_active);
    MFX_HIP(hipGetLastError());
    bool done = false;
    if (stop) MFX_TRY(all_frozen(0, done));
    for (int32_t s = 0; s < m.steps && !done; ++s) {
        MFX_TRY(gather());
        if (implicit) MFX_TRY(foldcg_dense(P, n32, k, m.G, frozen, Q, Q, st));
        hipLaunchKernelGGL(k_cg_step, grid, block, 0, st, h.ptr.get(), nsys, T, k, Y, R, P, Q, m.reg, m.lambda, m.tol, w.gamma.get(), w.bb.get(),
                           frozen, counts, fail);
        MFX_HIP(hipGetLastError());
        if (s + 1 == m.steps) break;  // (the direction of a step that never comes)
        if (implicit) MFX_TRY(foldcg_dense(R, n32, k, m.Minv, frozen, nullptr, Z, st));
        hipLaunchKernelGGL(k_cg_dir, grid, block, 0, st, nsys, k, R, Z, P, 0, w.gamma.get(), frozen, stop ? active + s + 1 : nullptr);
        MFX_HIP(hipGetLastError());
        if (stop) MFX_TRY(all_frozen((uint32_t) s + 1, done));
    }
    MFX_HIP(hipStreamSynchronize(st));  // (the workspace goes with this call)
    return MFX_OK;
}

int foldcg_inverse(const float* G, uint32_t k, float* Minv) {
    const size_t n = k;
    std::vector<double> L(n * n, 0.0), Xt(n * n, 0.0);  // G = L L^T; Xt[j][i] = (L^-1)[i][j], rows contiguous
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j <= i; ++j) {
            const double s = (double) G[i * n + j] - dot4(&L[i * n], &L[j * n], j);
            if (j < i) L[i * n + j] = s / L[j * n + j];
            else {
                MFX_REQUIRE(s > 0.0 && std::isfinite(s), "mfx_rec_fold_in_cg_setup: H^T H + lambda I is not positive definite at pivot %zu "
                            "(%g): the factors must be finite", i, s);
                L[i * n + i] = std::sqrt(s);
            }
        }
    for (size_t j = 0; j < n; ++j) {  // column j of L^-1 as row j of Xt, entries i = j .. n - 1
        Xt[j * n + j] = 1.0 / L[j * n + j];
        for (size_t i = j + 1; i < n; ++i) Xt[j * n + i] = -dot4(&L[i * n + j], &Xt[j * n + j], i - j) / L[i * n + i];
    }
    for (size_t i = 0; i < n; ++i)  // G^-1 = L^-T L^-1: entry (i, j), i <= j, = sum over t >= j of Xt[i][t] Xt[j][t]
        for (size_t j = i; j < n; ++j) {
            const float v = (float) dot4(&Xt[i * n + j], &Xt[j * n + j], n - j);
            Minv[i * n + j] = v;
            Minv[j * n + i] = v;
        }
    return MFX_OK;
}

int FoldCgWs::alloc(uint32_t max_seg, uint32_t k, uint32_t nslots, int32_t steps) {
    const size_t nk = std::max<size_t>(1, (size_t) max_seg * k);
    MFX_TRY(R.alloc(nk));
    MFX_TRY(Z.alloc(nk));
    MFX_TRY(P.alloc(nk));
    MFX_TRY(Q.alloc(nk));
    MFX_TRY(part.alloc(std::max<size_t>(1, (size_t) nslots * 2 * k)));
    MFX_TRY(bb.alloc(std::max<uint32_t>(1, max_seg)));
    MFX_TRY(gamma.alloc(std::max<uint32_t>(1, max_seg)));
    MFX_TRY(frozen.alloc(std::max<uint32_t>(1, max_seg)));
    return active.alloc((size_t) steps + 1);
}

int foldcg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, uint32_t k, const FoldCg& m, float* Y, bool warm, int32_t* counts,
                  uint32_t* fail, hipStream_t st, FoldCgWs* cw) {
    const uint32_t nseg = h.nseg;
    if (nseg == 0) return MFX_OK;
    const bool implicit = m.reg == 0;
    MFX_REQUIRE(!implicit || (m.G && m.Minv), "fold-in by conjugate gradients: the implicit model needs G and Minv");
    const size_t nk = (size_t) nseg * k;
    const bool stop = m.tol > 0.f;
    FoldCgWs own;  // the call's own vectors when the caller brought none
    DevBuf<int32_t> own_counts;
    if (cw) {
        MFX_REQUIRE(cw->R.size() >= nk && cw->Z.size() >= nk && cw->P.size() >= nk && cw->Q.size() >= nk &&
                        cw->part.size() >= std::max<size_t>(1, (size_t) h.nslots * 2 * k) && cw->bb.size() >= nseg && cw->gamma.size() >= nseg &&
                        cw->frozen.size() >= nseg && cw->active.size() >= (size_t) m.steps + 1,
                    "conjugate gradients: the caller's workspace is too small for this half");
        if (stop) MFX_HIP(hipMemsetAsync(cw->active.get(), 0, sizeof(uint32_t) * ((size_t) m.steps + 1), st));
    } else {
        cw = &own;
        MFX_TRY(own.R.alloc(nk));
        MFX_TRY(own.P.alloc(nk));
        MFX_TRY(own.Q.alloc(nk));
        if (implicit) MFX_TRY(own.Z.alloc(nk));
        MFX_TRY(own.part.alloc(std::max<size_t>(1, (size_t) h.nslots * 2 * k)));
        MFX_TRY(own.bb.alloc(nseg));
        MFX_TRY(own.gamma.alloc(nseg));
        MFX_TRY(own.frozen.alloc(nseg));
        if (stop) MFX_TRY(own.active.alloc_zero((size_t) m.steps + 1, st));  // [1 + steps]: the rows still active after the start and after each step
    }
    if (!counts) {
        MFX_TRY(own_counts.alloc(nseg));
        counts = own_counts.get();
    }
    float *R = cw->R.get(), *Q = cw->Q.get(), *part = cw->part.get();
    float* Z = implicit ? cw->Z.get() : R;  // the explicit models' preconditioner is the identity
    // b into R; warm: the gathered part of A y0 into Q, then G y0 on top (implicit)
    MFX_TRY(gather(warm ? 3 : 2, h, X, x_rows, k, implicit, m.alpha, Y, nullptr, Q, R, part, st));
    if (warm && implicit) MFX_TRY(foldcg_dense(Y, nseg, k, m.G, nullptr, Q, Q, st));
    hipLaunchKernelGGL(k_foldcg_start, dim3((nseg + 3) / 4), dim3(256), 0, st, h.ptr.get(), nseg, k, Y, R, Z, cw->P.get(), Q, (int32_t) warm, m.reg,
                       m.lambda, m.tol, cw->bb.get(), cw->frozen.get(), counts);
    MFX_HIP(hipGetLastError());
    return cg_iterate(h, 1, k, m, Y, *cw, counts, fail, stop ? cw->active.get() : nullptr,
                      [&] { return gather(1, h, X, x_rows, k, implicit, m.alpha, cw->P.get(), cw->frozen.get(), Q, nullptr, part, st); }, st);
}

}  // namespace mfx
