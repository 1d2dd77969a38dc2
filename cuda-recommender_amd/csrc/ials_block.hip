// ials_block.hip -- implicit-feedback ALS by block subspace sweeps ("iALS++", Rendle et al. 2021) on gfx950: ranks up to
// 1024 with blocks of d <= 128 coordinates.  A half-sweep keeps the score s_j = <x_j, y> of every stored pair and, for
// every block pi = [b d, min(k, (b + 1) d)) in ascending order, minimises each segment's objective exactly over y_pi:
//     (G[pi, pi] + sum_j w_j x_jpi x_jpi^T) z = sum_{r_j > 0} ((1 + w_j) - w_j s_j) x_jpi - G[pi, :] y
//     y_pi += z,   s_j += <x_jpi, z>
// (z = -Delta of include/mfx.h).  The kernels of this file, in the order of a half-sweep:
//   k_ialsb_gram_tile / _reduce   G = X^T X + lambda I: one wavefront per (32 x 32 tile of the upper block triangle, row
//                                 partition) on v_mfma_f32_32x32x2_f32, the partials summed in partition order
//   k_ialsb_pack / _pack_g        X block-major (block b: [rows + 1][width], last row zeros) so that the block systems gather
//                                 contiguous rows of `width` floats; the diagonal blocks of G contiguous
//   k_ialsb_scores                s_j from the full rows (one wavefront per work item of AlsHalf), empty segments: y = 0
//   k_ialsb_gy<ND>                P = Y G[:, pi] for every segment: 32 segments x width per wavefront on the MFMA
//   (k_ialsb_gram / gram16 / reduce: the block systems, als_solver.hip compiled as ials_block_step.hip)
//   k_ialsb_update                y_pi += z and s_j += <x_jpi, z> (one wavefront per work item)
// Fold-in (ialsb_fold_launch) repeats the sweep part over query rows against a side packed once, with a stop per row:
//   k_ialsb_fold_init / _freeze   the empty rows zeroed and frozen from the start; after a sweep a row frozen earlier gets its
//                                 bits back, any other row counts the sweep and freezes once it moved by <= tol of its size
// No float atomics; every sum has a fixed order: results are bitwise reproducible.
//
// Explicit feedback (alsb_*, the last part of this file) runs the same sweep on the objective sum_j (r_j - <x_j, y>)^2 +
// rho |y|^2 of a segment: no base Gramian, so no k_ialsb_gram_tile, _pack_g or _gy; in their place
//   k_alsb_p                      P = rho y_pi, rho = lambda or fp32(lambda * n) for a segment of n entries
//   (k_alsb_gram / gram16 / reduce: the block systems, als_solver.hip compiled as als_block_step.hip)
// and k_ialsb_pack, _scores, _update, _fold_init and _freeze as they are.
#include <algorithm>
#include <cmath>

#include "als_solver.hpp"

namespace mfx {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr uint32_t kGramWaves = 8192;   // wavefronts of the base Gramian aimed at (tiles x row partitions)
constexpr uint32_t kGramMinRows = 64;   // rows per partition at least
constexpr uint32_t kGramMaxParts = 1024;

uint32_t gram_tiles(uint32_t k) { const uint32_t nt = (k + 31) / 32; return nt * (nt + 1) / 2; }
uint32_t gram_parts(uint32_t rows, uint32_t k) {
    const uint32_t by_rows = std::max<uint32_t>(1, (rows + kGramMinRows - 1) / kGramMinRows);
    const uint32_t want = std::max<uint32_t>(1, kGramWaves / gram_tiles(k));
    return std::min(std::min(want, by_rows), kGramMaxParts);
}

// start of block b in the block-major copy of X [rows][k]: every block 16-byte aligned (k_ialsb_gram16 gathers with 16-byte loads)
__host__ __device__ __forceinline__ size_t xb_offset(uint32_t rows, uint32_t d, uint32_t b) {
    return (size_t) b * (((size_t) rows + 1) * d + 3 & ~(size_t) 3);
}

// tile t of the upper block triangle in the order (0,0), (0,1), ... (0,nt-1), (1,1), ...
__device__ __forceinline__ void tile_of(uint32_t t, uint32_t nt, uint32_t& I, uint32_t& J) {
    uint32_t i = 0;
    while (t >= nt - i) { t -= nt - i; ++i; }
    I = i; J = i + t;
}

// Lane l = (c31, h) supplies X[row q + h][32 I + c31] as the A operand and X[row q + h][32 J + c31] as the B operand:
// the tile accumulates sum over rows of x_I x_J^T as an exact fp32 fma chain in row order.
__global__ __launch_bounds__(64) void k_ialsb_gram_tile(const float* __restrict__ X, uint32_t rows, uint32_t k, uint32_t nt, uint32_t per,
                                                        float* __restrict__ part) {
    constexpr int U = 8;  // row pairs per step: all loads of a step go out before its MFMAs
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    uint32_t I, J;
    tile_of(blockIdx.x, nt, I, J);
    const uint32_t lo = blockIdx.y * per, hi = min(rows, lo + per);
    const uint32_t ci = 32 * I + c31, cj = 32 * J + c31;
    const bool oki = ci < k, okj = cj < k;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (uint32_t q0 = lo; q0 < hi; q0 += 2 * U) {
        float a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = q0 + 2 * u + h;
            a[u] = row < hi && oki ? X[(size_t) row * k + ci] : 0.f;
            b[u] = row < hi && okj ? X[(size_t) row * k + cj] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
    float* w = part + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * 1024;
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r * 64 + lane] = acc[r];
}

// One thread per accumulator slot: partitions summed in order; register r of lane (c31, h) of tile (I, J) is entry
// (32 I + (r & 3) + 8 (r >> 2) + 4 h, 32 J + c31).  A diagonal tile holds (i, j) and (j, i) with the same sums.
__global__ __launch_bounds__(256) void k_ialsb_gram_reduce(const float* __restrict__ part, uint32_t nparts, uint32_t ntiles, uint32_t nt,
                                                           uint32_t k, float lambda, float* __restrict__ G) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ntiles * 1024) return;
    float s = 0.f;
    for (uint32_t p = 0; p < nparts; ++p) s += part[(size_t) p * ntiles * 1024 + e];
    uint32_t I, J;
    tile_of(e >> 10, nt, I, J);
    const uint32_t r = (e >> 6) & 15, lane = e & 63;
    const uint32_t row = 32 * I + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = 32 * J + (lane & 31);
    if (row < k && col < k && row <= col) {
        const float v = row == col ? s + lambda : s;
        G[(size_t) row * k + col] = v;
        G[(size_t) col * k + row] = v;
    }
}

// X [rows][k] -> block-major: element (row, col) of block b = col / d at Xb[xb_offset(rows, d, b) + row width_b + (col - b d)];
// row `rows` of every block is all zeros (the gather target of positions past a segment's end).  One wavefront per row.
__global__ __launch_bounds__(256) void k_ialsb_pack(const float* __restrict__ X, uint32_t rows, uint32_t k, uint32_t d, float* __restrict__ Xb) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row > rows) return;
    for (uint32_t col = threadIdx.x & 63; col < k; col += 64) {
        const uint32_t b = col / d, w = min(d, k - b * d);
        Xb[xb_offset(rows, d, b) + (size_t) row * w + (col - b * d)] = row < rows ? X[(size_t) row * k + col] : 0.f;
    }
}
// the diagonal blocks of G: block b contiguous [width_b][width_b] at Gbb + b d d
__global__ __launch_bounds__(256) void k_ialsb_pack_g(const float* __restrict__ G, uint32_t k, uint32_t d, float* __restrict__ Gbb) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;  // (row of G, column inside the row's block)
    if (e >= k * d) return;
    const uint32_t row = e / d, c = e % d, b = row / d, w = min(d, k - b * d);
    if (c < w) Gbb[(size_t) b * d * d + (size_t) (row - b * d) * w + c] = G[(size_t) row * k + b * d + c];
}

__device__ __forceinline__ float wave_sum(float v) {  // butterfly over the 64 lanes: the same value, in a fixed order, in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float half_sum(float v) {  // the same over each half of the wavefront
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int kMaxK64 = kIalsBlockMaxRank / 64;  // columns per lane of a full row

// Scores of one work item's entries from the full rows: lane l holds y[l + 64 i]; an entry's row is read coalesced (k
// floats), multiplied and summed over the wavefront.  Two entries per step.  An empty segment's row of Y is zeroed.
__global__ __launch_bounds__(64) void k_ialsb_scores(const AlsItem* __restrict__ items, uint32_t nitems, const uint32_t* __restrict__ idx,
                                                     const float* __restrict__ X, float* __restrict__ Y, uint32_t k,
                                                     float* __restrict__ score) {
    const uint32_t lane = threadIdx.x & 63;
    if (blockIdx.x >= nitems) return;
    const AlsItem it = items[blockIdx.x];
    float* y = Y + (size_t) it.seg * k;
    if (it.hi == it.lo) {
        for (uint32_t c = lane; c < k; c += 64) y[c] = 0.f;
        return;
    }
    float yv[kMaxK64];
#pragma unroll
    for (int i = 0; i < kMaxK64; ++i) yv[i] = 64 * i + lane < k ? y[64 * i + lane] : 0.f;
    for (uint32_t q = it.lo; q < it.hi; q += 2) {
        const bool two = q + 1 < it.hi;
        const float* x0 = X + (size_t) idx[q] * k;
        const float* x1 = X + (size_t) idx[two ? q + 1 : q] * k;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxK64; ++i) {
            if (64u * i < k) {  // wave-uniform
                const bool in = 64 * i + lane < k;
                s0 = __builtin_fmaf(in ? x0[64 * i + lane] : 0.f, yv[i], s0);
                s1 = __builtin_fmaf(in ? x1[64 * i + lane] : 0.f, yv[i], s1);
            }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            score[q] = s0;
            if (two) score[q + 1] = s1;
        }
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

// P[seg][j] = sum_t Y[seg][t] G[b0 + j][t] (G is symmetric) for 32 segments x `width` columns per wavefront, ND = tiles of
// 32 columns.  MFMA step e of the 8-column group at kk: lane (r31, h) supplies Y[seg0 + r31][kk + 4 h + e] and
// G[b0 + 32 t + r31][kk + 4 h + e] -- four steps per 16-byte load, the sum over t in a fixed (permuted) order.
template <int ND>
__global__ __launch_bounds__(256) void k_ialsb_gy(const float* __restrict__ Y, uint32_t nseg, uint32_t k, const float* __restrict__ G,
                                                  uint32_t b0, uint32_t width, float* __restrict__ P) {
    const uint32_t lane = threadIdx.x & 63, r31 = lane & 31, h = lane >> 5;
    const uint32_t seg0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (seg0 >= nseg) return;
    const bool vec = (k & 3) == 0;
    const bool sok = seg0 + r31 < nseg;
    const float* yrow = Y + (size_t) (sok ? seg0 + r31 : seg0) * k;
    const float* grow[ND];
    bool gok[ND];
    f32x16 acc[ND];
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        gok[t] = 32 * t + r31 < width;
        grow[t] = G + (size_t) (b0 + (gok[t] ? 32 * t + r31 : 0)) * k;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    }
    for (uint32_t kk = 0; kk < k; kk += 8) {
        const uint32_t c = kk + 4 * h;
        const f32x4 a = load4(yrow, c, sok, k, vec);
        f32x4 b[ND];
#pragma unroll
        for (int t = 0; t < ND; ++t) b[t] = load4(grow[t], c, gok[t], k, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < ND; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[t][e], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < ND; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t seg = seg0 + (r & 3) + 8 * (r >> 2) + 4 * h, col = 32 * t + r31;
            if (seg < nseg && col < width) P[(size_t) seg * width + col] = acc[t][r];
        }
}

// y_pi += z (by the work item that holds the segment's first entry) and s_j += <x_jpi, z> for the item's entries: each half
// of the wavefront takes one entry, lane l32 the columns l32 + 32 i; four entry pairs in flight.
__global__ __launch_bounds__(64) void k_ialsb_update(const AlsItem* __restrict__ items, uint32_t nitems, const uint32_t* __restrict__ ptr,
                                                     const uint32_t* __restrict__ idx, const float* __restrict__ Xb, uint32_t x_rows,
                                                     const float* __restrict__ Z, uint32_t width, float* __restrict__ Y, uint32_t k,
                                                     uint32_t b0, float* __restrict__ score) {
    constexpr int U = 4, C = kIalsBlockMaxBlock / 32;
    const uint32_t lane = threadIdx.x & 63, l32 = lane & 31, h = lane >> 5;
    if (blockIdx.x >= nitems) return;
    const AlsItem it = items[blockIdx.x];
    if (it.hi == it.lo) return;
    float zv[C];
#pragma unroll
    for (int i = 0; i < C; ++i) zv[i] = 32 * i + l32 < width ? Z[(size_t) it.seg * width + 32 * i + l32] : 0.f;
    if (h == 0 && it.lo == ptr[it.seg]) {
        float* y = Y + (size_t) it.seg * k + b0;
#pragma unroll
        for (int i = 0; i < C; ++i)
            if (32 * i + l32 < width) y[32 * i + l32] += zv[i];
    }
    for (uint32_t q0 = it.lo; q0 < it.hi; q0 += 2 * U) {
        float xv[U][C];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q = q0 + 2 * u + h;
            const float* x = Xb + (size_t) (q < it.hi ? idx[q] : x_rows) * width;
#pragma unroll
            for (int i = 0; i < C; ++i) xv[u][i] = 32 * i + l32 < width ? x[32 * i + l32] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < C; ++i) s = __builtin_fmaf(xv[u][i], zv[i], s);
            s = half_sum(s);
            const uint32_t q = q0 + 2 * u + h;
            if (l32 == 0 && q < it.hi) score[q] += s;
        }
    }
}

__device__ __forceinline__ float wave_max(float v) {  // maximum over the 64 lanes (no order to fix: max is exact)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Before the first sweep of a fold-in, one wavefront per row: an empty row is zeroed (whatever the start row held), frozen and
// counts 0 sweeps; any other row counts `count` (0 when k_ialsb_freeze does the counting).  frozen may be NULL (no stop rule).
__global__ __launch_bounds__(256) void k_ialsb_fold_init(const uint32_t* __restrict__ ptr, uint32_t nseg, uint32_t k, float* __restrict__ Y,
                                                         uint32_t* __restrict__ frozen, int32_t* __restrict__ sweeps, int32_t count) {
    const uint32_t lane = threadIdx.x & 63, seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const bool empty = ptr[seg + 1] == ptr[seg];
    if (empty)
        for (uint32_t c = lane; c < k; c += 64) Y[(size_t) seg * k + c] = 0.f;
    if (lane == 0) {
        if (frozen) frozen[seg] = empty;
        if (sweeps) sweeps[seg] = empty ? 0 : count;
    }
}

// After a sweep, one wavefront per row, lane l the columns l + 64 i of Y and of `snap`, the copy of Y taken before the sweep.
// A row frozen earlier: the sweep is undone (its bits never change again).  Any other row: the sweep counts, and the row is
// frozen from now on if max_c |y[c] - snap[c]| <= tol max_c |y[c]| (fp32, maxima only: no order); the rows that stay active
// are counted into *active (one vector atomic per row, an integer: the sum has no order either).
__global__ __launch_bounds__(256) void k_ialsb_freeze(float* __restrict__ Y, const float* __restrict__ snap, uint32_t nseg, uint32_t k, float tol,
                                                      uint32_t* __restrict__ frozen, int32_t* __restrict__ sweeps, uint32_t* __restrict__ active) {
    const uint32_t lane = threadIdx.x & 63, seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    float* y = Y + (size_t) seg * k;
    const float* s = snap + (size_t) seg * k;
    if (frozen[seg]) {  // wave-uniform
        for (uint32_t c = lane; c < k; c += 64) y[c] = s[c];
        return;
    }
    float dmax = 0.f, ymax = 0.f;
    for (uint32_t c = lane; c < k; c += 64) {
        const float v = y[c];
        dmax = fmaxf(dmax, fabsf(v - s[c]));
        ymax = fmaxf(ymax, fabsf(v));
    }
    dmax = wave_max(dmax);
    ymax = wave_max(ymax);
    if (lane == 0) {
        sweeps[seg] += 1;
        if (dmax <= tol * ymax) frozen[seg] = 1;
        else atomicAdd(active, 1u);
    }
}

// Explicit feedback: P[seg][c] = rho y[b0 + c] for the block at b0, rho = lambda or fp32(lambda * n) for a segment of n
// entries (one rounding, as k_alsn_* form it); one thread per (segment, column of the block)
__global__ __launch_bounds__(256) void k_alsb_p(const float* __restrict__ Y, const uint32_t* __restrict__ ptr, uint32_t nseg, uint32_t k, uint32_t b0,
                                                uint32_t width, float lambda, int32_t reg, float* __restrict__ P) {
    const size_t e = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t) nseg * width) return;
    const uint32_t seg = (uint32_t) (e / width), c = (uint32_t) (e % width);
    const float rho = reg ? lambda * (float) (ptr[seg + 1] - ptr[seg]) : lambda;
    P[e] = rho * Y[(size_t) seg * k + b0 + c];
}

// Implicit objective with a regulariser per segment (k_ialsrb_*): P[seg][c] = fmaf(rho[seg], y[b0 + c], P[seg][c]) on top of
// P = Y G0[:, pi] as k_ialsb_gy left it; one thread per (segment, column of the block)
__global__ __launch_bounds__(256) void k_ialsrb_p(const float* __restrict__ Y, const float* __restrict__ rho, uint32_t nseg, uint32_t k, uint32_t b0,
                                                  uint32_t width, float* __restrict__ P) {
    const size_t e = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t) nseg * width) return;
    const uint32_t seg = (uint32_t) (e / width), c = (uint32_t) (e % width);
    P[e] = __builtin_fmaf(rho[seg], Y[(size_t) seg * k + b0 + c], P[e]);
}

// the first position whose value is not finite into *first_bad (grid-stride, one atomic per thread that found one)
__global__ __launch_bounds__(256) void k_alsb_check(uint64_t n, const float* __restrict__ val, unsigned long long* __restrict__ first_bad) {
    unsigned long long bad = ~0ull;
    for (uint64_t q = (uint64_t) blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t) gridDim.x * 256)
        if (!(fabsf(val[q]) <= 3.402823466e38f) && q < bad) bad = q;  // (NaN fails the compare)
    if (bad != ~0ull) atomicMin(first_bad, bad);
}

template <int ND>
void launch_gy(const float* Y, uint32_t nseg, uint32_t k, const float* G, uint32_t b0, uint32_t width, float* P, hipStream_t st) {
    hipLaunchKernelGGL(k_ialsb_gy<ND>, dim3((nseg + 127) / 128), dim3(256), 0, st, Y, nseg, k, G, b0, width, P);
}

// The sweeps of a fold-in with the stop per row; sweep() launches one sweep in place on Y
template <class Sweep>
int fold_loop(const AlsHalf& h, uint32_t k, float* Y, int32_t sweeps, float tol, int32_t* counts, hipStream_t st, Sweep&& sweep) {
    const uint32_t nseg = h.nseg;
    if (nseg == 0) return MFX_OK;
    const dim3 grid((nseg + 3) / 4), block(256);
    if (!(tol > 0.f)) {  // every non-empty row gets `sweeps`: no snapshot, no flags, nothing read back
        hipLaunchKernelGGL(k_ialsb_fold_init, grid, block, 0, st, h.ptr.get(), nseg, k, Y, (uint32_t*) nullptr, counts, sweeps);
        MFX_HIP(hipGetLastError());
        for (int32_t s = 0; s < sweeps; ++s) MFX_TRY(sweep());
        return MFX_OK;
    }
    DevBuf<float> snap;
    DevBuf<uint32_t> frozen, active;  // active [sweeps]: the rows still moving after each sweep
    DevBuf<int32_t> own_counts;
    MFX_TRY(snap.alloc((size_t) nseg * k));
    MFX_TRY(frozen.alloc(nseg));
    MFX_TRY(active.alloc_zero((size_t) sweeps, st));
    if (!counts) {
        MFX_TRY(own_counts.alloc(nseg));
        counts = own_counts.get();
    }
    hipLaunchKernelGGL(k_ialsb_fold_init, grid, block, 0, st, h.ptr.get(), nseg, k, Y, frozen.get(), counts, 0);
    MFX_HIP(hipGetLastError());
    for (int32_t s = 0; s < sweeps; ++s) {
        MFX_HIP(hipMemcpyAsync(snap.get(), Y, sizeof(float) * (size_t) nseg * k, hipMemcpyDeviceToDevice, st));
        MFX_TRY(sweep());
        hipLaunchKernelGGL(k_ialsb_freeze, grid, block, 0, st, Y, snap.get(), nseg, k, tol, frozen.get(), counts, active.get() + s);
        MFX_HIP(hipGetLastError());
        uint32_t left = 0;
        MFX_HIP(hipMemcpyAsync(&left, active.get() + s, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        if (left == 0) break;
    }
    return MFX_OK;
}

// One block (d >= k): the step is the solve itself, whatever the start.  The step forms the residual of the start in fp32,
// so a start adds rounding of the size of |y0|: next to an answer 58 times smaller (implicit model, k = 1 over 8000 rows,
// y0 ~ 0.1) that alone is a backward error of 6e-5.  A one-block sweep therefore starts every row from zero.
int one_block_start(float* Y, uint32_t nseg, uint32_t k, uint32_t d, hipStream_t st) {
    if (d >= k) MFX_HIP(hipMemsetAsync(Y, 0, sizeof(float) * (size_t) nseg * k, st));
    return MFX_OK;
}

}  // namespace

int IalsBlock::alloc(uint32_t k_, uint32_t d_, uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st) {
    k = k_; d = d_;
    const uint32_t nblocks = (k + d - 1) / d;
    MFX_TRY(G.alloc((size_t) k * k));
    MFX_TRY(gpart.alloc((size_t) gram_parts(max_rows_x, k) * gram_tiles(k) * 1024));
    MFX_TRY(Xb.alloc(xb_offset(max_rows_x, d, nblocks)));
    MFX_TRY(Gbb.alloc((size_t) nblocks * d * d));
    return alloc_half(max_seg, nnz, nslots, st);
}

int IalsBlock::alloc_gramian(uint32_t k_, uint32_t max_rows_x) {
    k = k_; d = 0;
    MFX_TRY(G.alloc((size_t) k * k));
    return gpart.alloc((size_t) gram_parts(max_rows_x, k) * gram_tiles(k) * 1024);
}

int IalsBlock::alloc_half(uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st) {
    MFX_TRY(P.alloc(std::max<size_t>(1, (size_t) max_seg * d)));
    MFX_TRY(Z.alloc(std::max<size_t>(1, (size_t) max_seg * d)));
    MFX_TRY(score.alloc_zero(nnz + kAlsEntryPad, st));  // (the padding stays zero: what the Gramian kernels read past the end is finite)
    MFX_TRY(ws.alloc(std::max<size_t>(1, als_ws_floats(nslots, d))));
    return MFX_OK;
}

int ialsb_gramian(IalsBlock& b, const float* X, uint32_t rows, float lambda, hipStream_t st) {
    const uint32_t k = b.k, nt = (k + 31) / 32, ntiles = gram_tiles(k), nparts = gram_parts(rows, k);
    const uint32_t per = (rows + nparts - 1) / nparts;
    MFX_REQUIRE((size_t) nparts * ntiles * 1024 <= b.gpart.size(), "implicit ALS by block sweeps: Gramian workspace too small for %u rows", rows);
    hipLaunchKernelGGL(k_ialsb_gram_tile, dim3(ntiles, nparts), dim3(64), 0, st, X, rows, k, nt, per, b.gpart.get());
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ialsb_gram_reduce, dim3(ntiles * 4), dim3(256), 0, st, b.gpart.get(), nparts, ntiles, nt, k, lambda, b.G.get());
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int ialsb_pack_launch(IalsBlock& b, const float* X, uint32_t x_rows, hipStream_t st) {
    const uint32_t k = b.k, d = b.d;
    MFX_REQUIRE(xb_offset(x_rows, d, (k + d - 1) / d) <= b.Xb.size(), "implicit ALS by block sweeps: workspace too small for %u fixed rows", x_rows);
    hipLaunchKernelGGL(k_ialsb_pack, dim3(x_rows / 4 + 1), dim3(256), 0, st, X, x_rows, k, d, b.Xb.get());
    MFX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ialsb_pack_g, dim3((k * d + 255) / 256), dim3(256), 0, st, b.G.get(), k, d, b.Gbb.get());
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int ialsb_sweep_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, uint32_t* spd_fail,
                       hipStream_t st, float alpha0, const float* rho) {
    const uint32_t k = b.k, d = b.d;
    MFX_REQUIRE(xb_offset(x_rows, d, (k + d - 1) / d) <= b.Xb.size() && (size_t) h.nseg * d <= std::max<size_t>(1, b.P.size()) &&
                    (size_t) h.nseg * d <= std::max<size_t>(1, b.Z.size()) && h.nnz + kAlsEntryPad <= b.score.size() &&
                    als_ws_floats(h.nslots, d) <= std::max<size_t>(1, b.ws.size()),
                "implicit ALS by block sweeps: workspace too small for this half");
    if (h.nseg == 0) return MFX_OK;
    MFX_TRY(one_block_start(Y, h.nseg, k, d, st));
    hipLaunchKernelGGL(k_ialsb_scores, dim3(h.nitems), dim3(64), 0, st, h.items.get(), h.nitems, h.idx.get(), X, Y, k, b.score.get());
    MFX_HIP(hipGetLastError());
    for (uint32_t b0 = 0, blk = 0; b0 < k; b0 += d, ++blk) {
        const uint32_t width = std::min(d, k - b0);
        switch ((width + 31) / 32) {
            case 1: launch_gy<1>(Y, h.nseg, k, b.G.get(), b0, width, b.P.get(), st); break;
            case 2: launch_gy<2>(Y, h.nseg, k, b.G.get(), b0, width, b.P.get(), st); break;
            case 3: launch_gy<3>(Y, h.nseg, k, b.G.get(), b0, width, b.P.get(), st); break;
            default: launch_gy<4>(Y, h.nseg, k, b.G.get(), b0, width, b.P.get(), st); break;
        }
        MFX_HIP(hipGetLastError());
        const float* Xblk = b.Xb.get() + xb_offset(x_rows, d, blk);
        if (rho) {  // b.G is G0 = fp32(alpha0 X^T X): the regulariser's share of P, then the k_ialsrb_* systems
            hipLaunchKernelGGL(k_ialsrb_p, dim3((uint32_t) (((size_t) h.nseg * width + 255) / 256)), dim3(256), 0, st, Y, rho, h.nseg, k, b0, width,
                               b.P.get());
            MFX_HIP(hipGetLastError());
            MFX_TRY(ialsrb_step_launch(h, Xblk, x_rows, b.Z.get(), width, b.Gbb.get() + (size_t) blk * d * d, alpha, alpha0, rho, b.score.get(),
                                       b.P.get(), b.ws.get(), spd_fail, st));
        } else
            MFX_TRY(ialsb_step_launch(h, Xblk, x_rows, b.Z.get(), width, b.Gbb.get() + (size_t) blk * d * d, alpha, b.score.get(), b.P.get(),
                                      b.ws.get(), spd_fail, st));
        hipLaunchKernelGGL(k_ialsb_update, dim3(h.nitems), dim3(64), 0, st, h.items.get(), h.nitems, h.ptr.get(), h.idx.get(), Xblk, x_rows,
                           b.Z.get(), width, Y, k, b0, b.score.get());
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

int ialsb_half_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, uint32_t* spd_fail,
                      hipStream_t st, float alpha0, const float* rho) {
    if (h.nseg == 0) return MFX_OK;
    MFX_TRY(ialsb_pack_launch(b, X, x_rows, st));
    return ialsb_sweep_launch(b, h, X, x_rows, Y, alpha, spd_fail, st, alpha0, rho);
}

int ialsrb_gramian(IalsBlock& b, const float* X, uint32_t rows, float alpha0, hipStream_t st) {
    MFX_TRY(ialsb_gramian(b, X, rows, 0.f, st));  // (S + 0 = S, bit for bit)
    return ialsr_scale_launch(b.G.get(), (size_t) b.k * b.k, alpha0, st);
}

int ialsb_fold_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float alpha, int32_t sweeps, float tol,
                      int32_t* counts, uint32_t* spd_fail, hipStream_t st, float alpha0, const float* rho) {
    return fold_loop(h, b.k, Y, sweeps, tol, counts, st,
                     [&]() { return ialsb_sweep_launch(b, h, X, x_rows, Y, alpha, spd_fail, st, alpha0, rho); });
}

// ---- Explicit feedback ------------------------------------------------------------------------------------------
int IalsBlock::alloc_explicit(uint32_t k_, uint32_t d_, uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st) {
    k = k_; d = d_;
    MFX_TRY(Xb.alloc(xb_offset(max_rows_x, d, (k + d - 1) / d)));
    return alloc_half(max_seg, nnz, nslots, st);
}

int als_check_finite(const float* d_val, uint64_t n, const char* what, hipStream_t st) {
    if (n == 0) return MFX_OK;
    DevBuf<unsigned long long> flag;
    MFX_TRY(flag.alloc(1));
    MFX_HIP(hipMemsetAsync(flag.get(), 0xFF, sizeof(unsigned long long), st));
    const uint32_t grid = (uint32_t) std::min<uint64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_alsb_check, dim3(grid), dim3(256), 0, st, n, d_val, flag.get());
    MFX_HIP(hipGetLastError());
    unsigned long long bad = ~0ull;
    MFX_HIP(hipMemcpyAsync(&bad, flag.get(), sizeof(bad), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (bad == ~0ull) return MFX_OK;
    float v = 0.f;
    MFX_HIP(hipMemcpy(&v, d_val + bad, sizeof(v), hipMemcpyDeviceToHost));
    return fail(MFX_ERR_INVALID, "%s %g at position %llu: finite values required", what, (double) v, bad);
}

int alsb_pack_launch(IalsBlock& b, const float* X, uint32_t x_rows, hipStream_t st) {
    const uint32_t k = b.k, d = b.d;
    MFX_REQUIRE(xb_offset(x_rows, d, (k + d - 1) / d) <= b.Xb.size(), "explicit ALS by block sweeps: workspace too small for %u fixed rows", x_rows);
    hipLaunchKernelGGL(k_ialsb_pack, dim3(x_rows / 4 + 1), dim3(256), 0, st, X, x_rows, k, d, b.Xb.get());
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int alsb_sweep_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg,
                      uint32_t* spd_fail, hipStream_t st) {
    const uint32_t k = b.k, d = b.d;
    MFX_REQUIRE(xb_offset(x_rows, d, (k + d - 1) / d) <= b.Xb.size() && (size_t) h.nseg * d <= std::max<size_t>(1, b.P.size()) &&
                    (size_t) h.nseg * d <= std::max<size_t>(1, b.Z.size()) && h.nnz + kAlsEntryPad <= b.score.size() &&
                    als_ws_floats(h.nslots, d) <= std::max<size_t>(1, b.ws.size()),
                "explicit ALS by block sweeps: workspace too small for this half");
    if (h.nseg == 0) return MFX_OK;
    MFX_TRY(one_block_start(Y, h.nseg, k, d, st));
    hipLaunchKernelGGL(k_ialsb_scores, dim3(h.nitems), dim3(64), 0, st, h.items.get(), h.nitems, h.idx.get(), X, Y, k, b.score.get());
    MFX_HIP(hipGetLastError());
    for (uint32_t b0 = 0, blk = 0; b0 < k; b0 += d, ++blk) {
        const uint32_t width = std::min(d, k - b0);
        hipLaunchKernelGGL(k_alsb_p, dim3((uint32_t) (((size_t) h.nseg * width + 255) / 256)), dim3(256), 0, st, Y, h.ptr.get(), h.nseg, k, b0,
                           width, lambda, reg, b.P.get());
        MFX_HIP(hipGetLastError());
        const float* Xblk = b.Xb.get() + xb_offset(x_rows, d, blk);
        MFX_TRY(alsb_step_launch(h, Xblk, x_rows, b.Z.get(), width, lambda, reg, b.score.get(), b.P.get(), b.ws.get(), spd_fail, st));
        hipLaunchKernelGGL(k_ialsb_update, dim3(h.nitems), dim3(64), 0, st, h.items.get(), h.nitems, h.ptr.get(), h.idx.get(), Xblk, x_rows,
                           b.Z.get(), width, Y, k, b0, b.score.get());
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

int alsb_half_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg,
                     uint32_t* spd_fail, hipStream_t st) {
    if (h.nseg == 0) return MFX_OK;
    MFX_TRY(alsb_pack_launch(b, X, x_rows, st));
    return alsb_sweep_launch(b, h, X, x_rows, Y, lambda, reg, spd_fail, st);
}

int alsb_fold_launch(IalsBlock& b, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, float lambda, int32_t reg, int32_t sweeps,
                     float tol, int32_t* counts, uint32_t* spd_fail, hipStream_t st) {
    return fold_loop(h, b.k, Y, sweeps, tol, counts, st, [&]() { return alsb_sweep_launch(b, h, X, x_rows, Y, lambda, reg, spd_fail, st); });
}

}  // namespace mfx
