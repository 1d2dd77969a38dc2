// rec_tiles.hpp -- the pass over the packed H that the recommender's kernels share (recommend.hip: mfx_rec_topn,
// rec_rank.hip: mfx_rec_count): the workgroup shape, the total order, the tile pass itself and its dispatch on KC.
// Device code, included by .hip files only.
#pragma once

#include <algorithm>
#include <type_traits>

#include "common.hpp"

#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())

namespace mfx {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kRecWaves = 4;                 // waves per workgroup
constexpr int kRecThreads = 64 * kRecWaves;
constexpr int kRecUsers = 32 * kRecWaves;    // users per workgroup
constexpr int kTile = 32;                    // items per LDS stage (one 32 x 32 MFMA tile per wave)
constexpr uint32_t kPad = 0xFFFFFFFFu;

// The total order: does (score as, item ai) come before (bs, bi)?  Written without short-circuits: the three compares
// cost less than the branches that `||` and `&&` leave in the per-entry code of the count pass and in the sorts.
__device__ inline bool beats(float as, uint32_t ai, float bs, uint32_t bi) {
    return (as > bs) | ((as == bs) & (ai < bi));
}

__device__ inline int wave_sum(int v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

inline int grid_for(size_t n) { return (int) std::min<size_t>((n + 255) / 256, 4096); }

// What a tile pass reads; the argument structs of the kernels that run one extend it.
struct TileArgs {
    const float* wp;   // [rows][kt]
    const float* hp;   // [nblk][nch][2*KC][32]
    uint32_t cols;
    int kt, nch, nblk, bps;
    const float* fac;  // FAC only: [nblk * 32] per-item factor of the ranking key (NaN: the item is never eligible)
};

// The item of accumulator entry r of a lane whose tile starts at ibase = 32 * tile + 4 * (lane >> 5).
__device__ inline uint32_t acc_item(uint32_t ibase, int r) { return ibase + (r & 3) + 8 * (r >> 2); }

// One LDS stage (NF4 16-byte vectors, contiguous in the packed H) through registers: the loads of stage s+1 are in flight
// while the MFMAs of stage s run.  The registers are a plain vector type: as float4 the compiler keeps stg[] of KC = 32 / 64
// in scratch (32 / 64 bytes per lane stored and reloaded every stage).
template <int NV, int NF4>
__device__ inline void load_stage(f32x4 (&stg)[NV], const float* src, int tid) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int e = tid + v * kRecThreads;
        if (NF4 % kRecThreads == 0 || e < NF4) stg[v] = s4[e];
    }
}
template <int NV, int NF4>
__device__ inline void store_stage(const f32x4 (&stg)[NV], float* dst, int tid) {
    f32x4* d4 = reinterpret_cast<f32x4*>(dst);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int e = tid + v * kRecThreads;
        if (NF4 % kRecThreads == 0 || e < NF4) d4[e] = stg[v];
    }
}

// The pass of one workgroup (kRecThreads threads) over the tiles of item slice `slice`: H double-buffered in LDS and shared
// by the four waves, the packed row `row` of a lane's slot (lane & 31) in registers as the B operand (+0 when !valid), the
// scores of 32 slots x 32 items per wave in acc (several t chunks for k > 128, same order), times the items' factors with
// FAC.  After the last chunk of every tile it calls on_tile(ibase, acc): entry r of acc is the key of item
// acc_item(ibase, r), which may lie past cols.  Control flow is uniform across the workgroup, so on_tile may use wave
// operations; it runs between the stage's MFMAs and the barrier that ends the stage.  (a by value: through a reference
// mfx_rec_count takes one or two VGPRs more for KC <= 16, which costs <2, true> a wave.)
template <int KC, bool FAC, class OnTile>
__device__ __forceinline__ void rec_tile_pass(const TileArgs a, int slice, uint32_t row, bool valid, OnTile&& on_tile) {
    constexpr int STAGE = 2 * KC * kTile;        // floats per LDS stage
    constexpr int NF4 = STAGE / 4;
    constexpr int NV = (NF4 + kRecThreads - 1) / kRecThreads;
    __shared__ __attribute__((aligned(16))) float hb[2][STAGE];

    const int tid = threadIdx.x, h = (tid & 63) >> 5, j = tid & 31;
    const int b0 = slice * a.bps;
    const int b1 = min(a.nblk, b0 + a.bps);
    const int nst = b1 > b0 ? (b1 - b0) * a.nch : 0;

    f32x4 stg[NV];
    float wf[KC];
    f32x16 acc;
    if (nst > 0) {
        load_stage<NV, NF4>(stg, a.hp + (size_t) b0 * a.nch * STAGE, tid);
        store_stage<NV, NF4>(stg, hb[0], tid);
    }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int c = st % a.nch;
        const int blk = b0 + st / a.nch;
        if (st + 1 < nst) load_stage<NV, NF4>(stg, a.hp + (size_t) (b0 * a.nch + st + 1) * STAGE, tid);
        if (a.nch > 1 || st == 0) {
            const float* wr = a.wp + (size_t) row * a.kt + c * 2 * KC + h;
#pragma unroll
            for (int s = 0; s < KC; ++s) wf[s] = valid ? wr[2 * s] : 0.f;
        }
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        }
        const float* hbuf = hb[st & 1] + h * kTile + j;
#pragma unroll
        for (int s = 0; s < KC; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(hbuf[2 * s * kTile], wf[s], acc, 0, 0, 0);

        if (c == a.nch - 1) {
            const uint32_t ibase = (uint32_t) blk * kTile + 4 * h;
            if (FAC) {  // a lane's 16 items are four runs of four ids: one 16-byte load of the factors per run
                const float4* f4 = reinterpret_cast<const float4*>(a.fac + ibase);  // (ibase < 2^32: cols < 2^32 - 1)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 f = f4[2 * g];
                    acc[4 * g] *= f.x; acc[4 * g + 1] *= f.y; acc[4 * g + 2] *= f.z; acc[4 * g + 3] *= f.w;
                }
            }
            on_tile(ibase, acc);
        }
        if (st + 1 < nst) store_stage<NV, NF4>(stg, hb[(st + 1) & 1], tid);
        __syncthreads();
    }
}

// f(std::integral_constant<int, KC>) for the handle's kc (1, 2, 4, ..., 64).
template <class F>
int dispatch_kc(int kc, F&& f) {
    switch (kc) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 4: return f(std::integral_constant<int, 4>());
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        case 32: return f(std::integral_constant<int, 32>());
        default: return f(std::integral_constant<int, 64>());
    }
}

}  // namespace

}  // namespace mfx
