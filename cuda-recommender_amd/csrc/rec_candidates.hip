// rec_candidates.hip -- re-ranking of given candidate lists (mfx_rec_query_candidates) and the scores of given pairs
// (mfx_rec_score) on gfx950.
//
// The second stage of a two-stage recommender: slot q names a user and a strictly ascending list of item ids (a CSR
// row); the answer is the n_top eligible items of the list in the order of mfx_rec_query.  The score of a candidate is
// the explicit fp32 FMA chain over t ascending that mfx_rec_target_keys runs, so one lane owns one candidate's
// accumulator for the whole chain; the work is a gather of rows of hq_ ([cols][kt], the bits of the tiles).
//
//   mfx_cand_check_ptr    the row pointers: from 0, non-decreasing; lists longer than a chunk are collected for the merge.
//   mfx_cand_check_idx    the ids: below cols, strictly ascending within a row.  Reads nothing when the pointers are bad.
//   mfx_cand_pieces       the piece table.  A piece is a slot cut at the multiples of kCandChunk of the global candidate
//                         position: piece g(q) + j of slot q with g(q) = q + ptr[q] / kCandChunk, which is strictly
//                         increasing, so the table needs no scan and the grid is nusers + candidates / kCandChunk
//                         workgroups whatever the lengths: work is scheduled by candidate count, not by slot.
//   mfx_cand_topn         one workgroup per piece: scores its candidates (64 per wave step), drops the excluded, filtered
//                         and NaN ones, sorts (key, item) in LDS and writes the best n_top.  A list of at most kCandChunk
//                         candidates is one piece whatever boundary it crosses (its second piece returns at once) and
//                         its keys never leave the CU; a longer list leaves one sorted partial list per piece.
//   mfx_cand_merge        one workgroup per long list: a running best n_top in LDS takes the partial lists one bitonic
//                         merge each.  (mfx_rec_merge of recommend.hip sorts all partial lists of a slot at once, which
//                         caps them at 8192 entries; a whole catalogue of 10^6 items at n_top = 1024 leaves 500 000.)
//   mfx_cand_score        mfx_rec_score: the same scoring step over a flat list of pairs, the W row per lane.
//   mfx_expl_topn / mfx_expl_merge / mfx_expl_totals
//                         mfx_rec_explain's second half ("Explanations" below): the same piece scheme over the query rows'
//                         own entries, the chain against z = A^-1 h_target instead of a row of W.
//
// Two forms of the gather, LOAD_GROUP or not (DESIGN 5.8 has the measurement): one lane reads its own row with 16-byte
// loads, or eight lanes read one 128-byte line of a row each, eight rows per wave instruction, and hand the lines to
// the owner lanes through a wave-private LDS stage whose next fill is in flight while the chains run.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rec_cand.hpp"  // the piece size, lane_chain, excluded, Events: shared with rec_diversify.hip
#include "recommend.hpp"

namespace mfx {

namespace {

constexpr int kStageT = 32;         // floats of a row per LDS stage: one 128-byte line
constexpr int kStageStride = 36;    // floats between the rows of a stage: 16-byte reads of 16 consecutive rows hit 64 distinct banks
constexpr int kStageRows = 64;
constexpr int kLanesPerRow = kStageT / 4, kRowsPerLoad = 64 / kLanesPerRow;
constexpr unsigned long long kCandFine = ~0ull;

// What the two check kernels leave: the first offending slot and what it offends (slot << 2 | kind; kCandFine: nothing),
// the number of lists longer than a chunk, and ptr[nusers].
struct CandInfo {
    unsigned long long first;
    uint32_t nlong, total;
};

struct CandArgs {
    const float* wp;           // [rows][kt]
    const float* hq;           // [cols][kt]
    const uint32_t* users;     // NULL: slot q is user q
    const uint32_t* ptr;       // [nu + 1]
    const uint32_t* idx;
    const uint32_t* piece_slot;  // [nu + total / kCandChunk]
    const uint32_t* ex_ptr;    // NULL: no exclusion
    const uint32_t* ex_idx;
    const float* fac;          // NULL, or [nblk * 32]: 1 / NaN per item (the item filter)
    int k, kt, n_top;
    uint32_t b0;               // first piece of this launch
    float* part_s;             // [2 * (total / kCandChunk + 2)][n_top] partial lists of the long slots
    uint32_t* part_i;
    uint32_t* out_items;       // [nu][n_top]
    float* out_scores;         // may be NULL
    uint32_t* n_el;            // may be NULL; zeroed, pieces add
};

// The scores of the 64 candidates of a wave, lane l owning (row wr of W, item): every lane of the wave calls this, the
// ones without a candidate with item 0.  stg: the wave's kStageRows x kStageStride floats of LDS (LOAD_GROUP only).
// Rows shorter than a line (kt < 32) take the lane form either way.
template <bool LOAD_GROUP>
__device__ __forceinline__ float score_wave(const float* hq, const float* wr, uint32_t item, int k, int kt, float* stg, int lane) {
    if (!LOAD_GROUP || kt < kStageT) return lane_chain(wr, hq + (size_t) item * kt, k, kt);
    const int sub = lane & (kLanesPerRow - 1), r0 = lane / kLanesPerRow;
    const float* src[kRowsPerLoad];  // the line of stage 0 this lane fetches for row r0 + 8 i of the wave
#pragma unroll
    for (int i = 0; i < kRowsPerLoad; ++i) src[i] = hq + (size_t) __shfl(item, r0 + kRowsPerLoad * i) * kt + 4 * sub;
    f32x4 v[kRowsPerLoad];
#pragma unroll
    for (int i = 0; i < kRowsPerLoad; ++i) v[i] = *reinterpret_cast<const f32x4*>(src[i]);
    float acc = 0.f;
    const float* mine = stg + lane * kStageStride;
    for (int t0 = 0; t0 < k; t0 += kStageT) {  // (kt is a multiple of 32 here: every line lies inside its row)
        wave_sync();  // the chains of the stage before have read
#pragma unroll
        for (int i = 0; i < kRowsPerLoad; ++i)
            *reinterpret_cast<f32x4*>(stg + (r0 + kRowsPerLoad * i) * kStageStride + 4 * sub) = v[i];
        if (t0 + kStageT < k) {
#pragma unroll
            for (int i = 0; i < kRowsPerLoad; ++i) v[i] = *reinterpret_cast<const f32x4*>(src[i] + t0 + kStageT);
        }
        wave_sync();
        const float* w = wr + t0;
        if (k - t0 >= kStageT) {
#pragma unroll
            for (int g = 0; g < kStageT / 4; ++g) {
                const f32x4 h = *reinterpret_cast<const f32x4*>(mine + 4 * g);
                const f32x4 ww = *reinterpret_cast<const f32x4*>(w + 4 * g);
                acc = __builtin_fmaf(h.x, ww.x, acc);
                acc = __builtin_fmaf(h.y, ww.y, acc);
                acc = __builtin_fmaf(h.z, ww.z, acc);
                acc = __builtin_fmaf(h.w, ww.w, acc);
            }
        } else {  // the last stage of a k that is no multiple of 32: the +0 padding of the rows must not be added (-0 + +0 = +0)
            for (int t = 0; t < k - t0; ++t) acc = __builtin_fmaf(mine[t], w[t], acc);
        }
    }
    return acc;
}

// The stages (k, j), j = k/2 .. 1, of a bitonic sorting network over P entries by the workgroup, best first.  Stages
// with j <= 64 keep every wave inside its own 128 entries, so a run of them needs the wave's own ordering only; `last`
// is the j of the stage before (> 64: other waves wrote what this stage reads).
__device__ inline void wg_bitonic_phase(float* ks, uint32_t* is, int P, int k, int& last, int tid) {
    for (int j = k >> 1; j > 0; j >>= 1) {
        if (j > 64 || last > 64) __syncthreads();
        else wave_sync();
        last = j;
        for (int x = tid; x < (P >> 1); x += kCandThreads) {
            const int a = ((x & ~(j - 1)) << 1) | (x & (j - 1));
            const int b = a + j;
            const float sa = ks[a], sb = ks[b];
            const uint32_t ia = is[a], ib = is[b];
            const bool sw = (a & k) == 0 ? beats(sb, ib, sa, ia) : beats(sa, ia, sb, ib);
            if (sw) {
                ks[a] = sb; ks[b] = sa;
                is[a] = ib; is[b] = ia;
            }
        }
    }
}

// bad ptr: kind 0 of slot q.  Long lists go to long_list in any order (their results do not depend on it).
__global__ void mfx_cand_check_ptr(const uint32_t* ptr, uint32_t nu, CandInfo* info, uint32_t* long_list) {
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < nu; q += (size_t) gridDim.x * blockDim.x) {
        const uint32_t lo = ptr[q], hi = ptr[q + 1];
        if (lo > hi || (q == 0 && lo != 0)) atomicMin(&info->first, (unsigned long long) q << 2);
        else if (hi - lo > (uint32_t) kCandChunk) long_list[atomicAdd(&info->nlong, 1u)] = (uint32_t) q;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info->total = ptr[nu];
}

// kind 1: an id >= cols; kind 2: an id not above the one before it in its row.  The slot of a position is searched
// only where one of the two shows (kind 2: at about every other row start of a valid batch).
__global__ void mfx_cand_check_idx(const uint32_t* ptr, const uint32_t* idx, uint32_t nu, uint32_t cols, CandInfo* info) {
    if (info->first != kCandFine) return;  // bad pointers: idx need not have ptr[nu] entries
    const size_t total = ptr[nu];
    for (size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t) gridDim.x * blockDim.x) {
        const uint32_t c = idx[p];
        const int kind = c >= cols ? 1 : (p > 0 && idx[p - 1] >= c) ? 2 : 0;
        if (!kind) continue;
        uint32_t lo = 0, hi = nu;  // the first slot whose row starts after p; the one before it holds p
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ptr[mid] <= p) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t s = lo - 1;
        if (kind == 1 || ptr[s] != p) atomicMin(&info->first, (unsigned long long) s << 2 | (unsigned) kind);
    }
}

__global__ void mfx_cand_pieces(const uint32_t* ptr, uint32_t nu, uint32_t* piece_slot) {
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < nu; q += (size_t) gridDim.x * blockDim.x) {
        const uint32_t lo = ptr[q], hi = ptr[q + 1];
        const size_t g = q + lo / kCandChunk;
        const uint32_t np = 1 + hi / kCandChunk - lo / kCandChunk;
        for (uint32_t j = 0; j < np; ++j) piece_slot[g + j] = (uint32_t) q;
    }
}

template <bool LOAD_GROUP>
__global__ __launch_bounds__(kCandThreads) void mfx_cand_topn(CandArgs a) {
    __shared__ float ks[kCandChunk];
    __shared__ uint32_t is[kCandChunk];
    __shared__ __attribute__((aligned(16))) float stg[LOAD_GROUP ? kCandWaves * kStageRows * kStageStride : 4];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t b = a.b0 + blockIdx.x;
    const uint32_t q = a.piece_slot[b];
    const uint32_t lo_s = a.ptr[q], hi_s = a.ptr[q + 1];
    const uint32_t blk0 = lo_s / kCandChunk, j = b - q - blk0;
    const bool whole = hi_s - lo_s <= (uint32_t) kCandChunk;
    if (whole && j) return;  // (the list crosses a chunk boundary: its first piece took all of it)
    uint32_t lo = lo_s, hi = hi_s;
    if (!whole) {
        const uint64_t c0 = (uint64_t) (blk0 + j) * kCandChunk;
        lo = c0 > lo_s ? (uint32_t) c0 : lo_s;
        hi = c0 + kCandChunk < hi_s ? (uint32_t) (c0 + kCandChunk) : hi_s;
    }
    const uint32_t n = hi - lo;  // <= kCandChunk; 0 for an empty list and for the piece after a list that ends on a boundary
    const uint32_t u = __builtin_amdgcn_readfirstlane(a.users ? a.users[q] : q);  // (one slot per workgroup: the W row is a scalar operand)
    const float* wr = a.wp + (size_t) u * a.kt;
    uint32_t elo = 0, ehi = 0;
    if (a.ex_ptr) { elo = a.ex_ptr[u]; ehi = a.ex_ptr[u + 1]; }
    int P = 64;
    while (P < (int) n) P <<= 1;

    int cnt = 0;
    for (uint32_t base = wave * 64; base < n; base += kCandThreads) {  // (uniform in the wave)
        const uint32_t c = base + lane;
        const bool valid = c < n;
        const uint32_t item = valid ? a.idx[lo + c] : 0;
        const float s = score_wave<LOAD_GROUP>(a.hq, wr, item, a.k, a.kt, stg + wave * kStageRows * kStageStride, lane);
        const float key = a.fac ? s * a.fac[item] : s;
        const bool ok = valid && key == key && !(ehi > elo && excluded(a.ex_idx, elo, ehi, item));
        if (valid) {
            ks[c] = ok ? key : -INFINITY;
            is[c] = ok ? item : kPad;
        }
        cnt += ok;
    }
    for (int c = (int) n + tid; c < P; c += kCandThreads) { ks[c] = -INFINITY; is[c] = kPad; }
    if (a.n_el) {
        cnt = wave_sum(cnt);
        if (lane == 0 && cnt) atomicAdd(a.n_el + q, (uint32_t) cnt);
    }
    int last = 128;  // (a barrier before the first stage)
    for (int k = 2; k <= P; k <<= 1) wg_bitonic_phase(ks, is, P, k, last, tid);
    __syncthreads();

    const size_t o = whole ? (size_t) q * a.n_top : (size_t) (2 * (size_t) (blk0 + j) + (j == 0)) * a.n_top;
    uint32_t* oi = whole ? a.out_items : a.part_i;
    float* os = whole ? a.out_scores : a.part_s;
    for (int e = tid; e < a.n_top; e += kCandThreads) {
        oi[o + e] = e < P ? is[e] : kPad;
        if (os) os[o + e] = e < P ? ks[e] : -INFINITY;
    }
}

// M: the power of two >= n_top.  A block of the global candidate positions holds at most one piece that is the first
// of its list and one that is not, hence the two partial lists per block.
__global__ __launch_bounds__(kCandThreads) void mfx_cand_merge(CandArgs a, const uint32_t* long_list, int M) {
    __shared__ float ks[2048];
    __shared__ uint32_t is[2048];
    const int tid = threadIdx.x;
    const uint32_t q = long_list[blockIdx.x];
    const uint32_t lo_s = a.ptr[q], hi_s = a.ptr[q + 1];
    const uint32_t blk0 = lo_s / kCandChunk, np = 1 + hi_s / kCandChunk - blk0;
    for (int e = tid; e < M; e += kCandThreads) { ks[e] = -INFINITY; is[e] = kPad; }
    for (uint32_t j = 0; j < np; ++j) {
        const size_t src = (size_t) (2 * (size_t) (blk0 + j) + (j == 0)) * a.n_top;
        __syncthreads();
        for (int e = tid; e < M; e += kCandThreads) {  // the partial list, worst first: best n_top so far + it = one bitonic run
            ks[2 * M - 1 - e] = e < a.n_top ? a.part_s[src + e] : -INFINITY;
            is[2 * M - 1 - e] = e < a.n_top ? a.part_i[src + e] : kPad;
        }
        int last = 128;
        wg_bitonic_phase(ks, is, 2 * M, 2 * M, last, tid);
    }
    __syncthreads();
    const size_t o = (size_t) q * a.n_top;
    for (int e = tid; e < a.n_top; e += kCandThreads) {
        a.out_items[o + e] = is[e];
        if (a.out_scores) a.out_scores[o + e] = ks[e];
    }
}

template <bool LOAD_GROUP>
__global__ __launch_bounds__(kCandThreads) void mfx_cand_score(const float* wp, const float* hq, const uint32_t* users,
                                                               const uint32_t* items, uint32_t np, int k, int kt, float* scores) {
    __shared__ __attribute__((aligned(16))) float stg[LOAD_GROUP ? kCandWaves * kStageRows * kStageStride : 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (size_t base = ((size_t) blockIdx.x * kCandWaves + wave) * 64; base < np; base += (size_t) gridDim.x * kCandThreads) {
        const size_t p = base + lane;
        const bool valid = p < np;
        const uint32_t item = valid ? items[p] : 0, u = valid ? users[p] : 0;
        const float s = score_wave<LOAD_GROUP>(hq, wp + (size_t) u * kt, item, k, kt, stg + wave * kStageRows * kStageStride, lane);
        if (valid) scores[p] = s;
    }
}

// ---- Explanations (mfx_rec_explain) ------------------------------------------------------------------------
// The score of target t for fold-in row q splits over the row's entries: <h_t, w_q> = sum_e b_e <h_e, z_qt>, z_qt = A_q^-1 h_t
// (the multi-right-hand-side solve of als_solver.hip leaves Z).  A piece of work is (slot, target, at most kCandChunk
// consecutive entries of the row): the pieces of a slot are those of mfx_cand_pieces over the ROW pointers, the target is
// blockIdx.y, so the grid follows the entry count.  Lane-owned chain with z as the left operand, one multiply by the
// entry's weight, then the sort of mfx_cand_topn with the POSITION in the row as the id: ids may repeat in a row, positions
// do not, and "contribution descending, then position ascending" is the total order of beats().  The item ids come back
// in on the way out.  A row longer than a piece leaves one sorted partial list per piece and target; mfx_expl_merge merges
// them as mfx_cand_merge does.
// (Every target of a slot gathers the same rows of H.  One workgroup per (piece, target) reads them once per target, from
// the L2 after the first; keeping n_targets accumulators per lane to read them once would cost up to 64 VGPRs and serialise
// the n_targets sorts in one workgroup -- not done.)
struct ExplArgs {
    const float* Z;            // [nu][nt][k]
    const float* hx;           // [cols + 1][k]: H row-major, the bits of the tiles
    const uint32_t* ptr;       // [nu + 1] the query rows
    const uint32_t* idx;
    const float* val;
    const uint32_t* targets;   // [nu][nt]; kPad: no target
    const uint32_t* piece_slot;
    int k, nt, n_expl;
    int implicit;              // the weight of an entry r: 0: r; 1: add_rn(alpha0, fp32(alpha r)), and only r > 0 counts
    float alpha, alpha0;
    uint32_t b0;
    size_t part_stride;        // entries of part_s / part_i per target
    float* part_s;             // [nt][2 * (total / kCandChunk + 2)][n_expl]
    uint32_t* part_i;
    uint32_t* out_items;       // [nu][nt][n_expl]
    float* out_contrib;
};

__device__ __forceinline__ float expl_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float expl_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

__global__ __launch_bounds__(kCandThreads) void mfx_expl_topn(ExplArgs a) {
    __shared__ float ks[kCandChunk];
    __shared__ uint32_t is[kCandChunk];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t b = a.b0 + blockIdx.x, t = blockIdx.y;
    const uint32_t q = a.piece_slot[b];
    const uint32_t lo_s = a.ptr[q], hi_s = a.ptr[q + 1];
    const uint32_t blk0 = lo_s / kCandChunk, j = b - q - blk0;
    const bool whole = hi_s - lo_s <= (uint32_t) kCandChunk;
    if (whole && j) return;  // (the row crosses a chunk boundary: its first piece took all of it)
    uint32_t lo = lo_s, hi = hi_s;
    if (!whole) {
        const uint64_t c0 = (uint64_t) (blk0 + j) * kCandChunk;
        lo = c0 > lo_s ? (uint32_t) c0 : lo_s;
        hi = c0 + kCandChunk < hi_s ? (uint32_t) (c0 + kCandChunk) : hi_s;
    }
    const uint32_t n = hi - lo;
    const size_t qt = (size_t) q * a.nt + t;
    const bool has_target = a.targets[qt] != kPad;  // (uniform in the workgroup)
    const float* z = a.Z + qt * a.k;
    int P = 64;
    while (P < (int) n) P <<= 1;
    for (uint32_t base = wave * 64; base < n; base += kCandThreads) {  // (uniform in the wave)
        const uint32_t c = base + lane;
        const bool valid = c < n;
        const uint32_t item = valid ? a.idx[lo + c] : 0;
        const float r = valid ? a.val[lo + c] : 0.f;
        const float d = lane_chain(z, a.hx + (size_t) item * a.k, a.k, a.k);
        const float w = a.implicit ? expl_add(a.alpha0, expl_mul(a.alpha, r)) : r;
        const float key = expl_mul(w, d);
        const bool ok = valid && has_target && key == key && (!a.implicit || r > 0.f);
        if (valid) {
            ks[c] = ok ? key : -INFINITY;
            is[c] = ok ? lo - lo_s + c : kPad;
        }
    }
    for (int c = (int) n + tid; c < P; c += kCandThreads) { ks[c] = -INFINITY; is[c] = kPad; }
    int last = 128;  // (a barrier before the first stage)
    for (int kk = 2; kk <= P; kk <<= 1) wg_bitonic_phase(ks, is, P, kk, last, tid);
    __syncthreads();
    if (whole) {
        const size_t o = qt * a.n_expl;
        for (int e = tid; e < a.n_expl; e += kCandThreads) {
            const uint32_t pos = e < P ? is[e] : kPad;
            a.out_items[o + e] = pos == kPad ? kPad : a.idx[lo_s + pos];
            a.out_contrib[o + e] = e < P ? ks[e] : -INFINITY;
        }
    } else {
        const size_t o = t * a.part_stride + (size_t) (2 * (size_t) (blk0 + j) + (j == 0)) * a.n_expl;
        for (int e = tid; e < a.n_expl; e += kCandThreads) {
            a.part_i[o + e] = e < P ? is[e] : kPad;
            a.part_s[o + e] = e < P ? ks[e] : -INFINITY;
        }
    }
}

// One workgroup per (long row, target); M: the power of two >= n_expl.  The partial lists hold positions in the row.
__global__ __launch_bounds__(kCandThreads) void mfx_expl_merge(ExplArgs a, const uint32_t* long_list, int M) {
    __shared__ float ks[128];
    __shared__ uint32_t is[128];
    const int tid = threadIdx.x;
    const uint32_t q = long_list[blockIdx.x], t = blockIdx.y;
    const uint32_t lo_s = a.ptr[q], hi_s = a.ptr[q + 1];
    const uint32_t blk0 = lo_s / kCandChunk, np = 1 + hi_s / kCandChunk - blk0;
    for (int e = tid; e < M; e += kCandThreads) { ks[e] = -INFINITY; is[e] = kPad; }
    for (uint32_t j = 0; j < np; ++j) {
        const size_t src = t * a.part_stride + (size_t) (2 * (size_t) (blk0 + j) + (j == 0)) * a.n_expl;
        __syncthreads();
        for (int e = tid; e < M; e += kCandThreads) {  // the partial list, worst first: best n_expl so far + it = one bitonic run
            ks[2 * M - 1 - e] = e < a.n_expl ? a.part_s[src + e] : -INFINITY;
            is[2 * M - 1 - e] = e < a.n_expl ? a.part_i[src + e] : kPad;
        }
        int last = 128;
        wg_bitonic_phase(ks, is, 2 * M, 2 * M, last, tid);
    }
    __syncthreads();
    const size_t o = ((size_t) q * a.nt + t) * a.n_expl;
    for (int e = tid; e < a.n_expl; e += kCandThreads) {
        a.out_items[o + e] = is[e] == kPad ? kPad : a.idx[lo_s + is[e]];
        a.out_contrib[o + e] = ks[e];
    }
}

// totals[q][t]: the pair-scoring chain of mfx_cand_score over (Y[q], H[target]), both rows [k] floats apart; -inf for kPad
__global__ void mfx_expl_totals(const float* Y, const float* hx, const uint32_t* targets, size_t n, int nt, int k, float* totals) {
    for (size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t) gridDim.x * blockDim.x) {
        const uint32_t tg = targets[p];
        totals[p] = tg == kPad ? -INFINITY : lane_chain(Y + (p / nt) * k, hx + (size_t) tg * k, k, k);
    }
}

// every target below cols or kPad; else the first offending position into *first
__global__ void mfx_expl_check_targets(const uint32_t* targets, size_t n, uint32_t cols, unsigned long long* first) {
    for (size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t) gridDim.x * blockDim.x) {
        const uint32_t tg = targets[p];
        if (tg >= cols && tg != kPad) atomicMin(first, (unsigned long long) p);
    }
}

// Which form of the gather a call takes: `measured` (what was faster on the MI355X) unless MFX_CAND_LOAD=group
// or =lane forces one -- the hook of tools/candidates_bench.py, which records both; the results are the same bits.
bool load_by_group(bool measured) {
    const char* v = std::getenv("MFX_CAND_LOAD");
    if (v && std::strcmp(v, "group") == 0) return true;
    if (v && std::strcmp(v, "lane") == 0) return false;
    return measured;
}
// mfx_cand_topn: the lane groups win where a row is 512 bytes or more and the lists are long (k = 128 / 256, 1000 candidates:
// 1.2x / 1.7x), and lose below that (k <= 64 at every length, every k at 100 candidates, where a workgroup has one step per
// wave and the 52 KiB of LDS leave three workgroups per CU instead of eight).  512 per slot lies between the two measured lengths.
constexpr int kGroupMinKt = 128;
constexpr uint64_t kGroupMinMeanList = 512;

}  // namespace

int Recommender::cand_stage(const char* fn, uint32_t nu, const uint32_t* cand_ptr, const uint32_t* cand_idx, mfx_memspace space,
                            CandLists& l) {
    l.ptr = cand_ptr;
    l.idx = cand_idx;
    l.idx_grid = 2048;  // (the number of candidates is still on the device: a fixed grid strides over them)
    if (space != MFX_HOST) return MFX_OK;
    const uint32_t total = cand_ptr[nu];
    MFX_REQUIRE(total == 0 || cand_idx, "%s: cand_idx is NULL but the lists hold %u candidates", fn, total);
    MFX_TRY(l.d_ptr.alloc((size_t) nu + 1));
    MFX_TRY(l.d_ptr.upload(cand_ptr, (size_t) nu + 1, MFX_HOST, st_));
    l.ptr = l.d_ptr.get();
    if (total) {
        MFX_TRY(l.d_idx.alloc(total));
        MFX_TRY(l.d_idx.upload(cand_idx, total, MFX_HOST, st_));
    }
    l.idx = l.d_idx.get();
    l.idx_grid = grid_for(total);
    return MFX_OK;
}

// the one host round trip: the rows are valid or not, how many candidates there are, how many lists are longer than a chunk
int Recommender::cand_check(const char* fn, uint32_t nu, CandLists& l) {
    hipStream_t st = st_;
    DevBuf<CandInfo> info;
    MFX_TRY(info.alloc(1));
    MFX_TRY(l.long_list.alloc(nu));
    CandInfo hi{kCandFine, 0, 0};
    MFX_HIP(hipMemcpyAsync(info.get(), &hi, sizeof(hi), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mfx_cand_check_ptr, dim3(grid_for(nu)), dim3(256), 0, st, l.ptr, nu, info.get(), l.long_list.get());
    MFX_LAUNCH_CHECK();
    if (l.idx) {
        hipLaunchKernelGGL(mfx_cand_check_idx, dim3(l.idx_grid), dim3(256), 0, st, l.ptr, l.idx, nu, (uint32_t) cols_, info.get());
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipMemcpyAsync(&hi, info.get(), sizeof(hi), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (hi.first != kCandFine) {
        const unsigned long long slot = hi.first >> 2;
        switch ((int) (hi.first & 3)) {
            case 0: return fail(MFX_ERR_INVALID, "%s: cand_ptr is not non-decreasing from 0 at slot %llu", fn, slot);
            case 1: return fail(MFX_ERR_INVALID, "%s: the list of slot %llu has an item id out of range [0, %lld)", fn, slot, (long long) cols_);
            default: return fail(MFX_ERR_INVALID, "%s: the item ids of slot %llu are not strictly ascending", fn, slot);
        }
    }
    l.total = hi.total;
    l.nlong = hi.nlong;
    MFX_REQUIRE(l.total == 0 || l.idx, "%s: cand_idx is NULL but the lists hold %u candidates", fn, l.total);
    return MFX_OK;
}

int Recommender::query_candidates(int64_t nusers, const uint32_t* users, const uint32_t* cand_ptr, const uint32_t* cand_idx,
                                  int32_t flags, int32_t n_top, uint32_t* items, float* scores, uint32_t* n_eligible,
                                  mfx_memspace space) {
    const char* fn = "mfx_rec_query_candidates";
    MFX_REQUIRE(n_top >= 1 && n_top <= 1024, "%s: n_top must be in [1, 1024] (got %d)", fn, n_top);
    MFX_REQUIRE(nusers >= 0 && nusers < (int64_t) 0xFFFFFFFFll, "%s: bad nusers %lld", fn, (long long) nusers);
    MFX_REQUIRE(users || nusers <= rows_, "%s: users = NULL needs nusers <= rows (%lld > %lld)", fn, (long long) nusers, (long long) rows_);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    MFX_REQUIRE((flags & ~MFX_CAND_NO_EXCLUDE) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) flags);
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(cand_ptr, "%s: cand_ptr is NULL", fn);
    MFX_REQUIRE(items, "%s: items is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const uint32_t nu = (uint32_t) nusers;
    const bool host = space == MFX_HOST;
    cand_s_[0] = cand_s_[1] = cand_s_[2] = 0.0;
    Events ev;
    MFX_TRY(ev.create());
    MFX_HIP(hipEventRecord(ev.e[0], st));

    DevBuf<uint32_t> d_users, piece_slot, d_items, d_nel, part_i;
    DevBuf<float> d_scores, part_s;
    CandLists lists;
    const uint32_t* du = nullptr;
    MFX_TRY(stage_ids(users, nu, space, (uint32_t) rows_, "mfx_rec_query_candidates: user id", d_users, &du));
    MFX_TRY(cand_stage(fn, nu, cand_ptr, cand_idx, space, lists));
    MFX_TRY(cand_check(fn, nu, lists));
    const uint32_t* dp = lists.ptr;
    const uint32_t* di = lists.idx;
    const uint32_t total = lists.total;

    const uint64_t npieces = (uint64_t) nu + total / kCandChunk;
    MFX_TRY(piece_slot.alloc(npieces));
    hipLaunchKernelGGL(mfx_cand_pieces, dim3(grid_for(nu)), dim3(256), 0, st, dp, nu, piece_slot.get());
    MFX_LAUNCH_CHECK();
    uint32_t* oi = items;
    float* os = scores;
    uint32_t* onel = n_eligible;
    if (host) {
        MFX_TRY(d_items.alloc((size_t) nu * n_top));
        oi = d_items.get();
        if (scores) { MFX_TRY(d_scores.alloc((size_t) nu * n_top)); os = d_scores.get(); }
        if (n_eligible) { MFX_TRY(d_nel.alloc(nu)); onel = d_nel.get(); }
    }
    if (onel) MFX_HIP(hipMemsetAsync(onel, 0, sizeof(uint32_t) * nu, st));
    if (lists.nlong) {
        const size_t np = 2 * ((size_t) total / kCandChunk + 2) * n_top;
        MFX_TRY(part_s.alloc(np));
        MFX_TRY(part_i.alloc(np));
    }
    MFX_TRY(ensure_hq());
    MFX_HIP(hipEventRecord(ev.e[1], st));

    CandArgs a{};
    a.wp = wp_.get(); a.hq = hq_.get();
    a.users = du; a.ptr = dp; a.idx = di; a.piece_slot = piece_slot.get();
    const bool ex = has_ex_ && !(flags & MFX_CAND_NO_EXCLUDE);
    a.ex_ptr = ex ? ex_ptr_.get() : nullptr; a.ex_idx = ex_idx_.get();
    a.fac = fac_keep_.get();
    a.k = (int) k_; a.kt = kt_; a.n_top = n_top;
    a.part_s = part_s.get(); a.part_i = part_i.get();
    a.out_items = oi; a.out_scores = os; a.n_el = onel;
    const bool group = load_by_group(kt_ >= kGroupMinKt && (uint64_t) total >= kGroupMinMeanList * nu);
    for (uint64_t b0 = 0; b0 < npieces; b0 += 1u << 30) {  // (grid.x stays below 2^31)
        a.b0 = (uint32_t) b0;
        const dim3 grid((uint32_t) std::min<uint64_t>(npieces - b0, 1u << 30));
        if (group) hipLaunchKernelGGL((mfx_cand_topn<true>), grid, dim3(kCandThreads), 0, st, a);
        else hipLaunchKernelGGL((mfx_cand_topn<false>), grid, dim3(kCandThreads), 0, st, a);
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipEventRecord(ev.e[2], st));
    if (lists.nlong) {
        int M = 1;
        while (M < n_top) M <<= 1;
        hipLaunchKernelGGL(mfx_cand_merge, dim3(lists.nlong), dim3(kCandThreads), 0, st, a, (const uint32_t*) lists.long_list.get(), M);
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipEventRecord(ev.e[3], st));
    if (host) {
        MFX_HIP(hipMemcpyAsync(items, oi, sizeof(uint32_t) * nu * n_top, hipMemcpyDeviceToHost, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, os, sizeof(float) * nu * n_top, hipMemcpyDeviceToHost, st));
        if (n_eligible) MFX_HIP(hipMemcpyAsync(n_eligible, onel, sizeof(uint32_t) * nu, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        MFX_HIP(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        cand_s_[i] = 1e-3 * ms;
    }
    return MFX_OK;
}

int Recommender::explain_check_targets(const char* fn, const uint32_t* d_targets, size_t n, int32_t n_targets) {
    DevBuf<unsigned long long> first;
    MFX_TRY(first.alloc(1));
    MFX_HIP(hipMemsetAsync(first.get(), 0xFF, sizeof(unsigned long long), st_));
    hipLaunchKernelGGL(mfx_expl_check_targets, dim3(grid_for(n)), dim3(256), 0, st_, d_targets, n, (uint32_t) cols_, first.get());
    MFX_LAUNCH_CHECK();
    unsigned long long bad = ~0ull;
    MFX_HIP(hipMemcpyAsync(&bad, first.get(), sizeof(bad), hipMemcpyDeviceToHost, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    MFX_REQUIRE(bad == ~0ull, "%s: target %llu of slot %llu is neither an item id in [0, %lld) nor the padding 0xFFFFFFFF", fn,
                bad % (unsigned long long) n_targets, bad / (unsigned long long) n_targets, (long long) cols_);
    return MFX_OK;
}

// Device pointers throughout.  d_items / d_contrib: [nu][nt][n_expl] (unread for n_expl = 0), d_totals: [nu][nt] or NULL.
int Recommender::explain_lists(const AlsHalf& h, const uint32_t* d_targets, int32_t nt, const float* Z, const float* Y, int32_t n_expl,
                               uint32_t* d_items, float* d_contrib, float* d_totals) {
    hipStream_t st = st_;
    const uint32_t nu = h.nseg;
    if (d_totals) {
        const size_t n = (size_t) nu * nt;
        hipLaunchKernelGGL(mfx_expl_totals, dim3(grid_for(n)), dim3(256), 0, st, Y, (const float*) hx_.get(), d_targets, n, (int) nt, (int) k_,
                           d_totals);
        MFX_LAUNCH_CHECK();
    }
    if (n_expl == 0) return MFX_OK;
    // the rows longer than a piece (the pointers were checked on the way in)
    DevBuf<CandInfo> info;
    DevBuf<uint32_t> long_list, piece_slot, part_i;
    DevBuf<float> part_s;
    MFX_TRY(info.alloc(1));
    MFX_TRY(long_list.alloc(nu));
    CandInfo hi{kCandFine, 0, 0};
    MFX_HIP(hipMemcpyAsync(info.get(), &hi, sizeof(hi), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mfx_cand_check_ptr, dim3(grid_for(nu)), dim3(256), 0, st, (const uint32_t*) h.ptr.get(), nu, info.get(), long_list.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipMemcpyAsync(&hi, info.get(), sizeof(hi), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    const uint32_t total = (uint32_t) h.nnz;
    const uint64_t npieces = (uint64_t) nu + total / kCandChunk;
    MFX_TRY(piece_slot.alloc(npieces));
    hipLaunchKernelGGL(mfx_cand_pieces, dim3(grid_for(nu)), dim3(256), 0, st, (const uint32_t*) h.ptr.get(), nu, piece_slot.get());
    MFX_LAUNCH_CHECK();
    ExplArgs a{};
    a.Z = Z; a.hx = hx_.get(); a.ptr = h.ptr.get(); a.idx = h.idx.get(); a.val = h.val.get(); a.targets = d_targets;
    a.piece_slot = piece_slot.get();
    a.k = (int) k_; a.nt = nt; a.n_expl = n_expl;
    a.implicit = plan_.implicit();
    a.alpha = plan_.alpha; a.alpha0 = plan_.alpha0;
    a.part_stride = 2 * ((size_t) total / kCandChunk + 2) * n_expl;
    if (hi.nlong) {
        MFX_TRY(part_s.alloc(a.part_stride * nt));
        MFX_TRY(part_i.alloc(a.part_stride * nt));
    }
    a.part_s = part_s.get(); a.part_i = part_i.get();
    a.out_items = d_items; a.out_contrib = d_contrib;
    for (uint64_t b0 = 0; b0 < npieces; b0 += 1u << 30) {  // (grid.x stays below 2^31)
        a.b0 = (uint32_t) b0;
        const dim3 grid((uint32_t) std::min<uint64_t>(npieces - b0, 1u << 30), (uint32_t) nt);
        hipLaunchKernelGGL(mfx_expl_topn, grid, dim3(kCandThreads), 0, st, a);
        MFX_LAUNCH_CHECK();
    }
    if (hi.nlong) {
        int M = 1;
        while (M < n_expl) M <<= 1;
        hipLaunchKernelGGL(mfx_expl_merge, dim3(hi.nlong, (uint32_t) nt), dim3(kCandThreads), 0, st, a, (const uint32_t*) long_list.get(), M);
        MFX_LAUNCH_CHECK();
    }
    return MFX_OK;
}

int Recommender::score(int64_t npairs, const uint32_t* users, const uint32_t* items, float* scores, mfx_memspace space) {
    const char* fn = "mfx_rec_score";
    MFX_REQUIRE(npairs >= 0 && npairs < (int64_t) 0xFFFFFFFFll, "%s: bad npairs %lld", fn, (long long) npairs);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    if (npairs == 0) return MFX_OK;
    MFX_REQUIRE(users && items, "%s: users or items is NULL", fn);
    MFX_REQUIRE(scores, "%s: scores is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const uint32_t np = (uint32_t) npairs;
    cand_s_[0] = cand_s_[1] = cand_s_[2] = 0.0;
    Events ev;
    MFX_TRY(ev.create());
    MFX_HIP(hipEventRecord(ev.e[0], st));
    DevBuf<uint32_t> d_users, d_items;
    DevBuf<float> d_scores;
    const uint32_t* du = nullptr;
    const uint32_t* di = nullptr;
    MFX_TRY(stage_ids(users, np, space, (uint32_t) rows_, "mfx_rec_score: user id", d_users, &du));
    MFX_TRY(stage_ids(items, np, space, (uint32_t) cols_, "mfx_rec_score: item id", d_items, &di));
    float* os = scores;
    if (space == MFX_HOST) {
        MFX_TRY(d_scores.alloc(np));
        os = d_scores.get();
    }
    MFX_TRY(ensure_hq());
    MFX_HIP(hipEventRecord(ev.e[1], st));
    const dim3 grid((uint32_t) std::min<size_t>(((size_t) np + kCandThreads - 1) / kCandThreads, 8 * (size_t) cus_));
    if (load_by_group(true))  // (the W row is a per-lane gather here too: 0.046 against 0.076 ms for 1.4 M pairs at k = 64)
        hipLaunchKernelGGL((mfx_cand_score<true>), grid, dim3(kCandThreads), 0, st, wp_.get(), hq_.get(), du, di, np, (int) k_, kt_, os);
    else
        hipLaunchKernelGGL((mfx_cand_score<false>), grid, dim3(kCandThreads), 0, st, wp_.get(), hq_.get(), du, di, np, (int) k_, kt_, os);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev.e[2], st));
    if (space == MFX_HOST) MFX_HIP(hipMemcpyAsync(scores, os, sizeof(float) * np, hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 2; ++i) {
        float ms = 0.f;
        MFX_HIP(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        cand_s_[i] = 1e-3 * ms;
    }
    return MFX_OK;
}

}  // namespace mfx
