// knn_device.hpp -- the shared layer of the item models on the interaction matrix: knn.hip (mfx_knn_*), slim.hip (mfx_slim_*)
// and ease.hip (mfx_ease_*).  Everything here sits in an anonymous namespace: each unit compiles its own copy, as knn.hip did
// while this text was part of it.  DESIGN 5.20 lists which kernel is an instance of what.
//
// A workgroup owns one output row (the neighbours of an item, the scores of a query user, a row of X^T X) and walks the item
// axis in tiles of T accumulators:
//   add      the term source adds its terms into the tile's T 64-bit integers in LDS with no-return LDS atomic adds (integer
//            adds commute exactly: no order of arrival changes a sum);
//   scan     every non-zero accumulator becomes a candidate (fp32 of the sum, item) and is cleared in the same pass, so the
//            tile is all zeros again for the next tile and the next row;
//   select   a candidate that beats() the threshold -- the keep-th entry of the running list once that is full -- goes into
//            the LDS candidate area behind the list; one that finds the area full stays in its accumulator, list and
//            candidates are sorted together (bitonic, the total order beats()), the best `keep` stay, and the tile is
//            scanned again for what is left.
// Device side: knn_begin / knn_scan / knn_sort_keep are the selection (knn_scan over KeyOfSum for sums, over KeyOfBits for
// ease.hip's fp32 scores), knn_row is add, scan and select over a term source, BuildSrc the term source of the three build
// kernels and knn_build_items / knn_build_tiles their work queue and tile walk, knn_diag the diagonal of X^T X, k_knn_rows the recommend kernel of item-kNN and SLIM.
// Host side: the checks of the matrix (check_x, StagedX, work_order), Staged / Out for arrays in either memory space,
// BuildPass for the launch of a build kernel and rows_recommend, the one body of the three mfx_*_recommend.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "rec_tiles.hpp"

namespace mfx {

namespace {

constexpr int kKnnThreads = 512;             // 8 waves: latency of the row loads is hidden by waves, not by unrolling
constexpr int kKnnWaves = kKnnThreads / 64;
constexpr int kKnnBatch = 4;                 // independent loads a thread keeps in flight in the term loops
constexpr uint32_t kKnnMaxEntries = 1u << 21;  // entries of a column (build) or of a query row (recommend)
constexpr int kKnnCtlWords = 16;
constexpr int kKnnLdsBudget = 81920;         // half of the CU's 160 KiB: two workgroups per CU
constexpr uint32_t kNone = 0xFFFFFFFFu;

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// fp32 -> 64-bit fixed point (two's complement), scale 2^36, truncated toward zero: ccd_scatter.hip's to_fixed.  |x| < 64.
__device__ __forceinline__ unsigned long long to_fixed(float x) {
    return (unsigned long long) (long long) ((double) x * 68719476736.0);
}

// The fp32 of an integer sum: one rounding int64 -> fp32, then the exact 2^-36 (KeyOfSum: the key of knn_row's scan).
__device__ __forceinline__ float from_fixed(unsigned long long v) {
    return mul_rn((float) (long long) v, 1.4551915228366852e-11f);
}

// The candidate area of a selection: 2048 slots above keep = 512, else 1024; the first `keep` are the running list.
inline int knn_area(int keep) { return keep > 512 ? 2048 : 1024; }
// The widest accumulator tile that leaves two workgroups per CU (a multiple of 64, at most 8192 = 64 KiB).
inline int knn_tile_max(int keep) { return std::min(8192, (kKnnLdsBudget - 4 * kKnnCtlWords - 8 * knn_area(keep)) / 8 / 64 * 64); }
inline size_t knn_lds_bytes(int T, int keep) { return (size_t) T * 8 + (size_t) knn_area(keep) * 8 + 4 * kKnnCtlWords; }

struct KnnLds {
    unsigned long long* acc;  // [T]
    float* key;               // [NC]
    uint32_t* id;             // [NC]
    uint32_t* ctl;            // [0] candidates in the area, [1] threshold item, [2] threshold key (bits), [3] bad flag, [4] queue slot
    int NC;
};

__device__ inline KnnLds knn_lds(unsigned char* raw, int T, int NC) {
    KnnLds s;
    s.acc = reinterpret_cast<unsigned long long*>(raw);
    s.key = reinterpret_cast<float*>(raw + (size_t) T * 8);
    s.id = reinterpret_cast<uint32_t*>(s.key + NC);
    s.ctl = s.id + NC;
    s.NC = NC;
    return s;
}

// Sorts the area's candidates by beats() and keeps the first `keep`; returns their number.  Called by every thread after
// a barrier; no thread adds a candidate between that barrier and the one inside, so ctl[0] is the same for all.
__device__ int knn_sort_keep(const KnnLds& s, int keep) {
    const int tid = threadIdx.x;
    const int cnt = min((int) s.ctl[0], s.NC);
    int n = 1;
    while (n < cnt) n <<= 1;
    for (int t = cnt + tid; t < n; t += kKnnThreads) {
        s.key[t] = -INFINITY;
        s.id[t] = kPad;
    }
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += kKnnThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const float ka = s.key[lo], kb = s.key[hi];
                const uint32_t ia = s.id[lo], ib = s.id[hi];
                const bool first_half = (lo & k) == 0;  // the better entry goes to the lower slot here, to the upper otherwise
                if (first_half ? beats(kb, ib, ka, ia) : beats(ka, ia, kb, ib)) {
                    s.key[lo] = kb; s.id[lo] = ib;
                    s.key[hi] = ka; s.id[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    const int kept = min(cnt, keep);
    if (tid == 0) {
        s.ctl[0] = (uint32_t) kept;
        const bool full = kept == keep;
        s.ctl[1] = full ? s.id[keep - 1] : kPad;
        s.ctl[2] = __float_as_uint(full ? s.key[keep - 1] : -INFINITY);
    }
    __syncthreads();
    return kept;
}

// The start of a row's selection: an empty list, no threshold, no bad term.
__device__ inline void knn_begin(const KnnLds& s) {
    if (threadIdx.x == 0) {
        s.ctl[0] = 0;
        s.ctl[1] = kPad;
        s.ctl[2] = __float_as_uint(-INFINITY);
        s.ctl[3] = 0;
    }
    __syncthreads();
}

// How a slot's 64 bits become a key.  KeyOfSum: the slot is an integer sum on the 2^-36 grid.  KeyOfBits: scores that are not
// sums on the grid (ease.hip) -- a slot holds kKnnLive | the bits of its fp32 key, or 0 when it is not eligible (an item of
// the row, a NaN score) or already taken, so that zero and negative keys are candidates too.
constexpr unsigned long long kKnnLive = 1ull << 32;
struct KeyOfSum {
    __device__ float operator()(unsigned long long v) const { return from_fixed(v); }
};
struct KeyOfBits {
    __device__ float operator()(unsigned long long v) const { return __uint_as_float((uint32_t) v); }
};

// Scan and select over one tile, without a barrier before the end of a pass.  A candidate that finds the area full stays in
// its slot; then list and area are merged, which raises the threshold, and the tile is scanned again for what is left.
// Every pass places at least NC - keep candidates or ends the tile.  The tile is all zeros on return.
template <class Key>
__device__ void knn_scan(const KnnLds& s, uint32_t base, uint32_t len, int keep, Key key_of) {
    const int tid = threadIdx.x;
    for (;;) {
        const float thr_key = __uint_as_float(s.ctl[2]);
        const uint32_t thr_id = s.ctl[1];
        for (uint32_t slot = tid; slot < len; slot += kKnnThreads) {
            const unsigned long long v = s.acc[slot];
            if (v == 0ull) continue;
            const float key = key_of(v);
            const uint32_t item = base + slot;
            if (beats(key, item, thr_key, thr_id)) {
                const uint32_t pos = atomicAdd(&s.ctl[0], 1u);
                if (pos >= (uint32_t) s.NC) continue;
                s.key[pos] = key;
                s.id[pos] = item;
            }
            s.acc[slot] = 0ull;
        }
        __syncthreads();
        if (s.ctl[0] <= (uint32_t) s.NC) break;  // (nobody touches ctl[0] again before the next barrier)
        knn_sort_keep(s, keep);
    }
}

// One output row: the tiles of the item axis, the terms of `src`, the best `keep` candidates.  On return key / id [0 .. count)
// hold them in order and ctl[3] says whether a thread met a bad term.  The accumulators are all zero on entry and on return.
template <class Src>
__device__ int knn_row(const KnnLds& s, const Src& src, uint32_t cols, uint32_t T, int keep) {
    knn_begin(s);
    bool bad = false;
    for (uint32_t base = 0; base < cols; base += min(T, cols - base)) {
        const uint32_t len = min(T, cols - base);
        bad |= src.add_terms(s.acc, base, len);
        __syncthreads();
        if (src.drop_seen(s.acc, base, len)) __syncthreads();
        knn_scan(s, base, len, keep, KeyOfSum());
    }
    if (bad) s.ctl[3] = 1;
    return knn_sort_keep(s, keep);  // (its barriers publish ctl[3])
}

// The items of a query row are no candidates: their slots of the tile are cleared.
__device__ inline void knn_drop_seen(unsigned long long* acc, const uint32_t* idx, uint32_t n, uint32_t base, uint32_t len) {
    for (uint32_t e = threadIdx.x; e < n; e += kKnnThreads) {
        const uint32_t off = idx[e] - base;
        if (off < len) acc[off] = 0ull;
    }
}

// ---------------------------------------------------------------------------------------------- the build's term source
// The row of X^T X of item i.  For every user u of column i (value x) and every entry (j, y) of row u with j != i the term
// fp32(x * y) goes to accumulator j.
struct BuildSrc {
    const uint32_t* ptr;   // CSR
    const uint32_t* idx;
    const float* val;
    const uint32_t* ridx;  // CSC of the same matrix
    const float* cval;
    uint32_t c0, c1, item;

    __device__ bool add_terms(unsigned long long* acc, uint32_t base, uint32_t len) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        bool bad = false;
        for (uint64_t e0 = (uint64_t) c0 + 64u * wave; e0 < c1; e0 += 64u * kKnnWaves) {
            const uint64_t e = e0 + lane;
            uint32_t a = 0, b = 0;
            float x = 0.f;
            if (e < c1) {
                const uint32_t u = ridx[e];
                x = cval[e];
                a = ptr[u];
                b = ptr[u + 1];
                if (base > 0) {  // the first entry of the sorted row at or after the tile's start
                    uint32_t hi = b;
                    while (a < hi) {
                        const uint32_t mid = a + (hi - a) / 2;
                        if (idx[mid] < base) a = mid + 1;
                        else hi = mid;
                    }
                }
            }
            const int nb = (int) min((uint64_t) 64, (uint64_t) c1 - e0);
            for (int l = 0; l < nb; ++l) {
                const uint32_t ra = __shfl(a, l), rb = __shfl(b, l);
                const float rx = __shfl(x, l);
                // 64 * kKnnBatch entries of the row per round, their loads in flight together (wave-uniform loop)
                for (uint64_t r0 = ra; r0 < rb; r0 += 64 * kKnnBatch) {
                    uint32_t j[kKnnBatch];
                    float y[kKnnBatch];
#pragma unroll
                    for (int b = 0; b < kKnnBatch; ++b) {
                        const uint64_t p = r0 + 64u * b + lane;
                        j[b] = kNone;
                        y[b] = 0.f;
                        if (p < rb) {
                            j[b] = idx[p];
                            y[b] = val[p];
                        }
                    }
                    if (__builtin_amdgcn_readfirstlane(j[0]) - base >= len) break;  // (sorted: the rest of the row lies beyond the tile)
#pragma unroll
                    for (int b = 0; b < kKnnBatch; ++b) {
                        const uint32_t off = j[b] - base;  // (kNone - base >= len: base + len <= cols < 2^32 - 1)
                        if (off >= len || j[b] == item) continue;
                        const float t = mul_rn(rx, y[b]);
                        if (!(__builtin_fabsf(t) < 64.f)) bad = true;  // (NaN compares false)
                        else atomicAdd(&acc[off], to_fixed(t));
                    }
                }
            }
        }
        return bad;
    }
    __device__ bool drop_seen(unsigned long long*, uint32_t, uint32_t) const { return false; }
};

__device__ inline void knn_zero_tile(const KnnLds& s, uint32_t T) {
    for (uint32_t t = threadIdx.x; t < T; t += kKnnThreads) s.acc[t] = 0ull;
    __syncthreads();
}

// The list of a finished row: the first `count` slots of the area, pads behind them (all pads when !ok).
__device__ inline void knn_store(const KnnLds& s, int count, int width, bool ok, uint32_t* out_id, float* out_key) {
    for (int q = threadIdx.x; q < width; q += kKnnThreads) {
        const bool real = ok && q < count;
        out_id[q] = real ? s.id[q] : kPad;
        if (out_key) out_key[q] = real ? s.key[q] : -INFINITY;
    }
}

// ---------------------------------------------------------------------------------------------- the build kernels' queue
// What k_knn_build, k_slim_gram and k_ease_gram take alike: the matrix in both orientations and the work queue.
struct BuildArgs {
    const uint32_t* ptr;
    const uint32_t* idx;
    const float* val;
    const uint32_t* cptr;
    const uint32_t* ridx;
    const float* cval;
    const uint32_t* order;  // [cols] the items, heaviest first
    uint32_t* queue;        // the next position of `order`
    uint32_t* first_bad;    // the smallest item with a bad term
    uint32_t cols, T;
};

// The workgroup's loop over the queue: zero the tile, then item by item -- the next position of `order` through ctl[4] --
// row(src) with the term source of the item.  row leaves the tile zero and returns whether this thread names the item for
// a bad term.
template <class Row>
__device__ void knn_build_items(const KnnLds& s, const BuildArgs& a, Row row) {
    knn_zero_tile(s, a.T);
    for (;;) {
        if (threadIdx.x == 0) s.ctl[4] = atomicAdd(a.queue, 1u);
        __syncthreads();
        const uint32_t pos = s.ctl[4];
        if (pos >= a.cols) break;
        const uint32_t i = a.order[pos];
        const BuildSrc src{a.ptr, a.idx, a.val, a.ridx, a.cval, a.cptr[i], a.cptr[i + 1], i};
        if (row(src)) atomicMin(a.first_bad, i);
    }
}

// The tiles of one item's row of X^T X for a kernel that does not select: add the terms, then tile(base, len) reads the
// sums and clears them (the barrier between the two is here, the one after the clearing too).  Returns the thread's bad flag.
template <class Tile>
__device__ bool knn_build_tiles(const KnnLds& s, const BuildSrc& src, uint32_t cols, uint32_t T, Tile tile) {
    bool bad = false;
    for (uint32_t base = 0; base < cols; base += min(T, cols - base)) {
        const uint32_t len = min(T, cols - base);
        bad |= src.add_terms(s.acc, base, len);
        __syncthreads();
        tile(base, len);
        __syncthreads();
    }
    return bad;
}

// The diagonal of X^T X, a wave per item (blocks of 256 threads): done(i, d_i) on lane 0 with d_i the fp32 of the integer sum
// of fp32(x * x) over column i; a bad term names the item.  The body of k_slim_diag and k_ease_diag.
template <class Done>
__device__ void knn_diag(const uint32_t* __restrict__ cptr, const float* __restrict__ cval, uint32_t cols, uint32_t* first_bad, Done done) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t) gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = (uint64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < cols; i += nw) {
        const uint32_t c0 = cptr[i], c1 = cptr[i + 1];
        unsigned long long sum = 0;
        bool bad = false;
        for (uint64_t e = (uint64_t) c0 + lane; e < c1; e += 64) {
            const float x = cval[e];
            const float t = mul_rn(x, x);
            if (!(t < 64.f)) bad = true;  // (NaN compares false)
            else sum += to_fixed(t);
        }
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (bad) atomicMin(first_bad, (uint32_t) i);
        if (lane == 0) done(i, from_fixed(sum));
    }
}

// ---------------------------------------------------------------------------------------------- the recommend kernels' rows
// What the three recommend kernels take alike: the query rows and the outputs.
struct RowsArgs {
    const uint32_t* ptr;   // [nusers + 1]
    const uint32_t* idx;
    const float* val;
    uint32_t* items;       // [nusers][n_top]
    float* scores;         // or NULL
    unsigned long long* bad_rows;
    uint32_t nusers, cols, T;
    int n_top, NC;
    bool keep_seen;
};

// The query row of a term source: its entries, and their slots cleared after the terms unless keep_seen.
struct RowSrc {
    const uint32_t* idx;
    const float* val;
    uint32_t n;
    bool keep_seen;
    __device__ bool drop_seen(unsigned long long* acc, uint32_t base, uint32_t len) const {
        if (keep_seen) return false;
        knn_drop_seen(acc, idx, n, base, len);
        return true;
    }
};

// A workgroup per query row: knn_row over the model's term source, Args::source(row).  A row of more than 2^21 entries or
// with a bad term is all pads and counted in bad_rows.
template <class Args>
__global__ __launch_bounds__(kKnnThreads) void k_knn_rows(Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_raw[];
    const KnnLds s = knn_lds(knn_raw, (int) a.T, a.NC);
    knn_zero_tile(s, a.T);
    for (uint32_t r = blockIdx.x; r < a.nusers; r += gridDim.x) {
        const uint32_t r0 = a.ptr[r], n = a.ptr[r + 1] - r0;
        const bool too_long = n > kKnnMaxEntries;
        const auto src = a.source(RowSrc{a.idx + r0, a.val + r0, too_long ? 0u : n, a.keep_seen});
        const int count = knn_row(s, src, a.cols, a.T, a.n_top);
        const bool ok = !too_long && !s.ctl[3];
        knn_store(s, count, a.n_top, ok, a.items + (size_t) r * a.n_top, a.scores ? a.scores + (size_t) r * a.n_top : nullptr);
        if (threadIdx.x == 0 && !ok) atomicAdd(a.bad_rows, 1ull);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- the kernels of the checks
// Segment r of a compressed matrix: its pointers inside [0, nnz] and in order, its ids strictly ascending and below `bound`.
__global__ void k_knn_check(const uint32_t* ptr, const uint32_t* idx, uint32_t nseg, uint32_t bound, uint32_t nnz, uint32_t* first_bad) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < nseg; r += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t lo = ptr[r], hi = ptr[r + 1];
        bool bad = lo > hi || hi > nnz || (r == 0 && lo != 0) || (r + 1 == nseg && hi != nnz);
        if (!bad) {
            uint32_t prev = 0;
            for (uint32_t e = lo; e < hi; ++e) {
                const uint32_t c = idx[e];
                if (c >= bound || (e > lo && c <= prev)) { bad = true; break; }
                prev = c;
            }
        }
        if (bad) atomicMin(first_bad, (uint32_t) r);
    }
}

// The work of item i, a wave per item: the sum over the users of column i of their rows' lengths; a column of more than
// 2^21 entries is named in first_long.
__global__ __launch_bounds__(256) void k_knn_work(const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ cptr,
                                                  const uint32_t* __restrict__ ridx, uint32_t cols, unsigned long long* __restrict__ work,
                                                  uint32_t* first_long) {
    const int lane = threadIdx.x & 63;
    const uint64_t nw = (uint64_t) gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = (uint64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < cols; i += nw) {
        const uint32_t c0 = cptr[i], c1 = cptr[i + 1];
        unsigned long long w = 0;
        for (uint64_t e = (uint64_t) c0 + lane; e < c1; e += 64) {
            const uint32_t u = ridx[e];
            w += ptr[u + 1] - ptr[u];
        }
        for (int off = 32; off > 0; off >>= 1) w += __shfl_xor(w, off);
        if (lane == 0) {
            work[i] = w;
            if (c1 - c0 > kKnnMaxEntries) atomicMin(first_long, (uint32_t) i);
        }
    }
}

// ---------------------------------------------------------------------------------------------- host helpers
int check_space(const char* fn, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    return MFX_OK;
}

// tile_items as given (0: automatic) -> the accumulator tile of a selection of `keep` over `cols` items.
int pick_tile(const char* fn, int32_t tile_items, int64_t cols, int keep, uint32_t* T) {
    const int tmax = knn_tile_max(keep);
    MFX_REQUIRE(tile_items >= 0 && tile_items % 64 == 0 && tile_items <= tmax,
                "%s: tile_items must be 0 or a multiple of 64 up to %d (got %d)", fn, tmax, tile_items);
    *T = tile_items > 0 ? (uint32_t) tile_items : (uint32_t) std::min<int64_t>((cols + 63) / 64 * 64, tmax);
    return MFX_OK;
}

// An input array on the device: the caller's own (MFX_DEVICE) or a copy of the host's.
template <typename T>
struct Staged {
    DevBuf<T> own;
    const T* p = nullptr;
    int set(const T* src, size_t n, mfx_memspace space, hipStream_t st) {
        if (space == MFX_DEVICE || n == 0) {
            p = src;
            return MFX_OK;
        }
        MFX_TRY(own.alloc(n));
        MFX_TRY(own.upload(src, n, space, st));
        p = own.get();
        return MFX_OK;
    }
};

// An allocation whose failure names what it was for.
template <typename T>
int alloc_named(const char* fn, const char* what, DevBuf<T>* buf, size_t count) {
    if (buf->alloc(count) != MFX_OK) return fail(MFX_ERR_ALLOC, "%s: %s, %zu bytes, could not be allocated", fn, what, count * sizeof(T));
    return MFX_OK;
}

// An output array on the device: the caller's own (MFX_DEVICE, or NULL for an output that is not asked for), or a device
// buffer that copy_out copies to the host's at the end of the call.  `what` names the buffer in its allocation failure.
template <typename T>
struct Out {
    DevBuf<T> own;
    T* p = nullptr;
    int set(T* out, size_t count, mfx_memspace space, const char* fn = nullptr, const char* what = nullptr) {
        p = out;
        if (space == MFX_HOST && out) {
            MFX_TRY(what ? alloc_named(fn, what, &own, count) : own.alloc(count));
            p = own.get();
        }
        return MFX_OK;
    }
    int copy_out(T* out, size_t count, mfx_memspace space, hipStream_t st) {  // (asynchronous)
        if (space == MFX_HOST && out) MFX_HIP(hipMemcpyAsync(out, p, sizeof(T) * count, hipMemcpyDeviceToHost, st));
        return MFX_OK;
    }
};

// One word on the device that kernels lower with atomicMin: kNone while nothing was found.
struct FirstBad {
    DevBuf<uint32_t> w;
    int init(hipStream_t st) {
        MFX_TRY(w.alloc(1));
        MFX_HIP(hipMemsetAsync(w.get(), 0xFF, sizeof(uint32_t), st));
        return MFX_OK;
    }
    int read(hipStream_t st, uint32_t* out) {  // synchronises
        MFX_HIP(hipMemcpyAsync(out, w.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        return MFX_OK;
    }
};

inline uint32_t grid_256(uint64_t n) { return (uint32_t) std::min<uint64_t>((n + 255) / 256, 65536); }

template <class Kern>
int allow_lds(Kern kern, size_t bytes) {
    if (bytes > 65536) MFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes));
    return MFX_OK;
}

double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// ---------------------------------------------------------------------------------------------- the matrix of the three builds
int check_x(const char* fn, const mfx_csx* X) {
    MFX_REQUIRE(X->nnz >= 1, "%s: the matrix has no entries", fn);
    MFX_REQUIRE(X->cols >= 2, "%s: cols must be at least 2 (got %lld)", fn, (long long) X->cols);
    MFX_REQUIRE(X->rows >= 1 && X->rows < 0xFFFFFFFFll && X->cols < 0xFFFFFFFFll && X->nnz < 0xFFFFFFFFll,
                "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    MFX_REQUIRE(X->csr_row_ptr && X->csr_col_idx && X->csr_val && X->csc_col_ptr && X->csc_row_idx && X->csc_val,
                "%s: X needs both orientations (a null array)", fn);
    return MFX_OK;
}

struct StagedX {
    Staged<uint32_t> ptr, idx, cptr, ridx;
    Staged<float> val, cval;
    uint32_t rows = 0, cols = 0, nnz = 0;

    // The six arrays on the device, their structure checked: the row side first, then the column side.
    int set(const char* fn, const mfx_csx* X, mfx_memspace space, hipStream_t st) {
        rows = (uint32_t) X->rows; cols = (uint32_t) X->cols; nnz = (uint32_t) X->nnz;
        MFX_TRY(ptr.set(X->csr_row_ptr, (size_t) rows + 1, space, st));
        MFX_TRY(idx.set(X->csr_col_idx, nnz, space, st));
        MFX_TRY(val.set(X->csr_val, nnz, space, st));
        MFX_TRY(cptr.set(X->csc_col_ptr, (size_t) cols + 1, space, st));
        MFX_TRY(ridx.set(X->csc_row_idx, nnz, space, st));
        MFX_TRY(cval.set(X->csc_val, nnz, space, st));
        FirstBad bad_row, bad_col;
        MFX_TRY(bad_row.init(st));
        MFX_TRY(bad_col.init(st));
        hipLaunchKernelGGL(k_knn_check, dim3(grid_256(rows)), dim3(256), 0, st, ptr.p, idx.p, rows, cols, nnz, bad_row.w.get());
        MFX_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_knn_check, dim3(grid_256(cols)), dim3(256), 0, st, cptr.p, ridx.p, cols, rows, nnz, bad_col.w.get());
        MFX_LAUNCH_CHECK();
        uint32_t first = kNone;
        MFX_TRY(bad_row.read(st, &first));
        MFX_REQUIRE(first == kNone, "%s: row %u of the CSR side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols",
                    fn, first);
        MFX_TRY(bad_col.read(st, &first));
        MFX_REQUIRE(first == kNone,
                    "%s: column %u of the CSC side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below rows", fn, first);
        return MFX_OK;
    }
};

// The work order of the queue (heaviest item first, ties by item), on the device.  Refuses an over-long column.
int work_order(const char* fn, const StagedX& x, hipStream_t st, DevBuf<uint32_t>* order) {
    const uint32_t cols = x.cols;
    FirstBad long_col;
    MFX_TRY(long_col.init(st));
    DevBuf<unsigned long long> work;
    MFX_TRY(work.alloc(cols));
    hipLaunchKernelGGL(k_knn_work, dim3(grid_256((uint64_t) cols * 64)), dim3(256), 0, st, x.ptr.p, x.cptr.p, x.ridx.p, cols, work.get(),
                       long_col.w.get());
    MFX_LAUNCH_CHECK();
    std::vector<unsigned long long> hwork(cols);
    MFX_HIP(hipMemcpyAsync(hwork.data(), work.get(), sizeof(unsigned long long) * cols, hipMemcpyDeviceToHost, st));
    uint32_t first = kNone;
    MFX_TRY(long_col.read(st, &first));
    MFX_REQUIRE(first == kNone, "%s: item %u: a column of more than 2^21 entries", fn, first);
    std::vector<uint32_t> horder(cols);
    std::iota(horder.begin(), horder.end(), 0u);
    std::sort(horder.begin(), horder.end(), [&](uint32_t a, uint32_t b) { return hwork[a] > hwork[b] || (hwork[a] == hwork[b] && a < b); });
    MFX_TRY(order->alloc(cols));
    MFX_TRY(order->upload(horder.data(), cols, MFX_HOST, st));
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int device_cus(int device, int* cus) {
    MFX_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
    *cus = std::max(*cus, 1);
    return MFX_OK;
}

// The launch of a build kernel (k_knn_build, k_slim_gram, k_ease_gram): begin() makes the word that names a bad term and
// the zeroed queue word, fill() the shared fields of the kernel's arguments, run() launches min(cols, 2 * cus) workgroups
// and reports the term.  Between begin() and run() the caller launches what shares the word (the diagonal kernels).
struct BuildPass {
    FirstBad bad_term;
    DevBuf<uint32_t> queue;
    int begin(hipStream_t st) {
        MFX_TRY(bad_term.init(st));
        MFX_TRY(queue.alloc_zero(1, st));
        return MFX_OK;
    }
    void fill(BuildArgs* a, const StagedX& x, const DevBuf<uint32_t>& order, uint32_t T) const {
        a->ptr = x.ptr.p; a->idx = x.idx.p; a->val = x.val.p;
        a->cptr = x.cptr.p; a->ridx = x.ridx.p; a->cval = x.cval.p;
        a->order = order.get(); a->queue = queue.get(); a->first_bad = bad_term.w.get();
        a->cols = x.cols; a->T = T;
    }
    template <class Args>
    int run(void (*kern)(Args), const char* fn, const Args& a, size_t lds, int cus, hipStream_t st) {  // synchronises
        MFX_TRY(allow_lds(kern, lds));
        const uint32_t grid = (uint32_t) std::min<uint64_t>(a.cols, (uint64_t) cus * 2);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kKnnThreads), lds, st, a);
        MFX_LAUNCH_CHECK();
        uint32_t first = kNone;
        MFX_TRY(bad_term.read(st, &first));
        MFX_REQUIRE(first == kNone, "%s: item %u: a term x_ui * x_uj that is not finite or of magnitude >= 64", fn, first);
        return MFX_OK;
    }
};
// The LDS of a build kernel that does not select: the tile and ctl.
inline size_t knn_tile_bytes(uint32_t T) { return (size_t) T * 8 + 4 * kKnnCtlWords; }

// ---------------------------------------------------------------------------------------------- the host side of recommend
// The arguments of mfx_knn_recommend, mfx_slim_recommend and mfx_ease_recommend behind the handle.
struct RowsQuery {
    int64_t nusers, nnz;
    const uint32_t* ptr;
    const uint32_t* idx;
    const float* val;
    int32_t n_top;
    int flags;
    int32_t tile_items;
    uint32_t* items;
    float* scores;
    int64_t* bad_rows;
    mfx_memspace space;
};

// One recommend call of a model of `cols` items: the checks of the arguments, the rows on the device and their structure
// check (its time goes to *t_check), `kern` with min(nusers, 8 * cus) workgroups (*t_pass), the results.  Args derives from
// RowsArgs; fill(&args) sets the model's own fields.  One synchronisation at the end, after everything is queued.
template <class Args, class Fill>
int rows_recommend(void (*kern)(Args), const char* fn, int64_t cols, int cus, int device, hipStream_t st, double* t_check, double* t_pass,
                   const RowsQuery& q, Fill fill) {
    MFX_TRY(check_space(fn, q.space));
    MFX_REQUIRE(q.n_top >= 1 && q.n_top <= 1024, "%s: n_top must be in [1, 1024] (got %d)", fn, q.n_top);
    MFX_REQUIRE((q.flags & ~MFX_KNN_KEEP_SEEN) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) q.flags);
    MFX_REQUIRE(q.nusers >= 0 && q.nusers < 0xFFFFFFFFll && q.nnz >= 0 && q.nnz < 0xFFFFFFFFll, "%s: nusers and nnz must be in [0, 2^32 - 1)", fn);
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, q.tile_items, cols, q.n_top, &T));
    if (q.bad_rows) *q.bad_rows = 0;
    if (q.nusers == 0) return MFX_OK;
    MFX_REQUIRE(q.ptr && q.items, "%s: ptr or items is NULL", fn);
    MFX_REQUIRE(q.nnz == 0 || (q.idx && q.val), "%s: idx or val is NULL", fn);
    MFX_TRY(use_device(device));
    hipEvent_t ev[3] = {};
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 3; ++i)
                if (e[i]) (void) hipEventDestroy(e[i]);
        }
    } guard{ev};
    for (auto& e : ev) MFX_HIP(hipEventCreate(&e));
    Staged<uint32_t> sp, si;
    Staged<float> sv;
    MFX_TRY(sp.set(q.ptr, (size_t) q.nusers + 1, q.space, st));
    MFX_TRY(si.set(q.idx, (size_t) q.nnz, q.space, st));
    MFX_TRY(sv.set(q.val, (size_t) q.nnz, q.space, st));
    const size_t total = (size_t) q.nusers * q.n_top;
    Out<uint32_t> oi;
    Out<float> os;
    MFX_TRY(oi.set(q.items, total, q.space));
    MFX_TRY(os.set(q.scores, total, q.space));
    DevBuf<unsigned long long> nbad;
    MFX_TRY(nbad.alloc_zero(1, st));
    FirstBad bad;
    MFX_TRY(bad.init(st));
    MFX_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_knn_check, dim3(grid_256((uint64_t) q.nusers)), dim3(256), 0, st, sp.p, si.p, (uint32_t) q.nusers, (uint32_t) cols,
                       (uint32_t) q.nnz, bad.w.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev[1], st));
    uint32_t first = kNone;
    MFX_TRY(bad.read(st, &first));
    MFX_REQUIRE(first == kNone, "%s: row %u: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols", fn, first);

    Args a{};
    a.ptr = sp.p; a.idx = si.p; a.val = sv.p;
    a.items = oi.p; a.scores = os.p; a.bad_rows = nbad.get();
    a.nusers = (uint32_t) q.nusers; a.cols = (uint32_t) cols; a.T = T;
    a.n_top = q.n_top; a.NC = knn_area(q.n_top);
    a.keep_seen = (q.flags & MFX_KNN_KEEP_SEEN) != 0;
    fill(&a);
    const size_t lds = knn_lds_bytes((int) T, q.n_top);
    MFX_TRY(allow_lds(kern, lds));
    const uint32_t grid = (uint32_t) std::min<uint64_t>((uint64_t) q.nusers, (uint64_t) cus * 8);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kKnnThreads), lds, st, a);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev[2], st));
    unsigned long long hbad = 0;
    MFX_HIP(hipMemcpyAsync(&hbad, nbad.get(), sizeof(hbad), hipMemcpyDeviceToHost, st));
    MFX_TRY(oi.copy_out(q.items, total, q.space, st));
    MFX_TRY(os.copy_out(q.scores, total, q.space, st));
    MFX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    MFX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *t_check += 1e-3 * ms;
    MFX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    *t_pass += 1e-3 * ms;
    if (q.bad_rows) *q.bad_rows = (int64_t) hbad;
    return MFX_OK;
}

}  // namespace

}  // namespace mfx
