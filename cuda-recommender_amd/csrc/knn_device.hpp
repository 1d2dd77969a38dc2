// knn_device.hpp -- the device skeleton and the host helpers that the units on the interaction matrix share: knn.hip
// (mfx_knn_*), slim.hip (mfx_slim_*) and ease.hip (mfx_ease_*).  Everything here sits in an anonymous namespace: each unit
// compiles its own copy, as knn.hip did while this text was part of it.
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
// knn_row is scan and select over a term source; slim.hip's Gram pass keeps `add` and gathers from the tile instead, ease.hip's
// writes the tile out densely; ease.hip's recommendation fills the tile with fp32 scores and selects with knn_dense_scan.
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

// The fp32 of an integer sum: one rounding int64 -> fp32, then the exact 2^-36 (what knn_row's scan does in line).
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

// One output row: the tiles of the item axis, the terms of `src`, the best `keep` candidates.  On return key / id [0 .. count)
// hold them in order and ctl[3] says whether a thread met a bad term.  The accumulators are all zero on entry and on return.
template <class Src>
__device__ int knn_row(const KnnLds& s, const Src& src, uint32_t cols, uint32_t T, int keep) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        s.ctl[0] = 0;
        s.ctl[1] = kPad;
        s.ctl[2] = __float_as_uint(-INFINITY);
        s.ctl[3] = 0;
    }
    __syncthreads();
    bool bad = false;
    for (uint32_t base = 0; base < cols; base += min(T, cols - base)) {
        const uint32_t len = min(T, cols - base);
        bad |= src.add_terms(s.acc, base, len);
        __syncthreads();
        if (src.drop_seen(s.acc, base, len)) __syncthreads();
        // The scan runs over the whole tile without a barrier.  A candidate that finds the area full stays in its
        // accumulator; then list and area are merged, which raises the threshold, and the tile is scanned again for what
        // is left.  Every pass places at least NC - keep candidates or ends the tile.
        for (;;) {
            const float thr_key = __uint_as_float(s.ctl[2]);
            const uint32_t thr_id = s.ctl[1];
            for (uint32_t slot = tid; slot < len; slot += kKnnThreads) {
                const unsigned long long v = s.acc[slot];
                if (v == 0ull) continue;
                const float key = mul_rn((float) (long long) v, 1.4551915228366852e-11f);  // one rounding int64 -> fp32, then the exact 2^-36
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
    if (bad) s.ctl[3] = 1;
    return knn_sort_keep(s, keep);  // (its barriers publish ctl[3])
}

// The sibling of knn_row's scan for scores that are not sums on the grid (ease.hip): every ELIGIBLE slot of the tile is a
// candidate, zero and negative keys included.  A slot holds kKnnLive | the bits of its fp32 key, or 0 when it is not eligible
// (an item of the row, a NaN score) or already taken.  Same threshold, area and merge as above; the tile is all zeros on
// return.  knn_dense_begin resets the selection at the start of a row; the caller ends the row with knn_sort_keep.
constexpr unsigned long long kKnnLive = 1ull << 32;

__device__ inline void knn_dense_begin(const KnnLds& s) {
    if (threadIdx.x == 0) {
        s.ctl[0] = 0;
        s.ctl[1] = kPad;
        s.ctl[2] = __float_as_uint(-INFINITY);
        s.ctl[3] = 0;
    }
    __syncthreads();
}

__device__ inline void knn_dense_scan(const KnnLds& s, uint32_t base, uint32_t len, int keep) {
    const int tid = threadIdx.x;
    for (;;) {
        const float thr_key = __uint_as_float(s.ctl[2]);
        const uint32_t thr_id = s.ctl[1];
        for (uint32_t slot = tid; slot < len; slot += kKnnThreads) {
            const unsigned long long v = s.acc[slot];
            if (v == 0ull) continue;
            const float key = __uint_as_float((uint32_t) v);
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

// ---------------------------------------------------------------------------------------------- the matrix of slim.hip and ease.hip
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

    // The six arrays on the device, their structure checked as by mfx_knn_build.
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

}  // namespace

}  // namespace mfx
