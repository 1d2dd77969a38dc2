// knn.hip -- item-kNN on the interaction matrix (mfx_knn_*) on gfx950: the sparse X^T X with a top-K per row, and the
// recommendation from the stored lists.  The contract -- the fp32 term, the 2^-36 fixed-point integer sums, the order and the
// limits -- is in include/mfx.h; DESIGN 5.16 has the sizing.
//
// Build and recommend share the device skeleton of knn_device.hpp, knn_row (add, scan, select over a term source), which
// slim.hip uses too.  The term sources: k_knn_build's BuildSrc (knn_device.hpp) takes the users of column i in batches of 64
// per wave (coalesced loads of the column, one lane per user for the row pointers and the lower-bound search of the tile's
// start in the sorted row), then runs the lanes across each row; k_knn_recommend's RecSrc runs the threads across the
// n_u * K (entry, slot) pairs of the query row.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <numeric>

#include "knn.hpp"
#include "knn_device.hpp"

namespace mfx {

namespace {

// Recommend: the scores of one query row.  For every entry (i, x) of the row and every stored slot (j, s) of i the term
// fp32(x * s) goes to accumulator j; with several tiles the pairs are walked once per tile.
struct RecSrc {
    const uint32_t* idx;   // the row's entries
    const float* val;
    uint32_t n;
    const uint32_t* nidx;  // [cols][K]
    const float* nsim;
    uint32_t K;
    bool keep_seen;

    __device__ bool add_terms(unsigned long long* acc, uint32_t base, uint32_t len) const {
        bool bad = false;
        const uint32_t npairs = n * K;  // (n <= 2^21, K <= 2^10)
        // four pairs per thread and round: their loads (entry -> slot id and similarity) are in flight together
        for (uint64_t p0 = threadIdx.x; p0 < npairs; p0 += kKnnBatch * kKnnThreads) {
            uint32_t j[kKnnBatch];
            float t[kKnnBatch];
#pragma unroll
            for (int b = 0; b < kKnnBatch; ++b) {
                const uint64_t p = p0 + (uint64_t) b * kKnnThreads;
                j[b] = kPad;
                t[b] = 0.f;
                if (p < npairs) {
                    const uint32_t e = (uint32_t) p / K, q = (uint32_t) p - e * K;
                    const size_t at = (size_t) idx[e] * K + q;
                    j[b] = nidx[at];
                    t[b] = mul_rn(val[e], nsim[at]);
                }
            }
#pragma unroll
            for (int b = 0; b < kKnnBatch; ++b) {
                const uint32_t off = j[b] - base;
                if (j[b] == kPad || off >= len) continue;
                if (!(__builtin_fabsf(t[b]) < 64.f)) bad = true;
                else atomicAdd(&acc[off], to_fixed(t[b]));
            }
        }
        return bad;
    }
    __device__ bool drop_seen(unsigned long long* acc, uint32_t base, uint32_t len) const {
        if (keep_seen) return false;
        for (uint32_t e = threadIdx.x; e < n; e += kKnnThreads) {
            const uint32_t off = idx[e] - base;
            if (off < len) acc[off] = 0ull;
        }
        return true;
    }
};

// ---------------------------------------------------------------------------------------------- kernels
struct KnnBuildArgs {
    const uint32_t* ptr;
    const uint32_t* idx;
    const float* val;
    const uint32_t* cptr;
    const uint32_t* ridx;
    const float* cval;
    const uint32_t* order;  // [cols] the items, heaviest first
    uint32_t* queue;        // the next position of `order`
    uint32_t* first_bad;    // the smallest item with a bad term
    uint32_t* nidx;         // [cols][K]
    float* nsim;
    uint32_t cols, T;
    int K, NC;
};

__global__ __launch_bounds__(kKnnThreads) void k_knn_build(KnnBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_raw[];
    const KnnLds s = knn_lds(knn_raw, (int) a.T, a.NC);
    knn_zero_tile(s, a.T);
    for (;;) {
        if (threadIdx.x == 0) s.ctl[4] = atomicAdd(a.queue, 1u);
        __syncthreads();
        const uint32_t pos = s.ctl[4];
        if (pos >= a.cols) break;
        const uint32_t i = a.order[pos];
        const BuildSrc src{a.ptr, a.idx, a.val, a.ridx, a.cval, a.cptr[i], a.cptr[i + 1], i};
        const int count = knn_row(s, src, a.cols, a.T, a.K);
        knn_store(s, count, a.K, true, a.nidx + (size_t) i * a.K, a.nsim + (size_t) i * a.K);
        if (threadIdx.x == 0 && s.ctl[3]) atomicMin(a.first_bad, i);
        __syncthreads();  // (the area and ctl are free for the next item)
    }
}

struct KnnRecArgs {
    const uint32_t* ptr;   // [nusers + 1]
    const uint32_t* idx;
    const float* val;
    const uint32_t* nidx;
    const float* nsim;
    uint32_t* items;       // [nusers][n_top]
    float* scores;         // or NULL
    unsigned long long* bad_rows;
    uint32_t nusers, cols, T;
    int K, n_top, NC;
    bool keep_seen;
};

__global__ __launch_bounds__(kKnnThreads) void k_knn_recommend(KnnRecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_raw[];
    const KnnLds s = knn_lds(knn_raw, (int) a.T, a.NC);
    knn_zero_tile(s, a.T);
    for (uint32_t r = blockIdx.x; r < a.nusers; r += gridDim.x) {
        const uint32_t r0 = a.ptr[r], n = a.ptr[r + 1] - r0;
        const bool too_long = n > kKnnMaxEntries;
        const RecSrc src{a.idx + r0, a.val + r0, too_long ? 0u : n, a.nidx, a.nsim, (uint32_t) a.K, a.keep_seen};
        const int count = knn_row(s, src, a.cols, a.T, a.n_top);
        const bool ok = !too_long && !s.ctl[3];
        knn_store(s, count, a.n_top, ok, a.items + (size_t) r * a.n_top, a.scores ? a.scores + (size_t) r * a.n_top : nullptr);
        if (threadIdx.x == 0 && !ok) atomicAdd(a.bad_rows, 1ull);
        __syncthreads();
    }
}

// Item i's list as handed to mfx_knn_create_from_lists: ids below cols or pad, pads at the tail only, finite similarities.
__global__ void k_knn_check_lists(const uint32_t* nidx, const float* nsim, uint32_t cols, int K, uint32_t* first_bad) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < cols; i += (uint64_t) gridDim.x * blockDim.x) {
        bool bad = false, padded = false;
        for (int q = 0; q < K; ++q) {
            const uint32_t j = nidx[i * K + q];
            if (j == kPad) padded = true;
            else if (padded || j >= cols || !(__builtin_fabsf(nsim[i * K + q]) < INFINITY)) { bad = true; break; }
        }
        if (bad) atomicMin(first_bad, (uint32_t) i);
    }
}

// The first n_top stored slots of the queried items (items == NULL: query q is item q).
__global__ void k_knn_neighbours(const uint32_t* nidx, const float* nsim, const uint32_t* items, uint64_t nq, uint32_t cols, int K, int n_top,
                                 uint32_t* out_items, float* out_sims, uint32_t* first_bad) {
    const uint64_t total = nq * (uint64_t) n_top;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t q = t / n_top;
        const int c = (int) (t - q * n_top);
        const uint32_t i = items ? items[q] : (uint32_t) q;
        if (i >= cols) {
            atomicMin(first_bad, (uint32_t) q);  // (nq < 2^32 - 1)
            continue;
        }
        out_items[t] = nidx[(size_t) i * K + c];
        if (out_sims) out_sims[t] = nsim[(size_t) i * K + c];
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------- Knn
int Knn::init(int64_t cols, int32_t K, int device) {
    cols_ = cols; K_ = K; device_ = device;
    MFX_TRY(use_device(device));
    MFX_HIP(hipDeviceGetAttribute(&cus_, hipDeviceAttributeMultiprocessorCount, device));
    cus_ = std::max(cus_, 1);
    MFX_TRY(nidx_.alloc((size_t) cols * K));
    MFX_TRY(nsim_.alloc((size_t) cols * K));
    return MFX_OK;
}

int Knn::build(Knn** out, const mfx_csx* X, int32_t K, int32_t tile_items, mfx_memspace space, int device) {
    const char* fn = "mfx_knn_build";
    MFX_REQUIRE(out && X, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(K >= 1 && K <= 1024, "%s: K must be in [1, 1024] (got %d)", fn, K);
    MFX_REQUIRE(X->nnz >= 1, "%s: the matrix has no entries", fn);
    MFX_REQUIRE(X->cols >= 2, "%s: cols must be at least 2 (got %lld)", fn, (long long) X->cols);
    MFX_REQUIRE(X->rows >= 1 && X->rows < 0xFFFFFFFFll && X->cols < 0xFFFFFFFFll && X->nnz < 0xFFFFFFFFll,
                "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    MFX_REQUIRE(X->csr_row_ptr && X->csr_col_idx && X->csr_val && X->csc_col_ptr && X->csc_row_idx && X->csc_val,
                "%s: X needs both orientations (a null array)", fn);
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, K, &T));

    std::unique_ptr<Knn> h(new Knn());
    MFX_TRY(h->init(X->cols, K, device));
    hipStream_t st = h->st_;
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t rows = (uint32_t) X->rows, cols = (uint32_t) X->cols, nnz = (uint32_t) X->nnz;
    Staged<uint32_t> ptr, idx, cptr, ridx;
    Staged<float> val, cval;
    MFX_TRY(ptr.set(X->csr_row_ptr, (size_t) rows + 1, space, st));
    MFX_TRY(idx.set(X->csr_col_idx, nnz, space, st));
    MFX_TRY(val.set(X->csr_val, nnz, space, st));
    MFX_TRY(cptr.set(X->csc_col_ptr, (size_t) cols + 1, space, st));
    MFX_TRY(ridx.set(X->csc_row_idx, nnz, space, st));
    MFX_TRY(cval.set(X->csc_val, nnz, space, st));

    FirstBad bad_row, bad_col, long_col, bad_term;
    for (FirstBad* f : {&bad_row, &bad_col, &long_col, &bad_term}) MFX_TRY(f->init(st));
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

    // the work of every item, and the order of the queue: heaviest first, ties by item
    DevBuf<unsigned long long> work;
    MFX_TRY(work.alloc(cols));
    hipLaunchKernelGGL(k_knn_work, dim3(grid_256((uint64_t) cols * 64)), dim3(256), 0, st, ptr.p, cptr.p, ridx.p, cols, work.get(), long_col.w.get());
    MFX_LAUNCH_CHECK();
    std::vector<unsigned long long> hwork(cols);
    MFX_HIP(hipMemcpyAsync(hwork.data(), work.get(), sizeof(unsigned long long) * cols, hipMemcpyDeviceToHost, st));
    MFX_TRY(long_col.read(st, &first));
    MFX_REQUIRE(first == kNone, "%s: item %u: a column of more than 2^21 entries", fn, first);
    std::vector<uint32_t> horder(cols);
    std::iota(horder.begin(), horder.end(), 0u);
    std::sort(horder.begin(), horder.end(), [&](uint32_t x, uint32_t y) { return hwork[x] > hwork[y] || (hwork[x] == hwork[y] && x < y); });
    DevBuf<uint32_t> order, queue;
    MFX_TRY(order.alloc(cols));
    MFX_TRY(order.upload(horder.data(), cols, MFX_HOST, st));
    MFX_TRY(queue.alloc_zero(1, st));
    MFX_HIP(hipStreamSynchronize(st));
    h->t_[0] = since(t0);

    const auto t1 = std::chrono::steady_clock::now();
    KnnBuildArgs a{};
    a.ptr = ptr.p; a.idx = idx.p; a.val = val.p;
    a.cptr = cptr.p; a.ridx = ridx.p; a.cval = cval.p;
    a.order = order.get(); a.queue = queue.get(); a.first_bad = bad_term.w.get();
    a.nidx = h->nidx_.get(); a.nsim = h->nsim_.get();
    a.cols = cols; a.T = T; a.K = K; a.NC = knn_area(K);
    const size_t lds = knn_lds_bytes((int) T, K);
    MFX_TRY(allow_lds(k_knn_build, lds));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(cols, (uint64_t) h->cus_ * 2);
    hipLaunchKernelGGL(k_knn_build, dim3(grid), dim3(kKnnThreads), lds, st, a);
    MFX_LAUNCH_CHECK();
    MFX_TRY(bad_term.read(st, &first));
    h->t_[1] = since(t1);
    MFX_REQUIRE(first == kNone, "%s: item %u: a term x_ui * x_uj that is not finite or of magnitude >= 64", fn, first);
    *out = h.release();
    return MFX_OK;
}

int Knn::from_lists(Knn** out, int64_t cols, int32_t K, const uint32_t* nbr_idx, const float* nbr_sim, mfx_memspace space, int device) {
    const char* fn = "mfx_knn_create_from_lists";
    MFX_REQUIRE(out && nbr_idx && nbr_sim, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(K >= 1 && K <= 1024, "%s: K must be in [1, 1024] (got %d)", fn, K);
    MFX_REQUIRE(cols >= 2 && cols < 0xFFFFFFFFll, "%s: cols must be in [2, 2^32 - 1) (got %lld)", fn, (long long) cols);
    std::unique_ptr<Knn> h(new Knn());
    MFX_TRY(h->init(cols, K, device));
    hipStream_t st = h->st_;
    const auto t0 = std::chrono::steady_clock::now();
    MFX_TRY(h->nidx_.upload(nbr_idx, (size_t) cols * K, space, st));
    MFX_TRY(h->nsim_.upload(nbr_sim, (size_t) cols * K, space, st));
    FirstBad bad;
    MFX_TRY(bad.init(st));
    hipLaunchKernelGGL(k_knn_check_lists, dim3(grid_256((uint64_t) cols)), dim3(256), 0, st, h->nidx_.get(), h->nsim_.get(), (uint32_t) cols, (int) K,
                       bad.w.get());
    MFX_LAUNCH_CHECK();
    uint32_t first = kNone;
    MFX_TRY(bad.read(st, &first));
    h->t_[0] = since(t0);
    MFX_REQUIRE(first == kNone, "%s: item %u: its ids must be below cols or pad, pads at the tail only, similarities of real slots finite", fn,
                first);
    *out = h.release();
    return MFX_OK;
}

int Knn::lists(uint32_t* nbr_idx, float* nbr_sim, mfx_memspace space) {
    MFX_TRY(check_space("mfx_knn_lists", space));
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t n = (size_t) cols_ * K_;
    if (nbr_idx) MFX_HIP(hipMemcpyAsync(nbr_idx, nidx_.get(), sizeof(uint32_t) * n, kind, st_));
    if (nbr_sim) MFX_HIP(hipMemcpyAsync(nbr_sim, nsim_.get(), sizeof(float) * n, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Knn::neighbours(int64_t nq, const uint32_t* items, int32_t n_top, uint32_t* out_items, float* out_sims, mfx_memspace space) {
    const char* fn = "mfx_knn_neighbours";
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(n_top >= 1 && n_top <= K_, "%s: n_top must be in [1, K = %d] (got %d)", fn, K_, n_top);
    MFX_REQUIRE(nq >= 0 && nq < 0xFFFFFFFFll, "%s: nq must be in [0, 2^32 - 1) (got %lld)", fn, (long long) nq);
    MFX_REQUIRE(items || nq <= cols_, "%s: items = NULL asks for the items 0 .. nq - 1: nq must not exceed cols", fn);
    if (nq == 0) return MFX_OK;
    MFX_REQUIRE(out_items, "%s: out_items is NULL", fn);
    MFX_TRY(use_device(device_));
    const size_t total = (size_t) nq * n_top;
    Staged<uint32_t> q;
    if (items) MFX_TRY(q.set(items, (size_t) nq, space, st_));
    DevBuf<uint32_t> oi;
    DevBuf<float> os;
    uint32_t* di = out_items;
    float* dsim = out_sims;
    if (space == MFX_HOST) {
        MFX_TRY(oi.alloc(total));
        di = oi.get();
        if (out_sims) {
            MFX_TRY(os.alloc(total));
            dsim = os.get();
        }
    }
    FirstBad bad;
    MFX_TRY(bad.init(st_));
    hipLaunchKernelGGL(k_knn_neighbours, dim3(grid_256(total)), dim3(256), 0, st_, nidx_.get(), nsim_.get(), q.p, (uint64_t) nq, (uint32_t) cols_, K_,
                       (int) n_top, di, dsim, bad.w.get());
    MFX_LAUNCH_CHECK();
    uint32_t first = kNone;
    MFX_TRY(bad.read(st_, &first));
    MFX_REQUIRE(first == kNone, "%s: query %u names an item >= cols", fn, first);
    if (space == MFX_HOST) {
        MFX_HIP(hipMemcpyAsync(out_items, di, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, st_));
        if (out_sims) MFX_HIP(hipMemcpyAsync(out_sims, dsim, sizeof(float) * total, hipMemcpyDeviceToHost, st_));
        MFX_HIP(hipStreamSynchronize(st_));
    }
    return MFX_OK;
}

int Knn::recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                   int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    const char* fn = "mfx_knn_recommend";
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(n_top >= 1 && n_top <= 1024, "%s: n_top must be in [1, 1024] (got %d)", fn, n_top);
    MFX_REQUIRE((flags & ~MFX_KNN_KEEP_SEEN) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) flags);
    MFX_REQUIRE(nusers >= 0 && nusers < 0xFFFFFFFFll && nnz >= 0 && nnz < 0xFFFFFFFFll, "%s: nusers and nnz must be in [0, 2^32 - 1)", fn);
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, cols_, n_top, &T));
    if (bad_rows) *bad_rows = 0;
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(ptr && items, "%s: ptr or items is NULL", fn);
    MFX_REQUIRE(nnz == 0 || (idx && val), "%s: idx or val is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
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
    MFX_TRY(sp.set(ptr, (size_t) nusers + 1, space, st));
    MFX_TRY(si.set(idx, (size_t) nnz, space, st));
    MFX_TRY(sv.set(val, (size_t) nnz, space, st));
    const size_t total = (size_t) nusers * n_top;
    DevBuf<uint32_t> oi;
    DevBuf<float> os;
    uint32_t* di = items;
    float* dsc = scores;
    if (space == MFX_HOST) {
        MFX_TRY(oi.alloc(total));
        di = oi.get();
        if (scores) {
            MFX_TRY(os.alloc(total));
            dsc = os.get();
        }
    }
    DevBuf<unsigned long long> nbad;
    MFX_TRY(nbad.alloc_zero(1, st));
    FirstBad bad;
    MFX_TRY(bad.init(st));
    MFX_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_knn_check, dim3(grid_256((uint64_t) nusers)), dim3(256), 0, st, sp.p, si.p, (uint32_t) nusers, (uint32_t) cols_, (uint32_t) nnz,
                       bad.w.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev[1], st));
    uint32_t first = kNone;
    MFX_TRY(bad.read(st, &first));
    MFX_REQUIRE(first == kNone, "%s: row %u: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols", fn, first);

    KnnRecArgs a{};
    a.ptr = sp.p; a.idx = si.p; a.val = sv.p;
    a.nidx = nidx_.get(); a.nsim = nsim_.get();
    a.items = di; a.scores = dsc; a.bad_rows = nbad.get();
    a.nusers = (uint32_t) nusers; a.cols = (uint32_t) cols_; a.T = T;
    a.K = K_; a.n_top = n_top; a.NC = knn_area(n_top);
    a.keep_seen = (flags & MFX_KNN_KEEP_SEEN) != 0;
    const size_t lds = knn_lds_bytes((int) T, n_top);
    MFX_TRY(allow_lds(k_knn_recommend, lds));
    const uint32_t grid = (uint32_t) std::min<uint64_t>((uint64_t) nusers, (uint64_t) cus_ * 8);
    hipLaunchKernelGGL(k_knn_recommend, dim3(grid), dim3(kKnnThreads), lds, st, a);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev[2], st));
    unsigned long long hbad = 0;
    MFX_HIP(hipMemcpyAsync(&hbad, nbad.get(), sizeof(hbad), hipMemcpyDeviceToHost, st));
    if (space == MFX_HOST) {
        MFX_HIP(hipMemcpyAsync(items, di, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, dsc, sizeof(float) * total, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    MFX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    t_[2] += 1e-3 * ms;
    MFX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    t_[3] += 1e-3 * ms;
    if (bad_rows) *bad_rows = (int64_t) hbad;
    return MFX_OK;
}

}  // namespace mfx
