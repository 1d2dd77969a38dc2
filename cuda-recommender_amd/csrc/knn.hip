// knn.hip -- item-kNN on the interaction matrix (mfx_knn_*) on gfx950: the sparse X^T X with a top-K per row, and the
// recommendation from the stored lists.  The contract -- the fp32 term, the 2^-36 fixed-point integer sums, the order and the
// limits -- is in include/mfx.h; DESIGN 5.16 has the sizing.
//
// Build and recommend stand on the shared layer of knn_device.hpp.  k_knn_build is knn_build_items (the work queue) around
// knn_row over BuildSrc, which takes the users of column i in batches of 64 per wave (one lane per user for the
// row pointers and the lower-bound search of the tile's start in the sorted row, then the lanes across each row).  Recommend
// is k_knn_rows over RecSrc, which runs the threads across the n_u * K (entry, slot) pairs of the query row, behind
// rows_recommend on the host.
#include <chrono>
#include <memory>

#include "knn.hpp"
#include "knn_device.hpp"

namespace mfx {

namespace {

// Recommend: the scores of one query row.  For every entry (i, x) of the row and every stored slot (j, s) of i the term
// fp32(x * s) goes to accumulator j; with several tiles the pairs are walked once per tile.
struct RecSrc : RowSrc {
    const uint32_t* nidx;  // [cols][K]
    const float* nsim;
    uint32_t K;

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
};

// ---------------------------------------------------------------------------------------------- kernels
struct KnnBuildArgs : BuildArgs {
    uint32_t* nidx;  // [cols][K]
    float* nsim;
    int K, NC;
};

__global__ __launch_bounds__(kKnnThreads) void k_knn_build(KnnBuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char knn_raw[];
    const KnnLds s = knn_lds(knn_raw, (int) a.T, a.NC);
    knn_build_items(s, a, [&](const BuildSrc& src) {
        const int count = knn_row(s, src, a.cols, a.T, a.K);
        knn_store(s, count, a.K, true, a.nidx + (size_t) src.item * a.K, a.nsim + (size_t) src.item * a.K);
        const bool bad = threadIdx.x == 0 && s.ctl[3];
        __syncthreads();  // (the area and ctl are free for the next item)
        return bad;
    });
}

// The fields of RowsArgs under their names, with the model's own among them in the order this struct always had: derived
// from RowsArgs (the model's fields behind the others) the all-user recommendation at K = 20 measured 1.0 % slower in three
// jobs, in this order it meets the parent's time.  k_knn_rows and rows_recommend go by the names.
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
    __device__ RecSrc source(const RowSrc& row) const { return RecSrc{row, nidx, nsim, (uint32_t) K}; }
};

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
    MFX_TRY(device_cus(device, &cus_));
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
    MFX_TRY(check_x(fn, X));
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, K, &T));

    std::unique_ptr<Knn> h(new Knn());
    MFX_TRY(h->init(X->cols, K, device));
    hipStream_t st = h->st_;
    const auto t0 = std::chrono::steady_clock::now();
    StagedX x;
    MFX_TRY(x.set(fn, X, space, st));
    BuildPass pass;
    MFX_TRY(pass.begin(st));  // (its two words belong to t_[0], as they always did; work_order ends at a synchronised stream)
    DevBuf<uint32_t> order;
    MFX_TRY(work_order(fn, x, st, &order));
    h->t_[0] = since(t0);

    const auto t1 = std::chrono::steady_clock::now();
    KnnBuildArgs a{};
    pass.fill(&a, x, order, T);
    a.nidx = h->nidx_.get(); a.nsim = h->nsim_.get();
    a.K = K; a.NC = knn_area(K);
    const int rc = pass.run(k_knn_build, fn, a, knn_lds_bytes((int) T, K), h->cus_, st);
    h->t_[1] = since(t1);
    MFX_TRY(rc);
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
    Out<uint32_t> oi;
    Out<float> os;
    MFX_TRY(oi.set(out_items, total, space));
    MFX_TRY(os.set(out_sims, total, space));
    FirstBad bad;
    MFX_TRY(bad.init(st_));
    hipLaunchKernelGGL(k_knn_neighbours, dim3(grid_256(total)), dim3(256), 0, st_, nidx_.get(), nsim_.get(), q.p, (uint64_t) nq, (uint32_t) cols_, K_,
                       (int) n_top, oi.p, os.p, bad.w.get());
    MFX_LAUNCH_CHECK();
    uint32_t first = kNone;
    MFX_TRY(bad.read(st_, &first));
    MFX_REQUIRE(first == kNone, "%s: query %u names an item >= cols", fn, first);
    MFX_TRY(oi.copy_out(out_items, total, space, st_));
    MFX_TRY(os.copy_out(out_sims, total, space, st_));
    if (space == MFX_HOST) MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Knn::recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                   int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return rows_recommend(k_knn_rows<KnnRecArgs>, "mfx_knn_recommend", cols_, cus_, device_, st_, &t_[2], &t_[3],
                          RowsQuery{nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space}, [&](KnnRecArgs* a) {
                              a->nidx = nidx_.get(); a->nsim = nsim_.get(); a->K = K_;
                          });
}

}  // namespace mfx
