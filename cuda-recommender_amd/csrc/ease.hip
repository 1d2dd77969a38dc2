// ease.hip -- EASE (mfx_ease_*) on gfx950: the closed-form dense item-item model B = I - P diag(P)^-1 with a zero diagonal,
// P = (X^T X + lambda I)^-1, and the recommendation from its rows.  The contract -- the bits of the Gram matrix, the chains
// of the inverse, the one division of a weight, the fma chain of a score, the limits -- is in include/mfx.h; DESIGN 5.19 has
// the kernels and the sizing.  The inverse is ease_inverse.hip.
//
// Kernels:
//   k_ease_diag       knn_diag: a wave per item, G_ii = fp32(d_i + lambda), d_i the integer sum of x_ui^2 over column i;
//   k_ease_gram       the build pass of item-kNN (knn_device.hpp: knn_build_items, BuildSrc::add_terms, knn_build_tiles) with
//                     the selection replaced by a dense write: with row i of X^T X in the LDS tile, the workgroup writes
//                     from_fixed(acc[t]) to G[i][base + t] (coalesced) and clears the tile;
//   k_ease_pdiag      P_jj into a vector, a P_jj that is not finite or not > 0 named;
//   k_ease_weights    elementwise, in place over P;
//   k_ease_check      a given B: finite, zero diagonal;
//   k_ease_recommend  a workgroup per query row walks the item axis in tiles of T; a thread owns the items tid + 512 q of the
//                     tile in registers, every wave walks the row's entries (64 at a time, broadcast), kKnnBatch entries'
//                     loads of B[i_e][base ...] in flight; the scores go to the LDS tile and knn_scan over KeyOfBits
//                     selects (knn_begin, knn_drop_seen and the host side, rows_recommend, are knn_device.hpp's too).
#include <memory>

#include "ease.hpp"
#include "knn_device.hpp"

namespace mfx {

namespace {

constexpr int kEaseOwn = 8192 / kKnnThreads;  // items of the widest tile that a thread owns

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// G_ii = fp32(d_i + lambda), d_i the fp32 of the integer sum of fp32(x * x) over column i.
__global__ __launch_bounds__(256) void k_ease_diag(const uint32_t* __restrict__ cptr, const float* __restrict__ cval, uint32_t cols, float lambda,
                                                   float* __restrict__ G, uint32_t* first_bad) {
    knn_diag(cptr, cval, cols, first_bad, [&](uint64_t i, float di) { G[(size_t) i * cols + i] = add_rn(di, lambda); });
}

struct EaseGramArgs : BuildArgs {
    float* G;  // [cols][cols]; the diagonal is k_ease_diag's
};

__global__ __launch_bounds__(kKnnThreads) void k_ease_gram(EaseGramArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ease_raw[];
    const KnnLds s = knn_lds(ease_raw, (int) a.T, 0);  // the tile and ctl: no candidate area
    knn_build_items(s, a, [&](const BuildSrc& src) {
        float* row = a.G + (size_t) src.item * a.cols;
        return knn_build_tiles(s, src, a.cols, a.T, [&](uint32_t base, uint32_t len) {
            for (uint32_t t = threadIdx.x; t < len; t += kKnnThreads) {
                if (base + t != src.item) row[base + t] = from_fixed(s.acc[t]);
                s.acc[t] = 0ull;
            }
        });
    });
}

// d[j] = P_jj; the smallest j whose P_jj is not finite or not > 0 goes to first_bad.
__global__ void k_ease_pdiag(const float* __restrict__ P, uint32_t n, float* __restrict__ d, uint32_t* first_bad) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (uint64_t) gridDim.x * blockDim.x) {
        const float p = P[(size_t) j * n + j];
        d[j] = p;
        if (!(p > 0.f) || !(p < INFINITY)) atomicMin(first_bad, (uint32_t) j);
    }
}

// B_ij = fp32(-P_ij / P_jj), B_ii = +0; B may be P.
__global__ __launch_bounds__(256) void k_ease_weights(const float* P, const float* __restrict__ d, uint32_t n, float* B) {
    const size_t total = (size_t) n * n;
    for (size_t e = (size_t) blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t) gridDim.x * 256) {
        const uint32_t i = (uint32_t) (e / n), j = (uint32_t) (e - (size_t) i * n);
        B[e] = i == j ? 0.f : __fdiv_rn(-P[e], d[j]);
    }
}

// A given B: every entry finite, the diagonal zero; the smallest bad row goes to first_bad.
__global__ __launch_bounds__(256) void k_ease_check(const float* __restrict__ B, uint32_t n, uint32_t* first_bad) {
    const size_t total = (size_t) n * n;
    for (size_t e = (size_t) blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t) gridDim.x * 256) {
        const uint32_t i = (uint32_t) (e / n), j = (uint32_t) (e - (size_t) i * n);
        const float b = B[e];
        if (!(__builtin_fabsf(b) < INFINITY) || (i == j && b != 0.f)) atomicMin(first_bad, i);
    }
}

struct EaseRecArgs : RowsArgs {
    const float* B;  // [cols][cols]
};

__global__ __launch_bounds__(kKnnThreads) void k_ease_recommend(EaseRecArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ease_raw[];
    const KnnLds s = knn_lds(ease_raw, (int) a.T, a.NC);
    knn_zero_tile(s, a.T);
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    for (uint32_t r = blockIdx.x; r < a.nusers; r += gridDim.x) {
        const uint32_t r0 = a.ptr[r], n = a.ptr[r + 1] - r0;
        const uint32_t* idx = a.idx + r0;
        const float* val = a.val + r0;
        int bad = n > kKnnMaxEntries;
        if (!bad)
            for (uint32_t e = tid; e < n; e += kKnnThreads) bad |= !(__builtin_fabsf(val[e]) < INFINITY);
        bad = __syncthreads_or(bad);
        int count = 0;
        if (!bad && n > 0) {  // (an empty row: pads, and not bad)
            knn_begin(s);
            for (uint32_t base = 0; base < a.cols; base += min(a.T, a.cols - base)) {
                const uint32_t len = min(a.T, a.cols - base);
                const int nq = (int) ((len + kKnnThreads - 1) / kKnnThreads);  // (the same for every thread)
                float sc[kEaseOwn];
#pragma unroll
                for (int q = 0; q < kEaseOwn; ++q) sc[q] = 0.f;
                for (uint32_t e0 = 0; e0 < n; e0 += 64) {  // every wave walks every entry: a lane loads one, all take each in turn
                    const uint32_t e = e0 + lane;
                    const uint32_t il = e < n ? idx[e] : 0u;
                    const float xl = e < n ? val[e] : 0.f;
                    const int nb = (int) min(64u, n - e0);
                    for (int l = 0; l < nb; l += kKnnBatch) {
                        float w[kKnnBatch][kEaseOwn];
#pragma unroll
                        for (int b = 0; b < kKnnBatch; ++b) {
                            if (l + b >= nb) break;
                            const float* row = a.B + (size_t) __shfl(il, l + b) * a.cols + base + tid;
#pragma unroll
                            for (int q = 0; q < kEaseOwn; ++q)
                                if (q < nq) w[b][q] = tid + (uint32_t) q * kKnnThreads < len ? row[(size_t) q * kKnnThreads] : 0.f;
                        }
#pragma unroll
                        for (int b = 0; b < kKnnBatch; ++b) {
                            if (l + b >= nb) break;
                            const float x = __shfl(xl, l + b);
#pragma unroll
                            for (int q = 0; q < kEaseOwn; ++q)
                                if (q < nq) sc[q] = __fmaf_rn(x, w[b][q], sc[q]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < kEaseOwn; ++q) {
                    const uint32_t slot = tid + (uint32_t) q * kKnnThreads;
                    if (q < nq && slot < len) s.acc[slot] = sc[q] != sc[q] ? 0ull : kKnnLive | __float_as_uint(sc[q]);
                }
                __syncthreads();
                if (!a.keep_seen) {
                    knn_drop_seen(s.acc, idx, n, base, len);
                    __syncthreads();
                }
                knn_scan(s, base, len, a.n_top, KeyOfBits());
            }
            count = knn_sort_keep(s, a.n_top);
        }
        knn_store(s, count, a.n_top, !bad, a.items + (size_t) r * a.n_top, a.scores ? a.scores + (size_t) r * a.n_top : nullptr);
        if (tid == 0 && bad) atomicAdd(a.bad_rows, 1ull);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- host helpers
int check_lambda(const char* fn, float lambda) {
    MFX_REQUIRE(lambda > 0.f && lambda < INFINITY, "%s: lambda must be finite and > 0 (got %g)", fn, (double) lambda);
    return MFX_OK;
}

int check_cols(const char* fn, int64_t cols) {
    MFX_REQUIRE(cols >= 2 && cols <= (int64_t) kEaseMaxCols, "%s: cols must be in [2, %u] (got %lld)", fn, kEaseMaxCols, (long long) cols);
    return MFX_OK;
}

int check_inv_flags(const char* fn, int flags) {
    MFX_REQUIRE((flags & ~MFX_EASE_INV_SIMPLE) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) flags);
    return MFX_OK;
}

uint32_t grid_stride(size_t total, int cus) { return (uint32_t) std::min<size_t>((total + 255) / 256, (size_t) cus * 32); }

// The Gram pass: G [cols][cols] on the device from the checked matrix.
int gram_pass(const char* fn, const StagedX& x, const DevBuf<uint32_t>& order, float lambda, uint32_t T, int cus, hipStream_t st, float* G) {
    BuildPass pass;
    MFX_TRY(pass.begin(st));
    hipLaunchKernelGGL(k_ease_diag, dim3(grid_256((uint64_t) x.cols * 64)), dim3(256), 0, st, x.cptr.p, x.cval.p, x.cols, lambda, G,
                       pass.bad_term.w.get());
    MFX_LAUNCH_CHECK();
    EaseGramArgs a{};
    pass.fill(&a, x, order, T);
    a.G = G;
    return pass.run(k_ease_gram, fn, a, knn_tile_bytes(T), cus, st);
}

// P ~ G^-1 on the device (both [n][n]); the workspace lives for the call.  Synchronises.
int inverse_pass(const char* fn, uint32_t n, const float* G, float* P, int flags, hipStream_t st) {
    DevBuf<float> ws;
    MFX_TRY(alloc_named(fn, "the workspace of the inverse (3 padded copies)", &ws, ease_inverse_ws_floats(n)));
    DevBuf<uint32_t> nfail;
    MFX_TRY(nfail.alloc_zero(1, st));
    MFX_TRY(ease_inverse_launch(G, n, P, ws.get(), nfail.get(), flags, st));
    uint32_t bad = 0;
    MFX_HIP(hipMemcpyAsync(&bad, nfail.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_REQUIRE(bad == 0, "%s: A is not positive definite (%u pivots <= 0 or not finite): it must be symmetric, positive definite and finite", fn,
                bad);
    return MFX_OK;
}

// B from P on the device, B may be P.  Synchronises.
int weights_pass(const char* fn, uint32_t n, const float* P, float* B, int cus, hipStream_t st) {
    DevBuf<float> d;
    MFX_TRY(d.alloc(n));
    FirstBad bad;
    MFX_TRY(bad.init(st));
    hipLaunchKernelGGL(k_ease_pdiag, dim3(grid_256(n)), dim3(256), 0, st, P, n, d.get(), bad.w.get());
    MFX_LAUNCH_CHECK();
    uint32_t first = kNone;
    MFX_TRY(bad.read(st, &first));
    MFX_REQUIRE(first == kNone, "%s: item %u: P_jj must be finite and > 0", fn, first);
    hipLaunchKernelGGL(k_ease_weights, dim3(grid_stride((size_t) n * n, cus)), dim3(256), 0, st, P, d.get(), n, B);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

// The end of a stand-alone call with an [n][n] result.  Synchronises.
int finish(Out<float>& r, float* out, size_t count, mfx_memspace space, hipStream_t st) {
    MFX_TRY(r.copy_out(out, count, space, st));
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- Ease
int Ease::init(int64_t cols, int device) {
    cols_ = cols; device_ = device;
    MFX_TRY(use_device(device));
    MFX_TRY(device_cus(device, &cus_));
    return MFX_OK;
}

int Ease::gram(const mfx_csx* X, float lambda, int32_t tile_items, float* G, mfx_memspace space, int device) {
    const char* fn = "mfx_ease_gram";
    MFX_REQUIRE(X && G, "%s: null argument", fn);
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_lambda(fn, lambda));
    MFX_TRY(check_x(fn, X));
    MFX_TRY(check_cols(fn, X->cols));
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, 1, &T));
    MFX_TRY(use_device(device));
    int cus = 1;
    MFX_TRY(device_cus(device, &cus));
    hipStream_t st = nullptr;
    StagedX x;
    MFX_TRY(x.set(fn, X, space, st));
    DevBuf<uint32_t> order;
    MFX_TRY(work_order(fn, x, st, &order));
    const size_t nn = (size_t) X->cols * X->cols;
    Out<float> g;
    MFX_TRY(g.set(G, nn, space, fn, "the Gram matrix [cols][cols]"));
    MFX_TRY(gram_pass(fn, x, order, lambda, T, cus, st, g.p));
    return finish(g, G, nn, space, st);
}

int Ease::inverse(int64_t n, const float* A, float* Ainv, int flags, mfx_memspace space, int device) {
    const char* fn = "mfx_ease_inverse";
    MFX_REQUIRE(A && Ainv, "%s: null argument", fn);
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_inv_flags(fn, flags));
    MFX_REQUIRE(n >= 1 && n <= (int64_t) kEaseMaxCols, "%s: n must be in [1, %u] (got %lld)", fn, kEaseMaxCols, (long long) n);
    MFX_TRY(use_device(device));
    hipStream_t st = nullptr;
    const size_t nn = (size_t) n * n;
    Staged<float> a;
    MFX_TRY(a.set(A, nn, space, st));
    Out<float> p;
    MFX_TRY(p.set(Ainv, nn, space, fn, "the inverse [n][n]"));
    MFX_TRY(inverse_pass(fn, (uint32_t) n, a.p, p.p, flags, st));
    return finish(p, Ainv, nn, space, st);
}

int Ease::weights_from_inverse(int64_t n, const float* P, float* B, mfx_memspace space, int device) {
    const char* fn = "mfx_ease_weights_from_inverse";
    MFX_REQUIRE(P && B, "%s: null argument", fn);
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_cols(fn, n));
    MFX_TRY(use_device(device));
    int cus = 1;
    MFX_TRY(device_cus(device, &cus));
    hipStream_t st = nullptr;
    const size_t nn = (size_t) n * n;
    Staged<float> p;
    MFX_TRY(p.set(P, nn, space, st));
    Out<float> b;
    MFX_TRY(b.set(B, nn, space, fn, "the weights [n][n]"));
    MFX_TRY(weights_pass(fn, (uint32_t) n, p.p, b.p, cus, st));
    return finish(b, B, nn, space, st);
}

int Ease::train(Ease** out, const mfx_csx* X, float lambda, int flags, int32_t tile_items, mfx_memspace space, int device) {
    const char* fn = "mfx_ease_train";
    MFX_REQUIRE(out && X, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_inv_flags(fn, flags));
    MFX_TRY(check_lambda(fn, lambda));
    MFX_TRY(check_x(fn, X));
    MFX_TRY(check_cols(fn, X->cols));
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, 1, &T));

    std::unique_ptr<Ease> h(new Ease());
    MFX_TRY(h->init(X->cols, device));
    hipStream_t st = h->st_;
    const uint32_t cols = (uint32_t) X->cols;
    const size_t nn = (size_t) cols * cols;
    DevBuf<float> G;
    {
        const auto t0 = std::chrono::steady_clock::now();
        StagedX x;
        MFX_TRY(x.set(fn, X, space, st));
        DevBuf<uint32_t> order;
        MFX_TRY(work_order(fn, x, st, &order));
        h->t_[0] = since(t0);

        const auto t1 = std::chrono::steady_clock::now();
        MFX_TRY(alloc_named(fn, "the Gram matrix [cols][cols]", &G, nn));
        MFX_TRY(gram_pass(fn, x, order, lambda, T, h->cus_, st, G.get()));
        h->t_[1] = since(t1);
    }
    const auto t2 = std::chrono::steady_clock::now();
    MFX_TRY(alloc_named(fn, "the inverse [cols][cols]", &h->B_, nn));
    MFX_TRY(inverse_pass(fn, cols, G.get(), h->B_.get(), flags, st));  // (its workspace is gone on return)
    G.release();
    h->t_[2] = since(t2);

    const auto t3 = std::chrono::steady_clock::now();
    MFX_TRY(weights_pass(fn, cols, h->B_.get(), h->B_.get(), h->cus_, st));  // in place over P
    h->t_[3] = since(t3);
    *out = h.release();
    return MFX_OK;
}

int Ease::from_weights(Ease** out, int64_t cols, const float* B, mfx_memspace space, int device) {
    const char* fn = "mfx_ease_create_from_weights";
    MFX_REQUIRE(out && B, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_cols(fn, cols));
    std::unique_ptr<Ease> h(new Ease());
    MFX_TRY(h->init(cols, device));
    const size_t nn = (size_t) cols * cols;
    MFX_TRY(alloc_named(fn, "the weights [cols][cols]", &h->B_, nn));
    MFX_TRY(h->B_.upload(B, nn, space, h->st_));
    FirstBad bad;
    MFX_TRY(bad.init(h->st_));
    hipLaunchKernelGGL(k_ease_check, dim3(grid_stride(nn, h->cus_)), dim3(256), 0, h->st_, h->B_.get(), (uint32_t) cols, bad.w.get());
    MFX_LAUNCH_CHECK();
    uint32_t first = kNone;
    MFX_TRY(bad.read(h->st_, &first));
    MFX_REQUIRE(first == kNone, "%s: row %u: every weight must be finite and the diagonal zero", fn, first);
    *out = h.release();
    return MFX_OK;
}

int Ease::weights(int64_t first, int64_t count, float* B_rows, mfx_memspace space) {
    const char* fn = "mfx_ease_weights";
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(first >= 0 && count >= 0 && first <= cols_ && count <= cols_ - first, "%s: rows [%lld, %lld + %lld) outside [0, %lld)", fn,
                (long long) first, (long long) first, (long long) count, (long long) cols_);
    if (count == 0) return MFX_OK;
    MFX_REQUIRE(B_rows, "%s: null argument", fn);
    MFX_TRY(use_device(device_));
    MFX_HIP(hipMemcpyAsync(B_rows, B_.get() + (size_t) first * cols_, sizeof(float) * (size_t) count * cols_,
                           space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Ease::recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                    int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return rows_recommend(k_ease_recommend, "mfx_ease_recommend", cols_, cus_, device_, st_, &t_[4], &t_[5],
                          RowsQuery{nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space},
                          [&](EaseRecArgs* a) { a->B = B_.get(); });
}

}  // namespace mfx
