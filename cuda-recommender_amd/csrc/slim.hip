// slim.hip -- SLIM on given supports (mfx_slim_*) on gfx950: for every item j the elastic-net regression of column j of X on
// the K columns of its support S_j, by covariance-update coordinate descent on the K x K Gram matrix of the support, and the
// recommendation from the trained weights.  The contract -- the Gram entries (item-kNN's similarities plus a diagonal), each
// fp32 operation of the solve in its order, the limits -- is in include/mfx.h; DESIGN 5.18 has the kernels and the sizing.
//
// Four kernels of its own and an instance of k_knn_rows (knn_device.hpp holds the layer shared with knn.hip and ease.hip):
//   k_slim_diag       knn_diag: a wave per item, d_a the integer sum of x_ua^2 over column a;
//   k_slim_gram       the build pass of item-kNN (knn_build_items, BuildSrc::add_terms, knn_build_tiles) with the selection
//                     replaced by a gather.  With row a of X^T X in the LDS tile, the workgroup writes row K of block a (a's
//                     own list) and, for every (j, p) of a's inverse list -- the lists S_j that hold a at slot p -- row p of
//                     block j, for the slots whose ids lie in the tile; then it clears the tile;
//   k_slim_solve      a wave per item: the block's Gram rows in LDS, lane b holds c_b and w_b (two per lane above K = 64), the
//                     scalar chain of coordinate a is computed by every lane alike, the K updates read row a of G from LDS;
//   k_knn_rows<SlimRecArgs>  knn_row over the transpose: a wave takes 64 entries of the query row, then its lanes run across
//                     each list (behind rows_recommend on the host).
// The inverse lists and the model's transpose are one structure (a counting sort on the host, targets ascending).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <numeric>

#include "knn_device.hpp"
#include "slim.hpp"

namespace mfx {

namespace {

constexpr int kSlimMaxK = 128;
constexpr int kSlimSolveWaves = 4;  // items per workgroup of the solve, as far as the LDS budget of knn_device.hpp allows

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// Item i's list: ids below cols, not i, distinct, pads at the tail only (and, given weights, those of real slots finite).
// nreal[i]: its real slots.
__global__ void k_slim_check_support(const uint32_t* S, const float* w, uint32_t cols, int K, uint32_t* nreal, uint32_t* first_bad) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < cols; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t* s = S + i * K;
        bool bad = false;
        int n = 0;
        for (int q = 0; q < K; ++q) {
            const uint32_t j = s[q];
            if (j == kPad) continue;
            if (n != q || j >= cols || j == (uint32_t) i || (w && !(__builtin_fabsf(w[i * K + q]) < INFINITY))) bad = true;
            for (int r = 0; r < q && !bad; ++r) bad = s[r] == j;
            if (bad) break;
            ++n;
        }
        nreal[i] = (uint32_t) n;
        if (bad) atomicMin(first_bad, (uint32_t) i);
    }
}

// d_a = the fp32 of the integer sum of fp32(x * x) over column a.
__global__ __launch_bounds__(256) void k_slim_diag(const uint32_t* __restrict__ cptr, const float* __restrict__ cval, uint32_t cols,
                                                   float* __restrict__ d, uint32_t* first_bad) {
    knn_diag(cptr, cval, cols, first_bad, [&](uint64_t i, float di) { d[i] = di; });
}

struct SlimGramArgs : BuildArgs {
    const uint32_t* S;      // [cols][K]
    const uint32_t* iptr;   // [cols + 1] the inverse lists: item a -> the (j, p) with S[j][p] == a
    const uint32_t* tj;
    const uint32_t* tp;
    const float* d;         // [cols]
    float* blocks;          // [cols][K + 1][K], zero on entry
    int K;
};

__global__ __launch_bounds__(kKnnThreads) void k_slim_gram(SlimGramArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char slim_raw[];
    const KnnLds s = knn_lds(slim_raw, (int) a.T, 0);  // the tile and ctl: no candidate area
    const uint32_t K = (uint32_t) a.K;
    const size_t blk = (size_t) (K + 1) * K;
    knn_build_items(s, a, [&](const BuildSrc& src) {
        const uint32_t i = src.item;
        const uint32_t e0 = a.iptr[i];
        const uint64_t npairs = (uint64_t) (a.iptr[i + 1] - e0) * K;
        const float di = a.d[i];
        return knn_build_tiles(s, src, a.cols, a.T, [&](uint32_t base, uint32_t len) {
            for (uint32_t t = threadIdx.x; t < K; t += kKnnThreads) {  // g of item i: row K of its own block
                const uint32_t id = a.S[(size_t) i * K + t], off = id - base;
                if (id != kPad && off < len) a.blocks[(size_t) i * blk + (size_t) K * K + t] = from_fixed(s.acc[off]);
            }
            for (uint64_t p = threadIdx.x; p < npairs; p += kKnnThreads) {  // row `slot` of every block whose list holds i
                const uint32_t er = npairs <= 0xFFFFFFFFull ? (uint32_t) p / K : (uint32_t) (p / K);
                const uint32_t t = (uint32_t) (p - (uint64_t) er * K);
                const uint32_t j = a.tj[e0 + er], slot = a.tp[e0 + er];
                const uint32_t id = a.S[(size_t) j * K + t], off = id - base;
                if (id == kPad || off >= len) continue;
                a.blocks[(size_t) j * blk + (size_t) slot * K + t] = id == i ? di : from_fixed(s.acc[off]);
            }
            __syncthreads();
            for (uint32_t t = threadIdx.x; t < len; t += kKnnThreads) s.acc[t] = 0ull;
        });
    });
}

struct SlimSolveArgs {
    const float* blocks;     // [n][K + 1][K]
    const uint32_t* nreal;   // [n] or NULL: K
    float* w;                // [n][K]
    int32_t* sweeps_used;    // [n]
    unsigned long long* failed;
    uint64_t n;
    int K, waves, stride;    // stride: floats of LDS per wave
    float l1, l2, tol;
    int sweeps;
    bool is_signed;
};

__global__ __launch_bounds__(64 * kSlimSolveWaves) void k_slim_solve(SlimSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char slim_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = a.K;
    const size_t blk = (size_t) (K + 1) * K;
    float* G = reinterpret_cast<float*>(slim_raw) + (size_t) wave * a.stride;
    for (uint64_t it = (uint64_t) blockIdx.x * a.waves + wave; it < a.n; it += (uint64_t) gridDim.x * a.waves) {
        const float* B = a.blocks + it * blk;
        const int n = a.nreal ? min((int) a.nreal[it], K) : K;
        // The wave alone uses its part of the LDS: the fences order its own reads and writes, lane against lane.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < n * K; q += 64) G[q] = B[q];
        float c0 = lane < n ? B[(size_t) K * K + lane] : 0.f;
        float c1 = lane + 64 < n ? B[(size_t) K * K + lane + 64] : 0.f;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float w0 = 0.f, w1 = 0.f;
        int used = 0;
        bool failed = false;
        for (int sw = 0; sw < a.sweeps; ++sw) {
            float m = 0.f;
            for (int ca = 0; ca < n; ++ca) {  // every lane computes the chain of coordinate ca alike
                const float d = G[ca * K + ca];
                const float den = add_rn(d, a.l2);
                if (!(den > 0.f)) continue;
                const int owner = ca & 63;
                const float wa = __shfl(ca < 64 ? w0 : w1, owner);
                const float cc = __shfl(ca < 64 ? c0 : c1, owner);
                const float z = __fmaf_rn(d, wa, cc);
                float t;
                if (a.is_signed) {
                    const float r = sub_rn(__builtin_fabsf(z), a.l1);
                    t = __builtin_copysignf(r > 0.f ? r : 0.f, z);
                } else {
                    const float r = sub_rn(z, a.l1);
                    t = r > 0.f ? r : 0.f;
                }
                const float v = __fdiv_rn(t, den);
                const float delta = sub_rn(v, wa);
                if (!(__builtin_fabsf(delta) < INFINITY)) {
                    failed = true;
                    break;
                }
                if (delta != 0.f) {
                    if (lane < n) c0 = __fmaf_rn(-delta, G[ca * K + lane], c0);
                    if (lane + 64 < n) c1 = __fmaf_rn(-delta, G[ca * K + lane + 64], c1);
                    if (lane == owner) {
                        if (ca < 64) w0 = v;
                        else w1 = v;
                    }
                    m = fmaxf(m, __builtin_fabsf(delta));
                }
            }
            if (failed) break;
            used = sw + 1;
            if (m <= a.tol) break;
        }
        if (lane < K) a.w[it * K + lane] = failed ? 0.f : w0;
        if (lane + 64 < K) a.w[it * K + lane + 64] = failed ? 0.f : w1;
        if (lane == 0) {
            a.sweeps_used[it] = failed ? 0 : used;
            if (failed) atomicAdd(a.failed, 1ull);
        }
    }
}

// The weights in the order of the transpose: tw[e] = w[tj[e]][tp[e]].
__global__ void k_slim_transpose_weights(const float* w, const uint32_t* tj, const uint32_t* tp, uint64_t n, int K, float* tw) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t) gridDim.x * blockDim.x)
        tw[e] = w[(size_t) tj[e] * K + tp[e]];
}

// Recommend: the scores of one query row.  For every entry (i, x) of the row and every stored (j, w) of source i the term
// fp32(x * w) goes to accumulator j.  The loop is BuildSrc's with lists in the place of rows: a wave takes 64 entries at a
// time, a lane each for the two list pointers and, past the first tile, for the lower-bound search of the tile's start in
// the ascending list; then list by list the lanes run across the targets, kKnnBatch loads in flight, and stop at the
// tile's end.  The lists of popular sources are long (an item that many lists name), and they carry most of the work.
struct SlimRecSrc : RowSrc {
    const uint32_t* iptr;  // [cols + 1]
    const uint32_t* tj;
    const float* tw;

    __device__ bool add_terms(unsigned long long* acc, uint32_t base, uint32_t len) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        bool bad = false;
        for (uint32_t e0 = 64u * wave; e0 < n; e0 += 64u * kKnnWaves) {
            const uint32_t e = e0 + lane;
            uint32_t a = 0, b = 0;
            float x = 0.f;
            if (e < n) {
                const uint32_t i = idx[e];
                x = val[e];
                a = iptr[i];
                b = iptr[i + 1];
                if (base > 0) {  // the first target of the ascending list at or after the tile's start
                    uint32_t hi = b;
                    while (a < hi) {
                        const uint32_t mid = a + (hi - a) / 2;
                        if (tj[mid] < base) a = mid + 1;
                        else hi = mid;
                    }
                }
            }
            const int nb = (int) min(64u, n - e0);
            for (int l = 0; l < nb; ++l) {
                const uint32_t ra = __shfl(a, l), rb = __shfl(b, l);
                const float rx = __shfl(x, l);
                // 64 * kKnnBatch targets of the list per round, their loads in flight together (wave-uniform loop)
                for (uint64_t r0 = ra; r0 < rb; r0 += 64 * kKnnBatch) {
                    uint32_t j[kKnnBatch];
                    float t[kKnnBatch];
#pragma unroll
                    for (int q = 0; q < kKnnBatch; ++q) {
                        const uint64_t p = r0 + 64u * q + lane;
                        j[q] = kPad;
                        t[q] = 0.f;
                        if (p < rb) {
                            j[q] = tj[p];
                            t[q] = mul_rn(rx, tw[p]);
                        }
                    }
                    if (__builtin_amdgcn_readfirstlane(j[0]) - base >= len) break;  // (ascending: the rest lies beyond the tile)
#pragma unroll
                    for (int q = 0; q < kKnnBatch; ++q) {
                        const uint32_t off = j[q] - base;  // (kPad - base >= len: base + len <= cols < 2^32 - 1)
                        if (off >= len) continue;
                        if (!(__builtin_fabsf(t[q]) < 64.f)) bad = true;
                        else atomicAdd(&acc[off], to_fixed(t[q]));
                    }
                }
            }
        }
        return bad;
    }
};

struct SlimRecArgs : RowsArgs {
    const uint32_t* iptr;
    const uint32_t* tj;
    const float* tw;
    __device__ SlimRecSrc source(const RowSrc& row) const { return SlimRecSrc{row, iptr, tj, tw}; }
};

// ---------------------------------------------------------------------------------------------- host helpers
int check_params(const char* fn, int32_t K, const SlimParams& p) {
    MFX_REQUIRE(K >= 1 && K <= kSlimMaxK, "%s: K must be in [1, %d] (got %d)", fn, kSlimMaxK, K);
    MFX_REQUIRE(p.l1 >= 0.f && p.l1 < INFINITY && p.l2 >= 0.f && p.l2 < INFINITY && p.tol >= 0.f && p.tol < INFINITY,
                "%s: l1, l2 and tol must be finite and >= 0 (got %g, %g, %g)", fn, (double) p.l1, (double) p.l2, (double) p.tol);
    MFX_REQUIRE(p.sweeps >= 1, "%s: sweeps must be at least 1 (got %d)", fn, p.sweeps);
    MFX_REQUIRE((p.flags & ~MFX_SLIM_SIGNED) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) p.flags);
    return MFX_OK;
}

// A checked support on the device and its inverse lists.
struct Support {
    DevBuf<uint32_t> S, nreal, iptr, tj, tp;
    size_t npairs = 0;

    // support [cols][K] (w [cols][K] or NULL) in `space`: copied, checked on the device, inverted by a counting sort here.
    int set(const char* fn, int64_t cols, int K, const uint32_t* support, const float* w, mfx_memspace space, hipStream_t st) {
        const size_t n = (size_t) cols * K;
        MFX_REQUIRE(n < 0xFFFFFFFFull, "%s: cols * K must be below 2^32 - 1 (the transpose is indexed with 32 bits)", fn);
        MFX_TRY(S.alloc(n));
        MFX_TRY(S.upload(support, n, space, st));
        MFX_TRY(nreal.alloc((size_t) cols));
        Staged<float> sw;
        if (w) MFX_TRY(sw.set(w, n, space, st));
        FirstBad bad;
        MFX_TRY(bad.init(st));
        hipLaunchKernelGGL(k_slim_check_support, dim3(grid_256((uint64_t) cols)), dim3(256), 0, st, S.get(), sw.p, (uint32_t) cols, K, nreal.get(),
                           bad.w.get());
        MFX_LAUNCH_CHECK();
        uint32_t first = kNone;
        MFX_TRY(bad.read(st, &first));
        MFX_REQUIRE(first == kNone,
                    "%s: item %u: the ids of its list must be distinct, below cols and not the item itself, pads at the tail only%s", fn, first,
                    w ? ", weights of real slots finite" : "");
        std::vector<uint32_t> copy;
        const uint32_t* hs = support;
        if (space == MFX_DEVICE) {
            copy.resize(n);
            MFX_HIP(hipMemcpyAsync(copy.data(), S.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
            MFX_HIP(hipStreamSynchronize(st));
            hs = copy.data();
        }
        std::vector<uint32_t> hptr((size_t) cols + 1, 0u);
        for (size_t q = 0; q < n; ++q)
            if (hs[q] != kPad) ++hptr[(size_t) hs[q] + 1];
        for (int64_t i = 0; i < cols; ++i) hptr[i + 1] += hptr[i];
        npairs = hptr[cols];
        std::vector<uint32_t> htj(npairs), htp(npairs), fill(hptr.begin(), hptr.end() - 1);
        for (int64_t j = 0; j < cols; ++j)  // (targets ascending inside every list)
            for (int p = 0; p < K; ++p) {
                const uint32_t i = hs[(size_t) j * K + p];
                if (i == kPad) break;
                htj[fill[i]] = (uint32_t) j;
                htp[fill[i]++] = (uint32_t) p;
            }
        MFX_TRY(iptr.alloc((size_t) cols + 1));
        MFX_TRY(iptr.upload(hptr.data(), (size_t) cols + 1, MFX_HOST, st));
        MFX_TRY(tj.alloc(npairs));
        MFX_TRY(tj.upload(htj.data(), npairs, MFX_HOST, st));
        MFX_TRY(tp.alloc(npairs));
        MFX_TRY(tp.upload(htp.data(), npairs, MFX_HOST, st));
        MFX_HIP(hipStreamSynchronize(st));  // (the host vectors go out of scope)
        return MFX_OK;
    }
};

// The Gram pass: the blocks [cols][K + 1][K] of the checked support into `blocks` (device memory).
int gram_pass(const char* fn, const StagedX& x, const DevBuf<uint32_t>& order, const uint32_t* S, const uint32_t* iptr, const uint32_t* tj,
              const uint32_t* tp, int K, uint32_t T, int cus, hipStream_t st, float* blocks) {
    const uint32_t cols = x.cols;
    BuildPass pass;
    DevBuf<float> d;
    MFX_TRY(d.alloc(cols));
    MFX_TRY(pass.begin(st));
    hipLaunchKernelGGL(k_slim_diag, dim3(grid_256((uint64_t) cols * 64)), dim3(256), 0, st, x.cptr.p, x.cval.p, cols, d.get(), pass.bad_term.w.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipMemsetAsync(blocks, 0, sizeof(float) * (size_t) cols * (K + 1) * K, st));
    SlimGramArgs a{};
    pass.fill(&a, x, order, T);
    a.S = S; a.iptr = iptr; a.tj = tj; a.tp = tp;
    a.d = d.get(); a.blocks = blocks; a.K = K;
    return pass.run(k_slim_gram, fn, a, knn_tile_bytes(T), cus, st);
}

// The name of the Gram workspace in its allocation failure.
std::string blocks_name(int64_t n) { return "the workspace of " + std::to_string(n) + " blocks [K + 1][K]"; }

int alloc_blocks(const char* fn, DevBuf<float>* blocks, int64_t n, int K) {
    return alloc_named(fn, blocks_name(n).c_str(), blocks, (size_t) n * (K + 1) * K);
}

// The solve of n blocks on the device: w [n][K], sweeps_used [n], *failed.  Synchronises.
int solve_pass(int64_t n, int K, const float* blocks, const uint32_t* nreal, const SlimParams& p, int cus, hipStream_t st, float* w,
               int32_t* sweeps_used, int64_t* failed) {
    DevBuf<unsigned long long> nfailed;
    MFX_TRY(nfailed.alloc_zero(1, st));
    SlimSolveArgs a{};
    a.blocks = blocks; a.nreal = nreal; a.w = w; a.sweeps_used = sweeps_used; a.failed = nfailed.get();
    a.n = (uint64_t) n; a.K = K;
    a.stride = (K * K + 3) / 4 * 4;  // the Gram rows; g goes to registers
    a.waves = std::max(1, std::min(kSlimSolveWaves, kKnnLdsBudget / (4 * a.stride)));
    a.l1 = p.l1; a.l2 = p.l2; a.tol = p.tol; a.sweeps = p.sweeps;
    a.is_signed = (p.flags & MFX_SLIM_SIGNED) != 0;
    const size_t lds = (size_t) a.waves * a.stride * 4;
    MFX_TRY(allow_lds(k_slim_solve, lds));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(((uint64_t) n + a.waves - 1) / a.waves, (uint64_t) cus * 8);
    hipLaunchKernelGGL(k_slim_solve, dim3(grid), dim3(64 * a.waves), lds, st, a);
    MFX_LAUNCH_CHECK();
    unsigned long long h = 0;
    MFX_HIP(hipMemcpyAsync(&h, nfailed.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    if (failed) *failed = (int64_t) h;
    return MFX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- Slim
int Slim::init(int64_t cols, int32_t K, int device) {
    cols_ = cols; K_ = K; device_ = device;
    MFX_TRY(use_device(device));
    MFX_TRY(device_cus(device, &cus_));
    MFX_TRY(w_.alloc((size_t) cols * K));
    MFX_TRY(sweeps_.alloc_zero((size_t) cols, st_));
    return MFX_OK;
}

int Slim::set_support(const char* fn, const uint32_t* support, const float* w, mfx_memspace space) {
    Support sup;
    MFX_TRY(sup.set(fn, cols_, K_, support, w, space, st_));
    S_ = std::move(sup.S); nreal_ = std::move(sup.nreal); iptr_ = std::move(sup.iptr); tj_ = std::move(sup.tj); tp_ = std::move(sup.tp);
    npairs_ = sup.npairs;
    return MFX_OK;
}

int Slim::transpose_weights() {
    MFX_TRY(tw_.alloc(npairs_));
    if (npairs_) {
        hipLaunchKernelGGL(k_slim_transpose_weights, dim3(grid_256(npairs_)), dim3(256), 0, st_, w_.get(), tj_.get(), tp_.get(), (uint64_t) npairs_, K_,
                           tw_.get());
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Slim::train(Slim** out, const mfx_csx* X, int32_t K, const uint32_t* support, const SlimParams& p, int32_t tile_items, int64_t* failed,
                mfx_memspace space, int device) {
    const char* fn = "mfx_slim_train";
    MFX_REQUIRE(out && X && support, "%s: null argument", fn);
    *out = nullptr;
    if (failed) *failed = 0;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_params(fn, K, p));
    MFX_TRY(check_x(fn, X));
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, K, &T));

    std::unique_ptr<Slim> h(new Slim());
    MFX_TRY(h->init(X->cols, K, device));
    hipStream_t st = h->st_;
    const auto t0 = std::chrono::steady_clock::now();
    StagedX x;
    MFX_TRY(x.set(fn, X, space, st));
    MFX_TRY(h->set_support(fn, support, nullptr, space));
    DevBuf<uint32_t> order;
    MFX_TRY(work_order(fn, x, st, &order));
    h->t_[0] = since(t0);

    const auto t1 = std::chrono::steady_clock::now();
    DevBuf<float> blocks;
    MFX_TRY(alloc_blocks(fn, &blocks, X->cols, K));
    MFX_TRY(gram_pass(fn, x, order, h->S_.get(), h->iptr_.get(), h->tj_.get(), h->tp_.get(), K, T, h->cus_, st, blocks.get()));
    h->t_[1] = since(t1);

    const auto t2 = std::chrono::steady_clock::now();
    MFX_TRY(solve_pass(X->cols, K, blocks.get(), h->nreal_.get(), p, h->cus_, st, h->w_.get(), h->sweeps_.get(), failed));
    MFX_TRY(h->transpose_weights());
    h->t_[2] = since(t2);
    *out = h.release();
    return MFX_OK;
}

int Slim::gram(const mfx_csx* X, int32_t K, const uint32_t* support, int32_t tile_items, float* blocks, mfx_memspace space, int device) {
    const char* fn = "mfx_slim_gram";
    MFX_REQUIRE(X && support && blocks, "%s: null argument", fn);
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(K >= 1 && K <= kSlimMaxK, "%s: K must be in [1, %d] (got %d)", fn, kSlimMaxK, K);
    MFX_TRY(check_x(fn, X));
    uint32_t T = 0;
    MFX_TRY(pick_tile(fn, tile_items, X->cols, K, &T));
    MFX_TRY(use_device(device));
    int cus = 1;
    MFX_TRY(device_cus(device, &cus));
    hipStream_t st = nullptr;
    StagedX x;
    MFX_TRY(x.set(fn, X, space, st));
    Support sup;
    MFX_TRY(sup.set(fn, X->cols, K, support, nullptr, space, st));
    DevBuf<uint32_t> order;
    MFX_TRY(work_order(fn, x, st, &order));
    const size_t count = (size_t) X->cols * (K + 1) * K;
    Out<float> b;
    MFX_TRY(b.set(blocks, count, space, fn, blocks_name(X->cols).c_str()));
    MFX_TRY(gram_pass(fn, x, order, sup.S.get(), sup.iptr.get(), sup.tj.get(), sup.tp.get(), K, T, cus, st, b.p));
    MFX_TRY(b.copy_out(blocks, count, space, st));
    if (space == MFX_HOST) MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int Slim::solve(int64_t n, int32_t K, const float* blocks, const uint32_t* n_real, const SlimParams& p, float* w, int32_t* sweeps_used,
                int64_t* failed, mfx_memspace space, int device) {
    const char* fn = "mfx_slim_solve";
    if (failed) *failed = 0;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_params(fn, K, p));
    MFX_REQUIRE(n >= 0 && n < 0xFFFFFFFFll, "%s: n must be in [0, 2^32 - 1) (got %lld)", fn, (long long) n);
    if (n == 0) return MFX_OK;
    MFX_REQUIRE(blocks && w && sweeps_used, "%s: null argument", fn);
    MFX_TRY(use_device(device));
    int cus = 1;
    MFX_TRY(device_cus(device, &cus));
    hipStream_t st = nullptr;
    Staged<float> sb;
    Staged<uint32_t> sn;
    MFX_TRY(sb.set(blocks, (size_t) n * (K + 1) * K, space, st));
    if (n_real) MFX_TRY(sn.set(n_real, (size_t) n, space, st));
    Out<float> ow;
    Out<int32_t> os;
    MFX_TRY(ow.set(w, (size_t) n * K, space));
    MFX_TRY(os.set(sweeps_used, (size_t) n, space));
    MFX_TRY(solve_pass(n, K, sb.p, sn.p, p, cus, st, ow.p, os.p, failed));
    MFX_TRY(ow.copy_out(w, (size_t) n * K, space, st));
    MFX_TRY(os.copy_out(sweeps_used, (size_t) n, space, st));
    if (space == MFX_HOST) MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int Slim::from_lists(Slim** out, int64_t cols, int32_t K, const uint32_t* support, const float* w, mfx_memspace space, int device) {
    const char* fn = "mfx_slim_create_from_lists";
    MFX_REQUIRE(out && support && w, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_REQUIRE(K >= 1 && K <= kSlimMaxK, "%s: K must be in [1, %d] (got %d)", fn, kSlimMaxK, K);
    MFX_REQUIRE(cols >= 2 && cols < 0xFFFFFFFFll, "%s: cols must be in [2, 2^32 - 1) (got %lld)", fn, (long long) cols);
    std::unique_ptr<Slim> h(new Slim());
    MFX_TRY(h->init(cols, K, device));
    const auto t0 = std::chrono::steady_clock::now();
    MFX_TRY(h->set_support(fn, support, w, space));
    MFX_TRY(h->w_.upload(w, (size_t) cols * K, space, h->st_));
    MFX_TRY(h->transpose_weights());
    h->t_[0] = since(t0);
    *out = h.release();
    return MFX_OK;
}

int Slim::weights(uint32_t* support, float* w, int32_t* sweeps_used, mfx_memspace space) {
    MFX_TRY(check_space("mfx_slim_weights", space));
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const size_t n = (size_t) cols_ * K_;
    if (support) MFX_HIP(hipMemcpyAsync(support, S_.get(), sizeof(uint32_t) * n, kind, st_));
    if (w) MFX_HIP(hipMemcpyAsync(w, w_.get(), sizeof(float) * n, kind, st_));
    if (sweeps_used) MFX_HIP(hipMemcpyAsync(sweeps_used, sweeps_.get(), sizeof(int32_t) * (size_t) cols_, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Slim::recommend(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top, int flags,
                    int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return rows_recommend(k_knn_rows<SlimRecArgs>, "mfx_slim_recommend", cols_, cus_, device_, st_, &t_[3], &t_[4],
                          RowsQuery{nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space}, [&](SlimRecArgs* a) {
                              a->iptr = iptr_.get(); a->tj = tj_.get(); a->tw = tw_.get();
                          });
}

}  // namespace mfx
