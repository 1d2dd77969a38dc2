// lgcn.hip -- LightGCN (He et al. 2020) by deterministic mini-batch steps (mfx_lgcn_*) on gfx950: BPR on the mean of the base
// embeddings and their L propagated copies under the symmetrically normalised interaction graph.  The contract -- the
// scale tables, the 1024-entry segments of a row's sum, the layer mean and the update -- is in include/mfx.h; DESIGN 5.22
// has the choices and the measurements.
//
// A step runs on one stream:
//   forward    2 L launches of k_lgcn_propagate (one half-pass each: user rows from item rows, item rows from user rows),
//              each followed by k_lgcn_combine where the side has rows above 1024 entries; the running layer sum and, on the
//              last layer, the scale c_L are fused into the half-pass.  The result lands in the BprCore's factors.
//   gradient + scatter   BprCore::grad_scatter: k_bpr_grad and k_bpr_scatter of bpr.hip as they are, on the final embeddings.
//   backward   k_lgcn_collect (fixed-point sums -> G, accumulators and claims back to rest), then the same 2 L half-passes
//              on G: the normalised adjacency is symmetric, so the gradient of the base is the propagated mean of G.
//   update     k_lgcn_update over every row of the base.
// k_lgcn_propagate: groups of gs = min(64, pow2 >= k) lanes share a work item, lanes across coordinates.  A work item is a
// row of at most 1024 entries or one 1024-entry segment of a longer row; the items are walked heaviest first in the order
// made at create, group g taking the items g, g + groups, ...  The group loads gs ids and scales at a time, one per lane,
// hands them round (a wave-wide group: through scalar registers) and keeps 8 row loads in flight ahead of the FMA chain.
// The chain of a coordinate is one lane's: no sum crosses lanes, so no bit depends on gs, the grid or the order of the items.
#include <algorithm>
#include <cmath>
#include <memory>
#include <numeric>

#include "lgcn.hpp"
#include "bpr_device.hpp"

#ifndef MFX_LAUNCH_CHECK
#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())
#endif

namespace mfx {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kLgcnMaxBatch = 1 << 20;
constexpr int kLgcnMaxLayers = 8;
constexpr uint32_t kLgcnSegment = 1024;  // entries of one FMA chain (include/mfx.h: part of the contract)
constexpr int kLgcnThreads = 256;
constexpr int kLgcnInFlight = 8;         // row loads of a lane ahead of its chain
constexpr uint32_t kLgcnMaxGrid = 2048;  // workgroups of a half-pass: 8 per CU

inline uint32_t grid_of(uint64_t threads) { return (uint32_t) ((threads + kLgcnThreads - 1) / kLgcnThreads); }

// ---------------------------------------------------------------------------------------------- kernels
// Entry e of the CSC side, (row r, column c), must stand in row r of the CSR side.  Both sides hold nnz entries without
// duplicates (k_bpr_check), so then they hold the same pattern.
__global__ void k_lgcn_check_transpose(const uint32_t* __restrict__ cptr, const uint32_t* __restrict__ cidx, const uint32_t* __restrict__ rptr,
                                       const uint32_t* __restrict__ ridx, uint32_t cols, uint32_t nnz, uint32_t* first_bad) {
    for (uint64_t e64 = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e64 < nnz; e64 += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t e = (uint32_t) e64;
        uint32_t lo = 0, hi = cols;  // cptr[lo] <= e < cptr[hi]
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cptr[mid] <= e) lo = mid;
            else hi = mid;
        }
        const uint32_t r = cidx[e];
        uint32_t a = rptr[r], b = rptr[r + 1];
        const uint32_t end = b;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (ridx[mid] < lo) a = mid + 1;
            else b = mid;
        }
        if (!(a < end && ridx[a] == lo)) atomicMin(first_bad, lo);
    }
}

struct PropArgs {
    const uint4* work;      // [n_work] (row, first entry, end entry, partial slot or kNone), heaviest first
    const uint32_t* idx;    // the ids of the destination side's rows: rows of X
    const float* s_src;     // the scales of the rows of X
    const float* s_dst;     // the scales of the destination rows
    const float* X;         // [n_src][k] layer l of the other side
    float* part;            // [n_part][k] segment sums of the rows above 1024 entries
    float* out;             // [n_dst][k] layer l + 1 of this side, or NULL when no later layer reads it
    const float* sum_in;    // [n_dst][k] the layer sum so far (layer 0 itself for l = 0); may be sum_out
    float* sum_out;         // [n_dst][k]
    float c_last;           // c_L
    uint32_t n_work;
    int k, gs, gsh;         // gs = 1 << gsh lanes share a work item
    int last;               // the last layer: the sum is scaled by c_L
};

// The end of a destination row's coordinate: the scale, the layer's value, the running sum.
__device__ __forceinline__ void lgcn_finish(const PropArgs& a, size_t o, float s_r, float total) {
    const float r = mul_rn(s_r, total);
    if (a.out) a.out[o] = r;
    const float t = add_rn(a.sum_in[o], r);
    a.sum_out[o] = a.last ? mul_rn(t, a.c_last) : t;
}

// Lane `lane` of the group's value.  A wave-wide group reads it into a scalar register: the row address is then a scalar
// base and the lane's own offset.
template <bool WAVE>
__device__ __forceinline__ uint32_t group_get(uint32_t v, uint32_t lane, int gs) {
    if (WAVE) return (uint32_t) __builtin_amdgcn_readlane((int) v, (int) lane);
    return (uint32_t) __shfl((int) v, (int) lane, gs);
}

// NC coordinates per lane and turn of the coordinate loop; WAVE: gs = 64.
template <int NC, bool WAVE>
__global__ __launch_bounds__(kLgcnThreads) void k_lgcn_propagate(PropArgs a) {
    const int gs = WAVE ? 64 : a.gs, k = a.k;
    const uint32_t cl = threadIdx.x & (uint32_t) (gs - 1);
    uint32_t group = (blockIdx.x * (uint32_t) kLgcnThreads + threadIdx.x) >> (WAVE ? 6 : a.gsh);
    if (WAVE) group = (uint32_t) __builtin_amdgcn_readfirstlane((int) group);
    const uint32_t n_groups = (gridDim.x * (uint32_t) kLgcnThreads) >> (WAVE ? 6 : a.gsh);
    for (uint32_t w = group; w < a.n_work; w += n_groups) {  // the walk through the work order
        const uint4 it = a.work[w];
        const float s_r = a.s_dst[it.x];
        for (int c0 = 0; c0 < k; c0 += gs * NC) {  // the coordinate loop
            float acc[NC];
            size_t off[NC];
            bool on[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int c = c0 + q * gs + (int) cl;
                acc[q] = 0.f;
                on[q] = c < k;
                off[q] = (size_t) (on[q] ? c : 0);
            }
            for (uint32_t e0 = it.y; e0 < it.z; e0 += (uint32_t) gs) {  // gs entries at a time
                const uint32_t cnt = min((uint32_t) gs, it.z - e0);
                uint32_t my_id = 0, my_s = 0;
                if (cl < cnt) {
                    my_id = a.idx[e0 + cl];
                    my_s = __float_as_uint(a.s_src[my_id]);
                }
                for (uint32_t t = 0; t < cnt; t += kLgcnInFlight) {  // the loads in flight
                    float x[kLgcnInFlight][NC], sv[kLgcnInFlight];
#pragma unroll
                    for (int b = 0; b < kLgcnInFlight; ++b) {
                        const uint32_t lane = (t + b) & (uint32_t) (gs - 1);
                        const uint32_t id = group_get<WAVE>(my_id, lane, gs);
                        sv[b] = __uint_as_float(group_get<WAVE>(my_s, lane, gs));
                        const float* row = a.X + (size_t) id * k;
#pragma unroll
                        for (int q = 0; q < NC; ++q) x[b][q] = (t + b < cnt && on[q]) ? row[off[q]] : 0.f;
                    }
#pragma unroll
                    for (int b = 0; b < kLgcnInFlight; ++b) {
                        if (t + b < cnt) {
#pragma unroll
                            for (int q = 0; q < NC; ++q) acc[q] = __builtin_fmaf(sv[b], x[b][q], acc[q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                if (!on[q]) continue;
                if (it.w == kNone) lgcn_finish(a, (size_t) it.x * k + off[q], s_r, acc[q]);
                else a.part[(size_t) it.w * k + off[q]] = acc[q];
            }
        }
    }
}

// The rows above 1024 entries: one thread per (row, coordinate) adds the segment sums left to right.
__global__ __launch_bounds__(kLgcnThreads) void k_lgcn_combine(PropArgs a, const uint4* __restrict__ heavy, uint32_t n_heavy) {
    const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t hr = gid / (uint32_t) a.k;
    if (hr >= n_heavy) return;
    const uint32_t c = (uint32_t) (gid - hr * (uint32_t) a.k);
    const uint4 h = heavy[hr];
    float total = a.part[(size_t) h.y * a.k + c];
    for (uint32_t s = 1; s < h.z; ++s) total = add_rn(total, a.part[(size_t) (h.y + s) * a.k + c]);
    lgcn_finish(a, (size_t) h.x * a.k + c, a.s_dst[h.x], total);
}

// G = the fixed-point sums of the touched rows rounded once (k_bpr_apply's conversion), 0 elsewhere; the accumulators and
// the claims return to their rest state, the counts stay for k_lgcn_update.
__global__ __launch_bounds__(kLgcnThreads) void k_lgcn_collect(unsigned long long* __restrict__ acc, const uint32_t* __restrict__ cnt,
                                                               uint32_t* __restrict__ claim, float* __restrict__ G, uint64_t n, uint32_t k) {
    const uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * k) return;
    const uint64_t r = e / k;
    float g = 0.f;
    if (cnt[r]) {
        g = mul_rn((float) (long long) acc[e], 1.4551915228366852e-11f);
        acc[e] = 0ull;
        if (e == r * k) claim[r] = kNone;
    }
    G[e] = g;
}

// The base update of every row that a counted slot touched or (layers >= 1) that has a neighbour.
__global__ __launch_bounds__(kLgcnThreads) void k_lgcn_update(float* __restrict__ X0, const float* __restrict__ D, const uint32_t* __restrict__ cnt,
                                                              const float* __restrict__ s, uint64_t n, uint32_t k, int layers, float lr,
                                                              float lambda) {
    const uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * k) return;
    const uint64_t r = e / k;
    const uint32_t m = cnt[r];
    if (m == 0 && !(layers >= 1 && s[r] != 0.f)) return;
    const float old = X0[e];
    X0[e] = add_rn(old, mul_rn(lr, sub_rn(D[e], mul_rn(mul_rn(lambda, (float) m), old))));
}

int check_space(const char* fn, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    return MFX_OK;
}

int check_matrix(const char* fn, const mfx_csx* R) {
    MFX_REQUIRE(R->nnz >= 1, "%s: the matrix has no entries", fn);
    MFX_REQUIRE(R->cols >= 2, "%s: cols must be at least 2 (got %lld)", fn, (long long) R->cols);
    MFX_REQUIRE(R->rows >= 1 && R->rows < 0xFFFFFFFFll && R->cols < 0xFFFFFFFFll && R->nnz < 0xFFFFFFFFll,
                "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    MFX_REQUIRE(R->csr_row_ptr && R->csr_col_idx, "%s: the CSR side of R is NULL", fn);
    MFX_REQUIRE(R->csc_col_ptr && R->csc_row_idx, "%s: the CSC side of R is NULL", fn);
    return MFX_OK;
}

int check_sizes(const char* fn, int64_t k, int32_t layers, float lr, float lambda) {
    MFX_REQUIRE(k >= 1 && k <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k);
    MFX_REQUIRE(layers >= 0 && layers <= kLgcnMaxLayers, "%s: layers must be in [0, %d] (got %d)", fn, kLgcnMaxLayers, layers);
    MFX_REQUIRE(std::isfinite(lr) && lr >= 0.f, "%s: lr must be finite and >= 0 (got %g)", fn, (double) lr);
    MFX_REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "%s: lambda must be finite and >= 0 (got %g)", fn, (double) lambda);
    return MFX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- the graph
// The scale table and the work order of one side from its pointers (host).
int LgcnGraph::build_side(LgcnSide& side, const std::vector<uint32_t>& ptr) {
    const size_t n = ptr.size() - 1;
    std::vector<float> s(n);
    std::vector<uint4> work, heavy;
    work.reserve(n);
    uint32_t n_part = 0;
    side.heaviest = 0;
    for (size_t r = 0; r < n; ++r) {
        const uint32_t lo = ptr[r], hi = ptr[r + 1], d = hi - lo;
        s[r] = d ? (float) (1.0 / std::sqrt((double) d)) : 0.f;
        side.heaviest = std::max(side.heaviest, d);
        if (d <= kLgcnSegment) {
            work.push_back(make_uint4((uint32_t) r, lo, hi, kNone));
            continue;
        }
        const uint32_t nseg = (d + kLgcnSegment - 1) / kLgcnSegment;
        heavy.push_back(make_uint4((uint32_t) r, n_part, nseg, 0u));
        for (uint32_t g = 0; g < nseg; ++g)
            work.push_back(make_uint4((uint32_t) r, lo + g * kLgcnSegment, std::min(hi, lo + (g + 1) * kLgcnSegment), n_part + g));
        n_part += nseg;
    }
    std::stable_sort(work.begin(), work.end(), [](const uint4& x, const uint4& y) { return x.z - x.y > y.z - y.y; });
    side.n = (int64_t) n;
    side.n_work = (uint32_t) work.size();
    side.n_heavy = (uint32_t) heavy.size();
    side.n_part = n_part;
    MFX_TRY(side.s.alloc(n));
    MFX_TRY(side.work.alloc(work.size()));
    MFX_TRY(side.heavy.alloc(heavy.size()));
    MFX_TRY(side.part.alloc((size_t) n_part * k_));
    MFX_TRY(side.s.upload(s.data(), n, MFX_HOST, st_));
    MFX_TRY(side.work.upload(work.data(), work.size(), MFX_HOST, st_));
    MFX_TRY(side.heavy.upload(heavy.data(), heavy.size(), MFX_HOST, st_));
    MFX_HIP(hipStreamSynchronize(st_));  // (the host vectors end here)
    return MFX_OK;
}

int LgcnGraph::init(const char* fn, const mfx_csx* R, mfx_memspace space, int64_t k, int layers, int device, hipStream_t st) {
    rows_ = R->rows; cols_ = R->cols; nnz_ = R->nnz; k_ = k; layers_ = layers; device_ = device; st_ = st;
    MFX_TRY(use_device(device));
    const uint32_t rows = (uint32_t) rows_, cols = (uint32_t) cols_, nnz = (uint32_t) nnz_;
    MFX_TRY(user_.ptr.alloc((size_t) rows + 1));
    MFX_TRY(user_.idx.alloc(nnz));
    MFX_TRY(item_.ptr.alloc((size_t) cols + 1));
    MFX_TRY(item_.idx.alloc(nnz));
    MFX_TRY(user_.ptr.upload(R->csr_row_ptr, (size_t) rows + 1, space, st));
    MFX_TRY(user_.idx.upload(R->csr_col_idx, nnz, space, st));
    MFX_TRY(item_.ptr.upload(R->csc_col_ptr, (size_t) cols + 1, space, st));
    MFX_TRY(item_.idx.upload(R->csc_row_idx, nnz, space, st));
    uint32_t first_bad = kNone;
    MFX_TRY(bpr_check_rows(user_.ptr.get(), user_.idx.get(), rows, cols, nnz, st, &first_bad));
    MFX_REQUIRE(first_bad == kNone,
                "%s: row %u of the CSR side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols", fn,
                first_bad);
    MFX_TRY(bpr_check_rows(item_.ptr.get(), item_.idx.get(), cols, rows, nnz, st, &first_bad));
    MFX_REQUIRE(first_bad == kNone,
                "%s: column %u of the CSC side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below rows", fn,
                first_bad);
    DevBuf<uint32_t> bad;
    MFX_TRY(bad.alloc(1));
    MFX_HIP(hipMemsetAsync(bad.get(), 0xFF, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_lgcn_check_transpose, dim3(std::min<uint32_t>(grid_of(nnz), 65536u)), dim3(kLgcnThreads), 0, st, item_.ptr.get(),
                       item_.idx.get(), user_.ptr.get(), user_.idx.get(), cols, nnz, bad.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipMemcpyAsync(&first_bad, bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_REQUIRE(first_bad == kNone, "%s: column %u of the CSC side holds an entry that the CSR side lacks: the CSC side must be the transpose", fn,
                first_bad);
    // (the pointers are checked: the host copies may be trusted now)
    std::vector<uint32_t> rp((size_t) rows + 1), cp((size_t) cols + 1);
    MFX_HIP(hipMemcpyAsync(rp.data(), user_.ptr.get(), sizeof(uint32_t) * rp.size(), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipMemcpyAsync(cp.data(), item_.ptr.get(), sizeof(uint32_t) * cp.size(), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_TRY(build_side(user_, rp));
    MFX_TRY(build_side(item_, cp));
    for (int b = 0; b < 2; ++b) {
        if (layers < 2 + b) break;  // (E^1 is read by layer 2, E^2 by layer 3)
        MFX_TRY(layerW_[b].alloc((size_t) rows * k));
        MFX_TRY(layerH_[b].alloc((size_t) cols * k));
    }
    return MFX_OK;
}

int LgcnGraph::half_pass(const LgcnSide& dst, const float* s_src, const float* X, float* out, const float* sum_in, float* sum_out, bool last) {
    PropArgs a{};
    a.work = dst.work.get(); a.idx = dst.idx.get();
    a.s_src = s_src; a.s_dst = dst.s.get();
    a.X = X; a.part = dst.part.get(); a.out = out; a.sum_in = sum_in; a.sum_out = sum_out;
    a.c_last = 1.f / (float) (layers_ + 1);
    a.n_work = dst.n_work;
    a.k = (int) k_;
    a.gs = 1;
    while (a.gs < 64 && a.gs < a.k) a.gs *= 2;
    a.gsh = __builtin_ctz((unsigned) a.gs);
    a.last = last ? 1 : 0;
    const uint32_t per_wg = (uint32_t) kLgcnThreads >> a.gsh;
    const dim3 grid(std::min<uint32_t>((dst.n_work + per_wg - 1) / per_wg, kLgcnMaxGrid)), block(kLgcnThreads);
    if (a.gs < 64) hipLaunchKernelGGL((k_lgcn_propagate<1, false>), grid, block, 0, st_, a);
    else if (a.k <= 64) hipLaunchKernelGGL((k_lgcn_propagate<1, true>), grid, block, 0, st_, a);
    else if (a.k <= 128) hipLaunchKernelGGL((k_lgcn_propagate<2, true>), grid, block, 0, st_, a);
    else hipLaunchKernelGGL((k_lgcn_propagate<4, true>), grid, block, 0, st_, a);
    MFX_LAUNCH_CHECK();
    if (dst.n_heavy) {
        hipLaunchKernelGGL(k_lgcn_combine, dim3(grid_of((uint64_t) dst.n_heavy * a.k)), block, 0, st_, a, dst.heavy.get(), dst.n_heavy);
        MFX_LAUNCH_CHECK();
    }
    return MFX_OK;
}

int LgcnGraph::propagate(const float* inW, const float* inH, float* outW, float* outH) {
    if (layers_ == 0) {  // (c_0 = 1: the mean of one layer is the layer)
        MFX_HIP(hipMemcpyAsync(outW, inW, sizeof(float) * rows_ * k_, hipMemcpyDeviceToDevice, st_));
        MFX_HIP(hipMemcpyAsync(outH, inH, sizeof(float) * cols_ * k_, hipMemcpyDeviceToDevice, st_));
        return MFX_OK;
    }
    const float *srcW = inW, *srcH = inH;
    for (int l = 0; l < layers_; ++l) {
        const bool last = l + 1 == layers_;
        float* nextW = last ? nullptr : layerW_[l & 1].get();
        float* nextH = last ? nullptr : layerH_[l & 1].get();
        MFX_TRY(half_pass(user_, item_.s.get(), srcH, nextW, l == 0 ? inW : outW, outW, last));
        MFX_TRY(half_pass(item_, user_.s.get(), srcW, nextH, l == 0 ? inH : outH, outH, last));
        srcW = nextW;
        srcH = nextH;
    }
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- one step
LgcnCore::~LgcnCore() {
    for (auto e : ev_)
        if (e) (void) hipEventDestroy(e);
}

int LgcnCore::init(const char* fn, const mfx_csx* R, mfx_memspace space, int64_t k, int64_t batch, int layers, int device) {
    MFX_TRY(bpr_.init(R->rows, R->cols, k, batch, device));
    MFX_TRY(graph_.init(fn, R, space, k, layers, device, bpr_.st_));
    const size_t nw = (size_t) R->rows * k, nh = (size_t) R->cols * k;
    MFX_TRY(W0_.alloc(nw));
    MFX_TRY(H0_.alloc(nh));
    MFX_TRY(GW_.alloc(nw));
    MFX_TRY(GH_.alloc(nh));
    MFX_TRY(DW_.alloc(nw));
    MFX_TRY(DH_.alloc(nh));
    for (auto& e : ev_) MFX_HIP(hipEventCreate(&e));
    return MFX_OK;
}

int LgcnCore::set_base(const float* W0, const float* H0, mfx_memspace space) {
    MFX_TRY(use_device(bpr_.device_));
    MFX_TRY(W0_.upload(W0, (size_t) bpr_.rows_ * bpr_.k_, space, bpr_.st_));
    MFX_TRY(H0_.upload(H0, (size_t) bpr_.cols_ * bpr_.k_, space, bpr_.st_));
    MFX_HIP(hipStreamSynchronize(bpr_.st_));
    return MFX_OK;
}

int LgcnCore::get_base(float* W0, float* H0, mfx_memspace space) {
    MFX_TRY(use_device(bpr_.device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (W0) MFX_HIP(hipMemcpyAsync(W0, W0_.get(), sizeof(float) * bpr_.rows_ * bpr_.k_, kind, bpr_.st_));
    if (H0) MFX_HIP(hipMemcpyAsync(H0, H0_.get(), sizeof(float) * bpr_.cols_ * bpr_.k_, kind, bpr_.st_));
    MFX_HIP(hipStreamSynchronize(bpr_.st_));
    return MFX_OK;
}

int LgcnCore::forward() { return graph_.propagate(W0_.get(), H0_.get(), bpr_.W_.get(), bpr_.H_.get()); }

int LgcnCore::step(uint32_t n, float lr, float lambda) {
    if (n == 0) return MFX_OK;
    hipStream_t st = bpr_.st_;
    const uint64_t rows = (uint64_t) bpr_.rows_, cols = (uint64_t) bpr_.cols_;
    const uint32_t k = (uint32_t) bpr_.k_;
    bpr_.profile_ = profile_;
    if (profile_) MFX_HIP(hipEventRecord(ev_[1], st));
    MFX_TRY(forward());
    MFX_TRY(bpr_.grad_scatter(n));
    hipLaunchKernelGGL(k_lgcn_collect, dim3(grid_of(rows * k)), dim3(kLgcnThreads), 0, st, bpr_.accW_.get(), bpr_.cntW_.get(), bpr_.claimW_.get(),
                       GW_.get(), rows, k);
    MFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lgcn_collect, dim3(grid_of(cols * k)), dim3(kLgcnThreads), 0, st, bpr_.accH_.get(), bpr_.cntH_.get(), bpr_.claimH_.get(),
                       GH_.get(), cols, k);
    MFX_LAUNCH_CHECK();
    MFX_TRY(graph_.propagate(GW_.get(), GH_.get(), DW_.get(), DH_.get()));
    if (profile_) MFX_HIP(hipEventRecord(ev_[2], st));
    hipLaunchKernelGGL(k_lgcn_update, dim3(grid_of(rows * k)), dim3(kLgcnThreads), 0, st, W0_.get(), DW_.get(), bpr_.cntW_.get(),
                       graph_.user_.s.get(), rows, k, graph_.layers_, lr, lambda);
    MFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_lgcn_update, dim3(grid_of(cols * k)), dim3(kLgcnThreads), 0, st, H0_.get(), DH_.get(), bpr_.cntH_.get(),
                       graph_.item_.s.get(), cols, k, graph_.layers_, lr, lambda);
    MFX_LAUNCH_CHECK();
    // (a row's count is read by all the threads of the row, in more than one workgroup at large k: it is cleared after the kernel)
    MFX_HIP(hipMemsetAsync(bpr_.cntW_.get(), 0, sizeof(uint32_t) * rows, st));
    MFX_HIP(hipMemsetAsync(bpr_.cntH_.get(), 0, sizeof(uint32_t) * cols, st));
    if (profile_) {
        MFX_HIP(hipEventRecord(ev_[3], st));
        MFX_HIP(hipEventSynchronize(ev_[3]));
        const hipEvent_t seq[7] = {ev_[0], ev_[1], bpr_.ev_[1], bpr_.ev_[2], bpr_.ev_[3], ev_[2], ev_[3]};
        for (int p = 0; p < 6; ++p) {
            float ms = 0.f;
            MFX_HIP(hipEventElapsedTime(&ms, seq[p], seq[p + 1]));
            phase_s_[p] += 1e-3 * ms;
        }
    }
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the solver
int LgcnSolver::create(LgcnSolver** out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, int32_t layers, uint64_t seed,
                       mfx_memspace space) {
    const char* fn = "mfx_lgcn_create";
    MFX_REQUIRE(out && R && p, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_sizes(fn, (int64_t) p->k, layers, lr, p->lambda));
    MFX_REQUIRE(batch >= 1 && batch <= kLgcnMaxBatch, "%s: batch must be in [1, 2^20] (got %lld)", fn, (long long) batch);
    MFX_TRY(check_matrix(fn, R));
    std::unique_ptr<LgcnSolver> s(new LgcnSolver());
    s->lr_ = lr; s->lambda_ = p->lambda; s->seed_ = seed;
    MFX_TRY(s->core_.init(fn, R, space, p->k, std::min<int64_t>(batch, R->nnz), layers, p->device));
    s->core_.bpr_.batch_ = batch;  // (a step never has more than nnz slots: the slot arrays are sized for min(batch, nnz))
    s->core_.profile_ = p->profile != 0;
    *out = s.release();
    return MFX_OK;
}

int LgcnSolver::set_base(const float* W0, const float* H0, mfx_memspace space) {
    MFX_REQUIRE(W0 && H0, "mfx_lgcn_set_base: W0 or H0 is NULL");
    MFX_TRY(check_space("mfx_lgcn_set_base", space));
    MFX_TRY(core_.set_base(W0, H0, space));
    have_base_ = true;
    return MFX_OK;
}

int LgcnSolver::get_base(float* W0, float* H0, mfx_memspace space) {
    MFX_REQUIRE(have_base_, "mfx_lgcn_get_base: no base embeddings were set");
    MFX_TRY(check_space("mfx_lgcn_get_base", space));
    return core_.get_base(W0, H0, space);
}

int LgcnSolver::get_factors(float* W, float* H, mfx_memspace space) {
    MFX_REQUIRE(have_base_, "mfx_lgcn_get_factors: no base embeddings were set");
    MFX_TRY(check_space("mfx_lgcn_get_factors", space));
    MFX_TRY(use_device(core_.bpr_.device_));
    MFX_TRY(core_.forward());
    return core_.bpr_.download(W, H, space);
}

void LgcnSolver::times(double seconds[6]) const {
    for (int p = 0; p < 6; ++p) seconds[p] = core_.phase_s_[p];
}

// n_steps steps from the current slot, or (to_epoch_end) the steps up to the end of the epoch that holds it.
int LgcnSolver::run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds) {
    BprCore& b = core_.bpr_;
    MFX_TRY(use_device(b.device_));
    hipStream_t st = b.st_;
    MFX_HIP(hipMemsetAsync(b.stats_.get(), 0, 4 * sizeof(unsigned long long), st));
    hipEvent_t t0 = b.ev_[5], t1 = b.ev_[6];
    MFX_HIP(hipEventRecord(t0, st));
    const uint64_t s0 = bpr_stream(seed_), nnz = (uint64_t) core_.graph_.nnz_;
    int64_t slots = 0;
    for (int64_t s = 0; to_epoch_end || s < n_steps; ++s) {
        const uint32_t n = (uint32_t) std::min<uint64_t>((uint64_t) b.batch_, nnz - pos_ % nnz);
        if (core_.profile_) MFX_HIP(hipEventRecord(core_.ev_[0], st));
        MFX_TRY(b.sample(s0, pos_, n, core_.graph_.user_.ptr.get(), core_.graph_.user_.idx.get(), (uint32_t) nnz));
        MFX_TRY(core_.step(n, lr_, lambda_));
        pos_ += n;
        slots += n;
        if (to_epoch_end && pos_ % nnz == 0) break;
    }
    MFX_HIP(hipEventRecord(t1, st));
    unsigned long long h[4] = {0, 0, 0, 0};
    MFX_HIP(hipMemcpyAsync(h, b.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    MFX_HIP(hipEventElapsedTime(&ms, t0, t1));
    if (seconds) *seconds = 1e-3 * ms;
    if (stats) {
        stats[0] = slots;
        for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    }
    return MFX_OK;
}

int LgcnSolver::steps(int64_t n_steps, int64_t stats[4], double* seconds) {
    MFX_REQUIRE(n_steps >= 0, "mfx_lgcn_steps: n_steps must not be negative (got %lld)", (long long) n_steps);
    MFX_REQUIRE(have_base_, "mfx_lgcn_steps: no base embeddings were set (mfx_lgcn_set_base)");
    return run(n_steps, false, stats, seconds);
}

int LgcnSolver::epochs(int32_t n_epochs, int64_t* stats, double* seconds) {
    MFX_REQUIRE(n_epochs >= 0, "mfx_lgcn_epochs: n_epochs must not be negative (got %d)", n_epochs);
    MFX_REQUIRE(have_base_, "mfx_lgcn_epochs: no base embeddings were set (mfx_lgcn_set_base)");
    for (int32_t e = 0; e < n_epochs; ++e) MFX_TRY(run(0, true, stats ? stats + 4 * e : nullptr, seconds ? seconds + e : nullptr));
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the single operators
int lgcn_propagate(const mfx_csx* R, const float* W0, const float* H0, int64_t k, int32_t layers, float* W, float* H, int device) {
    const char* fn = "mfx_lgcn_propagate";
    MFX_REQUIRE(R && W0 && H0 && W && H, "%s: null argument", fn);
    MFX_TRY(check_sizes(fn, k, layers, 0.f, 0.f));
    MFX_TRY(check_matrix(fn, R));
    MFX_TRY(use_device(device));
    LgcnGraph g;
    MFX_TRY(g.init(fn, R, MFX_HOST, k, layers, device, nullptr));
    const size_t nw = (size_t) R->rows * k, nh = (size_t) R->cols * k;
    DevBuf<float> w0, h0, w, h;
    MFX_TRY(w0.alloc(nw));
    MFX_TRY(h0.alloc(nh));
    MFX_TRY(w.alloc(nw));
    MFX_TRY(h.alloc(nh));
    MFX_TRY(w0.upload(W0, nw, MFX_HOST, g.st_));
    MFX_TRY(h0.upload(H0, nh, MFX_HOST, g.st_));
    MFX_TRY(g.propagate(w0.get(), h0.get(), w.get(), h.get()));
    MFX_HIP(hipMemcpyAsync(W, w.get(), sizeof(float) * nw, hipMemcpyDeviceToHost, g.st_));
    MFX_HIP(hipMemcpyAsync(H, h.get(), sizeof(float) * nh, hipMemcpyDeviceToHost, g.st_));
    MFX_HIP(hipStreamSynchronize(g.st_));
    return MFX_OK;
}

int lgcn_apply(const mfx_csx* R, int64_t k, float* W0, float* H0, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
               const uint8_t* skipped, int32_t layers, float lr, float lambda, int64_t stats[4], int device) {
    const char* fn = "mfx_lgcn_apply";
    MFX_REQUIRE(R && W0 && H0 && stats, "%s: R, W0, H0 or stats is NULL", fn);
    MFX_TRY(check_sizes(fn, k, layers, lr, lambda));
    MFX_REQUIRE(n >= 0 && n <= kLgcnMaxBatch, "%s: n must be in [0, 2^20] (got %lld)", fn, (long long) n);
    MFX_TRY(check_matrix(fn, R));
    MFX_REQUIRE(n == 0 || (u && i && j), "%s: u, i or j is NULL", fn);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return MFX_OK;
    LgcnCore core;
    MFX_TRY(core.init(fn, R, MFX_HOST, k, n, layers, device));
    hipStream_t st = core.bpr_.st_;
    MFX_TRY(core.bpr_.set_slots(fn, n, u, i, j, skipped));
    MFX_TRY(core.set_base(W0, H0, MFX_HOST));
    MFX_TRY(core.step((uint32_t) n, lr, lambda));
    unsigned long long h[4] = {0, 0, 0, 0};
    MFX_HIP(hipMemcpyAsync(h, core.bpr_.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    MFX_TRY(core.get_base(W0, H0, MFX_HOST));
    stats[0] = n;
    for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    return MFX_OK;
}

}  // namespace mfx
