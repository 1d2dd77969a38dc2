// hybrid.hip -- hybrid BPR (mfx_hyb_*) on gfx950: the pairwise step of bpr.hip on rows whose vectors are the weighted sums
// of the embeddings of their features, so that a row without interactions still has a vector (LightFM's model without
// biases).  The contract -- the embedding chain, the rounding of a row's sums to G, the second level of fixed-point sums and
// the update of a feature -- is in include/mfx.h ("Hybrid BPR"); DESIGN 5.23 has the choices and the measurements.
//
// A step runs on one stream, no kernel over rows + cols or over the features:
//   k_hyb_embed    gs lanes per (slot, role), lanes across coordinates: the FMA chain of the row's entries in stored order
//                  into the BprCore's W_ / H_ (scratch here).  The group loads gs ids and values at a time, one per lane,
//                  hands them round and keeps 8 embedding-row loads in flight ahead of the chain (k_lgcn_propagate's
//                  pattern).  Slots that share a row write the same bits.  The same kernel over every row of a side is the
//                  materialisation behind get_factors and mfx_hyb_embed.
//   gradient + scatter   BprCore::grad_scatter: k_bpr_grad and k_bpr_scatter of bpr.hip as they are, on the embedded rows.
//   k_hyb_spread   gs lanes per (slot, role), in the place of k_bpr_apply: the group whose slot holds the row's claim rounds
//                  the row's sums to G (registers), puts the row's accumulators, count and claim back to rest and adds
//                  fp32(v * G[c]) as 64-bit integers into the accumulator row of every feature of the row -- 8-byte adds
//                  that are contiguous across the lanes of a group, the shape of k_bpr_scatter.  The lane that loaded an
//                  entry adds m_r to its feature's count and bids for the feature with atomicMin(claim[f], 3 t + role).
//   k_hyb_apply    gs lanes per (slot, role): walks the row's entries again; where a feature's claim word holds the group's
//                  own key it rounds the feature's sums once, updates the feature and puts its state back to rest.
// Integer adds commute exactly, and a coordinate's chain is one lane's: no bit depends on gs, the grid, the loads in flight
// or the order of arrival.
#include <algorithm>
#include <cmath>
#include <memory>
#include <numeric>

#include "hybrid.hpp"
#include "bpr_device.hpp"

#ifndef MFX_LAUNCH_CHECK
#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())
#endif

namespace mfx {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kHybMaxBatch = 1 << 20;
constexpr uint32_t kHybMaxEntries = 1024;  // entries of a row of a feature matrix (include/mfx.h: part of the contract)
constexpr int kHybThreads = 256;
constexpr int kHybInFlight = 8;            // embedding-row loads of a lane ahead of its chain
constexpr uint32_t kHybMaxGrid = 4096;     // workgroups of a launch: 16 per CU; the groups walk the work beyond

inline uint32_t grid_of(uint64_t threads) { return (uint32_t) ((threads + kHybThreads - 1) / kHybThreads); }

// fp32 -> 64-bit fixed point (two's complement), scale 2^36, truncated toward zero, for |x| < 2^27: the product is exact in
// double (24 significant bits and an exponent) and below 2^63.
__device__ __forceinline__ unsigned long long to_fixed27(float x) {
    return (unsigned long long) (long long) ((double) x * 68719476736.0);
}

// ---------------------------------------------------------------------------------------------- kernels
// Row r of a feature matrix: its pointers inside [0, nnz] and in order, at most 1024 entries, its ids strictly ascending and
// below nf, its values finite with |v| <= 1.
__global__ void k_hyb_check(const uint32_t* ptr, const uint32_t* idx, const float* val, uint32_t n, uint32_t nf, uint32_t nnz,
                            uint32_t* first_bad) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t lo = ptr[r], hi = ptr[r + 1];
        bool bad = lo > hi || hi > nnz || (r == 0 && lo != 0) || (r + 1 == n && hi != nnz);
        if (!bad) bad = hi - lo > kHybMaxEntries;
        if (!bad) {
            uint32_t prev = 0;
            for (uint32_t e = lo; e < hi; ++e) {
                const uint32_t f = idx[e];
                if (f >= nf || (e > lo && f <= prev) || !(fabsf(val[e]) <= 1.f)) { bad = true; break; }  // (a NaN is not <= 1)
                prev = f;
            }
        }
        if (bad) atomicMin(first_bad, (uint32_t) r);
    }
}

struct HybSideArgs {
    const uint32_t* ptr;       // [n + 1]
    const uint32_t* idx;       // [nnz]
    const float* val;          // [nnz]
    float* E;                  // [nf][k]
    unsigned long long* acc;   // [nf][k]
    uint32_t* cnt;             // [nf]
    uint32_t* claim;           // [nf]
    float* X;                  // [n][k] the embedded rows (the BprCore's factors)
    unsigned long long* accX;  // [n][k] the BprCore's accumulators, counts and claims of the rows
    uint32_t* cntX;
    uint32_t* claimX;
};

struct HybArgs {
    HybSideArgs user, item;
    const uint32_t* u;       // [n] the slots
    const uint32_t* i;
    const uint32_t* j;
    const uint8_t* skipped;  // [n]
    const uint8_t* state;    // [n]
    uint64_t n_work;         // 3 n (slot, role) pairs, or (full != 0) the rows of a side
    int k, gs, gsh;          // gs = 1 << gsh lanes share a work item
    int full;                // k_hyb_embed: 0 = the rows of the slots; 1 = every user row, 2 = every item row
    float lr, lambda;
};

// NC coordinates per lane and turn of the coordinate loop.
template <int NC>
__global__ __launch_bounds__(kHybThreads) void k_hyb_embed(HybArgs a) {
    const int gs = a.gs, k = a.k;
    const uint32_t cl = threadIdx.x & (uint32_t) (gs - 1);
    const uint32_t group = (blockIdx.x * (uint32_t) kHybThreads + threadIdx.x) >> a.gsh;
    const uint32_t n_groups = (gridDim.x * (uint32_t) kHybThreads) >> a.gsh;
    for (uint64_t w = group; w < a.n_work; w += n_groups) {  // the walk through the (slot, role) pairs or the rows
        bool item_side;
        uint32_t row;
        if (a.full) {
            item_side = a.full == 2;
            row = (uint32_t) w;
        } else {
            const uint32_t t = (uint32_t) (w / 3);
            const int role = (int) (w - (uint64_t) t * 3);
            if (a.skipped[t]) continue;  // (k_bpr_grad reads no row of a skipped slot)
            item_side = role != 0;
            row = role == 0 ? a.u[t] : role == 1 ? a.i[t] : a.j[t];
        }
        const uint32_t* ptr = item_side ? a.item.ptr : a.user.ptr;
        const uint32_t* idx = item_side ? a.item.idx : a.user.idx;
        const float* val = item_side ? a.item.val : a.user.val;
        const float* E = item_side ? a.item.E : a.user.E;
        float* out = (item_side ? a.item.X : a.user.X) + (size_t) row * k;
        const uint32_t lo = ptr[row], hi = ptr[row + 1];
        for (int c0 = 0; c0 < k; c0 += gs * NC) {  // the coordinate loop
            float acc[NC];
            size_t off[NC];
            bool on[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int c = c0 + q * gs + (int) cl;
                // fmaf(v, x, -0) is fp32(v * x) in every bit, the sign of a zero product included: the chain starts from the
                // first product
                acc[q] = -0.f;
                on[q] = c < k;
                off[q] = (size_t) (on[q] ? c : 0);
            }
            for (uint32_t e0 = lo; e0 < hi; e0 += (uint32_t) gs) {  // gs entries at a time
                const uint32_t cnt = min((uint32_t) gs, hi - e0);
                uint32_t my_id = 0, my_v = 0;
                if (cl < cnt) {
                    my_id = idx[e0 + cl];
                    my_v = __float_as_uint(val[e0 + cl]);
                }
                for (uint32_t b0 = 0; b0 < cnt; b0 += kHybInFlight) {  // the loads in flight
                    float x[kHybInFlight][NC], sv[kHybInFlight];
#pragma unroll
                    for (int b = 0; b < kHybInFlight; ++b) {
                        const int lane = (int) ((b0 + b) & (uint32_t) (gs - 1));
                        const uint32_t id = (uint32_t) __shfl((int) my_id, lane, gs);
                        sv[b] = __uint_as_float((uint32_t) __shfl((int) my_v, lane, gs));
                        const float* erow = E + (size_t) id * k;
#pragma unroll
                        for (int q = 0; q < NC; ++q) x[b][q] = (b0 + b < cnt && on[q]) ? erow[off[q]] : 0.f;
                    }
#pragma unroll
                    for (int b = 0; b < kHybInFlight; ++b) {
                        if (b0 + b < cnt) {
#pragma unroll
                            for (int q = 0; q < NC; ++q) acc[q] = __builtin_fmaf(sv[b], x[b][q], acc[q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (on[q]) out[off[q]] = hi == lo ? 0.f : acc[q];  // (an empty row gives +0)
        }
    }
}

template <int NC>
__global__ __launch_bounds__(kHybThreads) void k_hyb_spread(HybArgs a) {
    const int gs = a.gs, k = a.k;
    const uint32_t cl = threadIdx.x & (uint32_t) (gs - 1);
    const uint32_t group = (blockIdx.x * (uint32_t) kHybThreads + threadIdx.x) >> a.gsh;
    const uint32_t n_groups = (gridDim.x * (uint32_t) kHybThreads) >> a.gsh;
    for (uint64_t w = group; w < a.n_work; w += n_groups) {  // the walk through the (slot, role) pairs
        const uint32_t t = (uint32_t) (w / 3);
        const int role = (int) (w - (uint64_t) t * 3);
        if (a.state[t] != kCounted) continue;
        if (role == 2 && a.j[t] == a.i[t]) continue;  // (the row was this slot's as the positive item already)
        const bool item_side = role != 0;
        const uint32_t row = role == 0 ? a.u[t] : role == 1 ? a.i[t] : a.j[t];
        uint32_t* claim = (item_side ? a.item.claimX : a.user.claimX) + row;
        if (*claim != t) continue;  // (another slot's row; it may be back at rest by now, which is no slot number either)
        uint32_t* cntp = (item_side ? a.item.cntX : a.user.cntX) + row;
        const uint32_t m = *cntp;
        const uint32_t key = (uint32_t) w;  // 3 t + role
        const uint32_t* ptr = item_side ? a.item.ptr : a.user.ptr;
        const uint32_t* idx = item_side ? a.item.idx : a.user.idx;
        const float* val = item_side ? a.item.val : a.user.val;
        unsigned long long* accE = item_side ? a.item.acc : a.user.acc;
        uint32_t* cntE = item_side ? a.item.cnt : a.user.cnt;
        uint32_t* claimE = item_side ? a.item.claim : a.user.claim;
        unsigned long long* accr = (item_side ? a.item.accX : a.user.accX) + (size_t) row * k;
        const uint32_t lo = ptr[row], hi = ptr[row + 1];
        for (int c0 = 0; c0 < k; c0 += gs * NC) {  // the coordinate loop
            float G[NC];
            size_t off[NC];
            bool on[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const int c = c0 + q * gs + (int) cl;
                on[q] = c < k;
                off[q] = (size_t) (on[q] ? c : 0);
                G[q] = 0.f;
                if (on[q]) {
                    G[q] = mul_rn((float) (long long) accr[off[q]], 1.4551915228366852e-11f);  // one rounding int64 -> fp32, then the exact 2^-36
                    accr[off[q]] = 0ull;
                }
            }
            for (uint32_t e0 = lo; e0 < hi; e0 += (uint32_t) gs) {  // gs entries at a time
                const uint32_t cnt = min((uint32_t) gs, hi - e0);
                uint32_t my_id = 0, my_v = 0;
                if (cl < cnt) {
                    my_id = idx[e0 + cl];
                    my_v = __float_as_uint(val[e0 + cl]);
                    if (c0 == 0) {  // the lane that loaded the entry counts the row on its feature and bids for it
                        atomicAdd(cntE + my_id, m);
                        atomicMin(claimE + my_id, key);
                    }
                }
                for (uint32_t b = 0; b < cnt; ++b) {
                    const uint32_t id = (uint32_t) __shfl((int) my_id, (int) b, gs);
                    const float v = __uint_as_float((uint32_t) __shfl((int) my_v, (int) b, gs));
                    unsigned long long* dst = accE + (size_t) id * k;
#pragma unroll
                    for (int q = 0; q < NC; ++q)
                        if (on[q]) atomicAdd(dst + off[q], to_fixed27(mul_rn(v, G[q])));
                }
            }
        }
        // (every lane of the group has read *claim and *cntp above: a group lies inside one wave, whose lanes pass a load together)
        if (cl == 0) {
            *cntp = 0u;
            *claim = kNone;
        }
    }
}

__global__ __launch_bounds__(kHybThreads) void k_hyb_apply(HybArgs a) {
    const int gs = a.gs, k = a.k;
    const uint32_t cl = threadIdx.x & (uint32_t) (gs - 1);
    const uint32_t group = (blockIdx.x * (uint32_t) kHybThreads + threadIdx.x) >> a.gsh;
    const uint32_t n_groups = (gridDim.x * (uint32_t) kHybThreads) >> a.gsh;
    for (uint64_t w = group; w < a.n_work; w += n_groups) {  // the walk through the (slot, role) pairs
        const uint32_t t = (uint32_t) (w / 3);
        const int role = (int) (w - (uint64_t) t * 3);
        if (a.state[t] != kCounted) continue;
        if (role == 2 && a.j[t] == a.i[t]) continue;
        const bool item_side = role != 0;
        const uint32_t row = role == 0 ? a.u[t] : role == 1 ? a.i[t] : a.j[t];
        const uint32_t key = (uint32_t) w;  // 3 t + role
        const uint32_t* ptr = item_side ? a.item.ptr : a.user.ptr;
        const uint32_t* idx = item_side ? a.item.idx : a.user.idx;
        float* E = item_side ? a.item.E : a.user.E;
        unsigned long long* accE = item_side ? a.item.acc : a.user.acc;
        uint32_t* cntE = item_side ? a.item.cnt : a.user.cnt;
        uint32_t* claimE = item_side ? a.item.claim : a.user.claim;
        const uint32_t lo = ptr[row], hi = ptr[row + 1];
        for (uint32_t e0 = lo; e0 < hi; e0 += (uint32_t) gs) {  // gs entries at a time
            const uint32_t cnt = min((uint32_t) gs, hi - e0);
            uint32_t my_id = 0;
            int mine = 0;
            if (cl < cnt) {
                my_id = idx[e0 + cl];
                mine = claimE[my_id] == key;  // (only the group that spread the row can find its key)
            }
            for (uint32_t b = 0; b < cnt; ++b) {
                if (!__shfl(mine, (int) b, gs)) continue;
                const uint32_t f = (uint32_t) __shfl((int) my_id, (int) b, gs);
                const float reg = mul_rn(a.lambda, (float) cntE[f]);
                float* X = E + (size_t) f * k;
                unsigned long long* acc = accE + (size_t) f * k;
                for (int c = (int) cl; c < k; c += gs) {
                    const float s = mul_rn((float) (long long) acc[c], 1.4551915228366852e-11f);
                    const float old = X[c];
                    X[c] = add_rn(old, mul_rn(a.lr, sub_rn(s, mul_rn(reg, old))));
                    acc[c] = 0ull;
                }
                // (every lane of the group has read cntE[f] above, in one load of the wave)
                if (cl == 0) {
                    cntE[f] = 0u;
                    claimE[f] = kNone;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- host helpers
int check_space(const char* fn, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    return MFX_OK;
}

int check_sizes(const char* fn, int64_t k, float lr, float lambda) {
    MFX_REQUIRE(k >= 1 && k <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k);
    MFX_REQUIRE(std::isfinite(lr) && lr >= 0.f, "%s: lr must be finite and >= 0 (got %g)", fn, (double) lr);
    MFX_REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "%s: lambda must be finite and >= 0 (got %g)", fn, (double) lambda);
    return MFX_OK;
}

// What can be said of a feature matrix without touching the device.  n < 0: any number of rows.
int check_features(const char* fn, const char* what, const mfx_features* F, int64_t n) {
    if (!F) return MFX_OK;  // (the identity)
    MFX_REQUIRE(n < 0 || F->n == n, "%s: the %s features have %lld rows, the matrix has %lld", fn, what, (long long) F->n, (long long) n);
    MFX_REQUIRE(F->n >= 0 && F->n < 0xFFFFFFFFll, "%s: the rows of the %s features must be below 2^32 - 1", fn, what);
    MFX_REQUIRE(F->nf >= 1 && F->nf < 0xFFFFFFFFll, "%s: nf of the %s features must be in [1, 2^32 - 1) (got %lld)", fn, what, (long long) F->nf);
    MFX_REQUIRE(F->ptr, "%s: ptr of the %s features is NULL", fn, what);
    return MFX_OK;
}

int gs_of(int64_t k) {
    int gs = 1;
    while (gs < 64 && gs < k) gs *= 2;
    return gs;
}

HybSideArgs side_args(const HybSide& s, float* X, unsigned long long* accX, uint32_t* cntX, uint32_t* claimX) {
    HybSideArgs a{};
    a.ptr = s.ptr.get(); a.idx = s.idx.get(); a.val = s.val.get();
    a.E = s.E.get(); a.acc = s.acc.get(); a.cnt = s.cnt.get(); a.claim = s.claim.get();
    a.X = X; a.accX = accX; a.cntX = cntX; a.claimX = claimX;
    return a;
}

dim3 grid_for(uint64_t n_work, int gs) { return dim3(std::min<uint32_t>(grid_of(n_work * (uint64_t) gs), kHybMaxGrid)); }

int launch_embed(const HybArgs& a, hipStream_t st) {
    if (a.n_work == 0) return MFX_OK;
    const dim3 grid = grid_for(a.n_work, a.gs), block(kHybThreads);
    if (a.k <= 64) hipLaunchKernelGGL((k_hyb_embed<1>), grid, block, 0, st, a);
    else if (a.k <= 128) hipLaunchKernelGGL((k_hyb_embed<2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_hyb_embed<4>), grid, block, 0, st, a);
    MFX_LAUNCH_CHECK();
    return MFX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- one side
int HybSide::init(const char* fn, const char* what, const mfx_features* F, int64_t rows, mfx_memspace space, hipStream_t st) {
    n = rows;
    MFX_TRY(ptr.alloc((size_t) n + 1));
    if (!F) {  // the identity: feature r on row r with the value 1, through the code path of a given matrix
        nf = n; nnz = n;
        std::vector<uint32_t> p((size_t) n + 1);
        std::iota(p.begin(), p.end(), 0u);
        const std::vector<float> ones((size_t) n, 1.f);
        MFX_TRY(idx.alloc((size_t) n));
        MFX_TRY(val.alloc((size_t) n));
        MFX_TRY(ptr.upload(p.data(), (size_t) n + 1, MFX_HOST, st));
        MFX_TRY(idx.upload(p.data(), (size_t) n, MFX_HOST, st));
        MFX_TRY(val.upload(ones.data(), (size_t) n, MFX_HOST, st));
        MFX_HIP(hipStreamSynchronize(st));  // (the host vectors end here)
        return MFX_OK;
    }
    nf = F->nf;
    MFX_TRY(ptr.upload(F->ptr, (size_t) n + 1, space, st));
    uint32_t last = 0;
    MFX_HIP(hipMemcpyAsync(&last, ptr.get() + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    nnz = last;
    MFX_REQUIRE(nnz == 0 || (F->idx && F->val), "%s: idx or val of the %s features is NULL", fn, what);
    MFX_TRY(idx.alloc((size_t) nnz));
    MFX_TRY(val.alloc((size_t) nnz));
    MFX_TRY(idx.upload(F->idx, (size_t) nnz, space, st));
    MFX_TRY(val.upload(F->val, (size_t) nnz, space, st));
    if (n == 0) return MFX_OK;
    DevBuf<uint32_t> bad;
    MFX_TRY(bad.alloc(1));
    MFX_HIP(hipMemsetAsync(bad.get(), 0xFF, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_hyb_check, dim3(std::min<uint32_t>(grid_of((uint64_t) n), 65536u)), dim3(kHybThreads), 0, st, ptr.get(), idx.get(),
                       val.get(), (uint32_t) n, (uint32_t) nf, (uint32_t) nnz, bad.get());
    MFX_LAUNCH_CHECK();
    uint32_t first_bad = kNone;
    MFX_HIP(hipMemcpyAsync(&first_bad, bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_REQUIRE(first_bad == kNone,
                "%s: row %u of the %s features: its pointers must ascend from 0 to the number of entries, it may hold at most 1024 entries, "
                "its ids must be strictly ascending and below nf, its values finite with |v| <= 1",
                fn, first_bad, what);
    return MFX_OK;
}

int HybSide::alloc_state(int64_t k, hipStream_t st) {
    const size_t ne = (size_t) nf * k;
    MFX_TRY(E.alloc(ne));
    MFX_TRY(acc.alloc_zero(ne, st));
    MFX_TRY(cnt.alloc_zero((size_t) nf, st));
    MFX_TRY(claim.alloc((size_t) nf));
    MFX_HIP(hipMemsetAsync(claim.get(), 0xFF, sizeof(uint32_t) * (size_t) nf, st));
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- one step
HybCore::~HybCore() {
    for (auto e : ev_)
        if (e) (void) hipEventDestroy(e);
}

int HybCore::init(const char* fn, int64_t rows, int64_t cols, int64_t k, int64_t batch, const mfx_features* Fu, const mfx_features* Fi,
                  mfx_memspace space, int device) {
    MFX_TRY(bpr_.init(rows, cols, k, batch, device));
    hipStream_t st = bpr_.st_;
    MFX_TRY(user_.init(fn, "user", Fu, rows, space, st));
    MFX_TRY(item_.init(fn, "item", Fi, cols, space, st));
    MFX_TRY(user_.alloc_state(k, st));
    MFX_TRY(item_.alloc_state(k, st));
    for (auto& e : ev_) MFX_HIP(hipEventCreate(&e));
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int HybCore::set_tables(const float* Eu, const float* Ei, mfx_memspace space) {
    MFX_TRY(use_device(bpr_.device_));
    MFX_TRY(user_.E.upload(Eu, (size_t) user_.nf * bpr_.k_, space, bpr_.st_));
    MFX_TRY(item_.E.upload(Ei, (size_t) item_.nf * bpr_.k_, space, bpr_.st_));
    MFX_HIP(hipStreamSynchronize(bpr_.st_));
    return MFX_OK;
}

int HybCore::get_tables(float* Eu, float* Ei, mfx_memspace space) {
    MFX_TRY(use_device(bpr_.device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (Eu) MFX_HIP(hipMemcpyAsync(Eu, user_.E.get(), sizeof(float) * user_.nf * bpr_.k_, kind, bpr_.st_));
    if (Ei) MFX_HIP(hipMemcpyAsync(Ei, item_.E.get(), sizeof(float) * item_.nf * bpr_.k_, kind, bpr_.st_));
    MFX_HIP(hipStreamSynchronize(bpr_.st_));
    return MFX_OK;
}

namespace {
HybArgs args_of(const HybCore& c, uint32_t n, float lr, float lambda) {
    const BprCore& b = c.bpr_;
    HybArgs a{};
    a.user = side_args(c.user_, b.W_.get(), b.accW_.get(), b.cntW_.get(), b.claimW_.get());
    a.item = side_args(c.item_, b.H_.get(), b.accH_.get(), b.cntH_.get(), b.claimH_.get());
    a.u = b.u_.get(); a.i = b.i_.get(); a.j = b.j_.get();
    a.skipped = b.skip_.get(); a.state = b.state_.get();
    a.n_work = (uint64_t) n * 3;
    a.k = (int) b.k_; a.gs = b.gs_; a.gsh = __builtin_ctz((unsigned) b.gs_);
    a.full = 0;
    a.lr = lr; a.lambda = lambda;
    return a;
}
}  // namespace

int HybCore::materialise(bool users, bool items) {
    HybArgs a = args_of(*this, 0, 0.f, 0.f);
    a.full = 1; a.n_work = (uint64_t) bpr_.rows_;
    if (users) MFX_TRY(launch_embed(a, bpr_.st_));
    a.full = 2; a.n_work = (uint64_t) bpr_.cols_;
    if (items) MFX_TRY(launch_embed(a, bpr_.st_));
    return MFX_OK;
}

int HybCore::step(uint32_t n, float lr, float lambda) {
    if (n == 0) return MFX_OK;
    hipStream_t st = bpr_.st_;
    bpr_.profile_ = profile_;
    const HybArgs a = args_of(*this, n, lr, lambda);
    if (profile_) MFX_HIP(hipEventRecord(ev_[1], st));
    MFX_TRY(launch_embed(a, st));
    MFX_TRY(bpr_.grad_scatter(n));
    const dim3 grid = grid_for(a.n_work, a.gs), block(kHybThreads);
    if (a.k <= 64) hipLaunchKernelGGL((k_hyb_spread<1>), grid, block, 0, st, a);
    else if (a.k <= 128) hipLaunchKernelGGL((k_hyb_spread<2>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_hyb_spread<4>), grid, block, 0, st, a);
    MFX_LAUNCH_CHECK();
    if (profile_) MFX_HIP(hipEventRecord(ev_[2], st));
    hipLaunchKernelGGL(k_hyb_apply, grid, block, 0, st, a);
    MFX_LAUNCH_CHECK();
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
int HybSolver::create(HybSolver** out, const mfx_csx* R, const mfx_features* Fu, const mfx_features* Fi, const mfx_params* p, float lr,
                      int64_t batch, uint64_t seed, mfx_memspace space) {
    const char* fn = "mfx_hyb_create";
    MFX_REQUIRE(out && R && p, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(check_sizes(fn, (int64_t) p->k, lr, p->lambda));
    MFX_REQUIRE(batch >= 1 && batch <= kHybMaxBatch, "%s: batch must be in [1, 2^20] (got %lld)", fn, (long long) batch);
    MFX_REQUIRE(R->nnz >= 1, "%s: the matrix has no entries", fn);
    MFX_REQUIRE(R->cols >= 2, "%s: cols must be at least 2 (got %lld)", fn, (long long) R->cols);
    MFX_REQUIRE(R->rows >= 1 && R->rows < 0xFFFFFFFFll && R->cols < 0xFFFFFFFFll && R->nnz < 0xFFFFFFFFll,
                "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    MFX_REQUIRE(R->csr_row_ptr && R->csr_col_idx, "%s: the CSR side of R is NULL", fn);
    MFX_TRY(check_features(fn, "user", Fu, R->rows));
    MFX_TRY(check_features(fn, "item", Fi, R->cols));
    std::unique_ptr<HybSolver> s(new HybSolver());
    s->nnz_ = R->nnz; s->lr_ = lr; s->lambda_ = p->lambda; s->seed_ = seed;
    MFX_TRY(s->core_.init(fn, R->rows, R->cols, p->k, std::min<int64_t>(batch, R->nnz), Fu, Fi, space, p->device));
    s->core_.bpr_.batch_ = batch;  // (a step never has more than nnz slots: the slot arrays are sized for min(batch, nnz))
    s->core_.profile_ = p->profile != 0;
    hipStream_t st = s->core_.bpr_.st_;
    const uint32_t rows = (uint32_t) R->rows;
    MFX_TRY(s->ptr_.alloc((size_t) rows + 1));
    MFX_TRY(s->idx_.alloc((size_t) R->nnz));
    MFX_TRY(s->ptr_.upload(R->csr_row_ptr, (size_t) rows + 1, space, st));
    MFX_TRY(s->idx_.upload(R->csr_col_idx, (size_t) R->nnz, space, st));
    uint32_t first_bad = kNone;
    MFX_TRY(bpr_check_rows(s->ptr_.get(), s->idx_.get(), rows, (uint32_t) R->cols, (uint32_t) R->nnz, st, &first_bad));
    MFX_REQUIRE(first_bad == kNone,
                "%s: row %u of the CSR side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols", fn,
                first_bad);
    *out = s.release();
    return MFX_OK;
}

int HybSolver::set_embeddings(const float* Eu, const float* Ei, mfx_memspace space) {
    MFX_REQUIRE(Eu && Ei, "mfx_hyb_set_embeddings: Eu or Ei is NULL");
    MFX_TRY(check_space("mfx_hyb_set_embeddings", space));
    MFX_TRY(core_.set_tables(Eu, Ei, space));
    have_tables_ = true;
    return MFX_OK;
}

int HybSolver::get_embeddings(float* Eu, float* Ei, mfx_memspace space) {
    MFX_REQUIRE(have_tables_, "mfx_hyb_get_embeddings: no embeddings were set");
    MFX_TRY(check_space("mfx_hyb_get_embeddings", space));
    return core_.get_tables(Eu, Ei, space);
}

int HybSolver::get_factors(float* W, float* H, mfx_memspace space) {
    MFX_REQUIRE(have_tables_, "mfx_hyb_get_factors: no embeddings were set");
    MFX_TRY(check_space("mfx_hyb_get_factors", space));
    MFX_TRY(use_device(core_.bpr_.device_));
    MFX_TRY(core_.materialise(W != nullptr, H != nullptr));  // (a side that is not asked for is not embedded)
    return core_.bpr_.download(W, H, space);
}

void HybSolver::times(double seconds[6]) const {
    for (int p = 0; p < 6; ++p) seconds[p] = core_.phase_s_[p];
}

// n_steps steps from the current slot, or (to_epoch_end) the steps up to the end of the epoch that holds it.
int HybSolver::run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds) {
    BprCore& b = core_.bpr_;
    MFX_TRY(use_device(b.device_));
    hipStream_t st = b.st_;
    MFX_HIP(hipMemsetAsync(b.stats_.get(), 0, 4 * sizeof(unsigned long long), st));
    hipEvent_t t0 = b.ev_[5], t1 = b.ev_[6];
    MFX_HIP(hipEventRecord(t0, st));
    const uint64_t s0 = bpr_stream(seed_), nnz = (uint64_t) nnz_;
    int64_t slots = 0;
    for (int64_t s = 0; to_epoch_end || s < n_steps; ++s) {
        const uint32_t n = (uint32_t) std::min<uint64_t>((uint64_t) b.batch_, nnz - pos_ % nnz);
        if (core_.profile_) MFX_HIP(hipEventRecord(core_.ev_[0], st));
        MFX_TRY(b.sample(s0, pos_, n, ptr_.get(), idx_.get(), (uint32_t) nnz));
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

int HybSolver::steps(int64_t n_steps, int64_t stats[4], double* seconds) {
    MFX_REQUIRE(n_steps >= 0, "mfx_hyb_steps: n_steps must not be negative (got %lld)", (long long) n_steps);
    MFX_REQUIRE(have_tables_, "mfx_hyb_steps: no embeddings were set (mfx_hyb_set_embeddings)");
    return run(n_steps, false, stats, seconds);
}

int HybSolver::epochs(int32_t n_epochs, int64_t* stats, double* seconds) {
    MFX_REQUIRE(n_epochs >= 0, "mfx_hyb_epochs: n_epochs must not be negative (got %d)", n_epochs);
    MFX_REQUIRE(have_tables_, "mfx_hyb_epochs: no embeddings were set (mfx_hyb_set_embeddings)");
    for (int32_t e = 0; e < n_epochs; ++e) MFX_TRY(run(0, true, stats ? stats + 4 * e : nullptr, seconds ? seconds + e : nullptr));
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the single operators
int hyb_embed(const mfx_features* F, const float* E, int64_t k, float* out, int device) {
    const char* fn = "mfx_hyb_embed";
    MFX_REQUIRE(F, "%s: F is NULL", fn);
    MFX_REQUIRE(k >= 1 && k <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k);
    MFX_TRY(check_features(fn, "given", F, -1));
    MFX_REQUIRE(E, "%s: E is NULL", fn);
    if (F->n == 0) return MFX_OK;
    MFX_REQUIRE(out, "%s: out is NULL", fn);
    MFX_TRY(use_device(device));
    hipStream_t st = nullptr;
    HybSide side;
    MFX_TRY(side.init(fn, "given", F, F->n, MFX_HOST, st));
    DevBuf<float> x;
    MFX_TRY(side.E.alloc((size_t) side.nf * k));
    MFX_TRY(x.alloc((size_t) side.n * k));
    MFX_TRY(side.E.upload(E, (size_t) side.nf * k, MFX_HOST, st));
    HybArgs a{};
    a.user = side_args(side, x.get(), nullptr, nullptr, nullptr);
    a.n_work = (uint64_t) side.n;
    a.k = (int) k; a.gs = gs_of(k); a.gsh = __builtin_ctz((unsigned) a.gs);
    a.full = 1;
    MFX_TRY(launch_embed(a, st));
    MFX_HIP(hipMemcpyAsync(out, x.get(), sizeof(float) * side.n * k, hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int hyb_apply(int64_t rows, int64_t cols, int64_t k, const mfx_features* Fu, const mfx_features* Fi, float* Eu, float* Ei, int64_t n,
              const uint32_t* u, const uint32_t* i, const uint32_t* j, const uint8_t* skipped, float lr, float lambda, int64_t stats[4],
              int device) {
    const char* fn = "mfx_hyb_apply";
    MFX_TRY(check_sizes(fn, k, lr, lambda));
    MFX_REQUIRE(n >= 0 && n <= kHybMaxBatch, "%s: n must be in [0, 2^20] (got %lld)", fn, (long long) n);
    MFX_REQUIRE(rows >= 1 && cols >= 1 && rows < 0xFFFFFFFFll && cols < 0xFFFFFFFFll, "%s: rows and cols must be in [1, 2^32 - 1)", fn);
    MFX_REQUIRE(Eu && Ei && stats, "%s: Eu, Ei or stats is NULL", fn);
    MFX_REQUIRE(n == 0 || (u && i && j), "%s: u, i or j is NULL", fn);
    MFX_TRY(check_features(fn, "user", Fu, rows));
    MFX_TRY(check_features(fn, "item", Fi, cols));
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return MFX_OK;
    HybCore core;
    MFX_TRY(core.init(fn, rows, cols, k, n, Fu, Fi, MFX_HOST, device));
    hipStream_t st = core.bpr_.st_;
    MFX_TRY(core.bpr_.set_slots(fn, n, u, i, j, skipped));
    MFX_TRY(core.set_tables(Eu, Ei, MFX_HOST));
    MFX_TRY(core.step((uint32_t) n, lr, lambda));
    unsigned long long h[4] = {0, 0, 0, 0};
    MFX_HIP(hipMemcpyAsync(h, core.bpr_.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    MFX_TRY(core.get_tables(Eu, Ei, MFX_HOST));
    stats[0] = n;
    for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    return MFX_OK;
}

}  // namespace mfx
