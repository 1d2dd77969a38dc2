// bpr.hip -- Bayesian Personalised Ranking by deterministic mini-batch steps (mfx_bpr_*) on gfx950.  The contract -- the
// sampler, the score chain, the sigmoid recipe, the fixed-point sums and the update -- is in include/mfx.h; DESIGN 5.15 has
// the sizing of the accumulation and the measurements.
//
// A step takes n <= 2^20 slots (u, i, j) and runs four kernels on one stream, none of them over more than the slots:
//   k_bpr_sample   (solver only) one thread per slot: the triple of the running slot number, and whether j is in row u.
//   k_bpr_grad     one thread per slot: d = H[i] - H[j], the lane-owned FMA chain x of W[u] . d (16-byte row loads when
//                  k % 4 == 0), g = 1 / (1 + e^x) by the recipe below, and the slot's state: counted, skipped or bad (x not
//                  finite or a term of magnitude >= 64: |fp32(g * y)| is monotone in |y|, so the greatest |d_c| and |W[u][c]|
//                  of the chain decide).  The counts leave a wave as one 64-bit add each.
//   k_bpr_scatter  gs lanes per counted slot, lanes across c: the terms g * d_c, g * W[u][c] and its negative go as 64-bit
//                  integers (2^-36 fixed point, the conversion of ccd_scatter.hip) into the accumulator rows of u, i and j with
//                  global_atomic_add_x2 -- 512 contiguous bytes per wave-instruction at gs = 64.  Integer adds commute exactly, so
//                  a row's sum does not depend on the order of arrival.  The group's first lane counts the slot on its three
//                  rows and bids for them with atomicMin(claim[row], slot number).
//   k_bpr_apply    gs lanes per (slot, role): the slot whose number stands in a row's claim word -- the smallest counted slot
//                  that touches the row -- rounds the row's sums to fp32 once, updates the row, and puts accumulators, count
//                  and claim back to their rest state.  Rows nobody touched are neither read nor written, so after create
//                  no kernel and no memset runs over rows + cols.
// The factors are read by k_bpr_grad and k_bpr_scatter and written by k_bpr_apply alone: every slot sees the factors of
// before the step.  With negative sampling by trials (bpr_neg.hip) k_bpr_trials runs after the sampler and picks
// j among M trial items; in WARP it also writes g and the state, and k_bpr_grad is left out.
#include <algorithm>
#include <cmath>
#include <memory>

#include "bpr.hpp"
#include "bpr_device.hpp"

#ifndef MFX_LAUNCH_CHECK
#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())
#endif

namespace mfx {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr uint32_t kNoClaim = 0xFFFFFFFFu;
constexpr int64_t kBprMaxBatch = 1 << 20;
constexpr int kBprThreads = 256;

// (the sampler and the single fp32 operations: bpr_device.hpp)

// g = 1 / (1 + e^x), the recipe of include/mfx.h: clamp to +-80, n = rint(x * log2 e), r = (x - n * LN2_HI) - n * LN2_LO,
// the degree-6 Taylor polynomial of e^r by Horner in separately rounded multiplies and adds, e = ldexp(poly, n) (exact: the
// result is a normal number), one add, one correctly rounded division.
__device__ __forceinline__ float bpr_sigmoid_neg(float x) {
    const float xc = fminf(fmaxf(x, -80.f), 80.f);
    const float n = __builtin_rintf(mul_rn(xc, 1.4426950408889634f));
    const float r = sub_rn(sub_rn(xc, mul_rn(n, 0.693359375f)), mul_rn(n, -2.12194440e-4f));
    float p = 1.f / 720.f;
    p = add_rn(mul_rn(p, r), 1.f / 120.f);
    p = add_rn(mul_rn(p, r), 1.f / 24.f);
    p = add_rn(mul_rn(p, r), 1.f / 6.f);
    p = add_rn(mul_rn(p, r), 0.5f);
    p = add_rn(mul_rn(p, r), 1.f);
    p = add_rn(mul_rn(p, r), 1.f);
    const float e = ldexpf(p, (int) n);
    return __fdiv_rn(1.f, add_rn(1.f, e));
}

// fp32 -> 64-bit fixed point (two's complement), scale 2^36, truncated toward zero: ccd_scatter.hip's to_fixed.  |x| < 64.
__device__ __forceinline__ unsigned long long to_fixed(float x) {
    return (unsigned long long) (long long) ((double) x * 68719476736.0);
}

// ---------------------------------------------------------------------------------------------- kernels
// Row r of the matrix: its pointers inside [0, nnz] and in order, its ids strictly ascending and below cols.
__global__ void k_bpr_check(const uint32_t* ptr, const uint32_t* idx, uint32_t rows, uint32_t cols, uint32_t nnz, uint32_t* first_bad) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t lo = ptr[r], hi = ptr[r + 1];
        bool bad = lo > hi || hi > nnz || (r == 0 && lo != 0) || (r + 1 == rows && hi != nnz);
        if (!bad) {
            uint32_t prev = 0;
            for (uint32_t e = lo; e < hi; ++e) {
                const uint32_t c = idx[e];
                if (c >= cols || (e > lo && c <= prev)) { bad = true; break; }
                prev = c;
            }
        }
        if (bad) atomicMin(first_bad, (uint32_t) r);
    }
}

__global__ void k_bpr_check_ids(const uint32_t* u, const uint32_t* i, const uint32_t* j, uint32_t n, uint32_t rows, uint32_t cols,
                                uint32_t* first_bad) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n && (u[t] >= rows || i[t] >= cols || j[t] >= cols)) atomicMin(first_bad, t);
}

__global__ __launch_bounds__(kBprThreads) void k_bpr_sample(uint64_t s0, uint64_t base, uint32_t n, const uint32_t* __restrict__ ptr,
                                                            const uint32_t* __restrict__ idx, uint32_t rows, uint32_t cols, uint32_t nnz,
                                                            uint32_t* __restrict__ u, uint32_t* __restrict__ i, uint32_t* __restrict__ j,
                                                            uint8_t* __restrict__ skipped) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    bpr_sample(s0, base + t, ptr, idx, rows, cols, nnz, u + t, i + t, j + t, skipped + t);
}

struct BprArgs {
    float* W;                  // [rows][k]
    float* H;                  // [cols][k]
    unsigned long long* accW;  // [rows][k] the sums of the step, 0 between steps
    unsigned long long* accH;  // [cols][k]
    uint32_t* cntW;            // [rows] counted slots of the row, 0 between steps
    uint32_t* cntH;
    uint32_t* claimW;          // [rows] the smallest counted slot of the row, kNoClaim between steps
    uint32_t* claimH;
    const uint32_t* u;         // [n]
    const uint32_t* i;
    const uint32_t* j;
    const uint8_t* skipped;    // [n]
    float* g;                  // [n] of the counted slots
    uint8_t* state;            // [n]
    unsigned long long* stats; // [4] slots, skipped, bad, correct
    uint32_t n;
    int k, gs, gsh;            // gs = 1 << gsh lanes share a row in the scatter and the apply
    float lr, lambda;
};

__global__ __launch_bounds__(kBprThreads) void k_bpr_grad(BprArgs a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint8_t st = 0xFF;  // beyond the step
    bool correct = false;
    if (t < a.n) {
        st = kSkipped;
        if (!a.skipped[t]) {
            const int k = a.k;
            const float* w = a.W + (size_t) a.u[t] * k;
            const float* hi = a.H + (size_t) a.i[t] * k;
            const float* hj = a.H + (size_t) a.j[t] * k;
            float x = 0.f, md = 0.f, mw = 0.f;
            int c = 0;
            if ((k & 3) == 0) {
#pragma unroll 2
                for (; c + 4 <= k; c += 4) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
                    const f32x4 p = *reinterpret_cast<const f32x4*>(hi + c);
                    const f32x4 q = *reinterpret_cast<const f32x4*>(hj + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = p[e] - q[e];
                        x = __builtin_fmaf(wv[e], d, x);
                        md = fmaxf(md, fabsf(d));
                        mw = fmaxf(mw, fabsf(wv[e]));
                    }
                }
            }
            for (; c < k; ++c) {
                const float d = hi[c] - hj[c];
                x = __builtin_fmaf(w[c], d, x);
                md = fmaxf(md, fabsf(d));
                mw = fmaxf(mw, fabsf(w[c]));
            }
            const float g = bpr_sigmoid_neg(x);
            // (x finite: every W[u][c] and d_c is finite, an infinite one would have made x infinite or NaN)
            const bool ok = fabsf(x) < INFINITY && fabsf(mul_rn(g, md)) < 64.f && fabsf(mul_rn(g, mw)) < 64.f;
            st = ok ? kCounted : kBad;
            correct = ok && x > 0.f;
            a.g[t] = g;
        }
        a.state[t] = st;
    }
    const int nskip = __popcll(__ballot(st == kSkipped)), nbad = __popcll(__ballot(st == kBad)), ncor = __popcll(__ballot(correct));
    if ((threadIdx.x & 63) == 0) {
        if (nskip) atomicAdd(a.stats + 1, (unsigned long long) nskip);
        if (nbad) atomicAdd(a.stats + 2, (unsigned long long) nbad);
        if (ncor) atomicAdd(a.stats + 3, (unsigned long long) ncor);
    }
}

__global__ __launch_bounds__(kBprThreads) void k_bpr_scatter(BprArgs a) {
    const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t t64 = gid >> a.gsh;  // (gs is a power of two)
    const int cl = (int) (gid & (uint32_t) (a.gs - 1));
    if (t64 >= a.n) return;
    const uint32_t t = (uint32_t) t64;
    if (a.state[t] != kCounted) return;
    const int k = a.k;
    const uint32_t u = a.u[t], i = a.i[t], j = a.j[t];
    const float g = a.g[t];
    if (cl == 0) {
        atomicAdd(a.cntW + u, 1u);
        atomicAdd(a.cntH + i, 1u);
        atomicAdd(a.cntH + j, 1u);
        atomicMin(a.claimW + u, t);
        atomicMin(a.claimH + i, t);
        atomicMin(a.claimH + j, t);
    }
    const size_t ou = (size_t) u * k, oi = (size_t) i * k, oj = (size_t) j * k;
    for (int c = cl; c < k; c += a.gs) {
        const float w = a.W[ou + c];
        const float d = a.H[oi + c] - a.H[oj + c];
        const unsigned long long fw = to_fixed(mul_rn(g, d)), fh = to_fixed(mul_rn(g, w));
        atomicAdd(a.accW + ou + c, fw);
        atomicAdd(a.accH + oi + c, fh);
        atomicAdd(a.accH + oj + c, 0ull - fh);
    }
}

__global__ __launch_bounds__(kBprThreads) void k_bpr_apply(BprArgs a) {
    const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t item = gid >> a.gsh;
    const int cl = (int) (gid & (uint32_t) (a.gs - 1));
    const uint64_t t64 = item / 3;
    const int role = (int) (item - t64 * 3);
    if (t64 >= a.n) return;
    const uint32_t t = (uint32_t) t64;
    if (a.state[t] != kCounted) return;
    if (role == 2 && a.j[t] == a.i[t]) return;  // (the row was this slot's as the positive item already)
    const uint32_t row = role == 0 ? a.u[t] : role == 1 ? a.i[t] : a.j[t];
    uint32_t* claim = (role == 0 ? a.claimW : a.claimH) + row;
    if (*claim != t) return;  // (another slot's row; it may be back at kNoClaim by now, which is no slot number either)
    uint32_t* cnt = (role == 0 ? a.cntW : a.cntH) + row;
    const float reg = mul_rn(a.lambda, (float) *cnt);
    const int k = a.k;
    float* X = (role == 0 ? a.W : a.H) + (size_t) row * k;
    unsigned long long* acc = (role == 0 ? a.accW : a.accH) + (size_t) row * k;
    for (int c = cl; c < k; c += a.gs) {
        const float s = mul_rn((float) (long long) acc[c], 1.4551915228366852e-11f);  // one rounding int64 -> fp32, then the exact 2^-36
        const float old = X[c];
        X[c] = add_rn(old, mul_rn(a.lr, sub_rn(s, mul_rn(reg, old))));
        acc[c] = 0ull;
    }
    // (every lane of the group has read *claim and *cnt above: a group lies inside one wave, whose lanes pass a load together)
    if (cl == 0) {
        *cnt = 0u;
        *claim = kNoClaim;
    }
}

inline uint32_t grid_of(uint64_t threads) { return (uint32_t) ((threads + kBprThreads - 1) / kBprThreads); }

int check_space(const char* fn, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    return MFX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- BprCore
BprCore::~BprCore() {
    for (auto e : ev_)
        if (e) (void) hipEventDestroy(e);
}

int BprCore::init(int64_t rows, int64_t cols, int64_t k, int64_t batch, int device) {
    rows_ = rows; cols_ = cols; k_ = k; batch_ = batch; device_ = device;
    gs_ = 1;
    while (gs_ < 64 && gs_ < k) gs_ *= 2;
    MFX_TRY(use_device(device));
    const size_t nw = (size_t) rows * k, nh = (size_t) cols * k;
    MFX_TRY(W_.alloc(nw));
    MFX_TRY(H_.alloc(nh));
    MFX_TRY(accW_.alloc_zero(nw, st_));
    MFX_TRY(accH_.alloc_zero(nh, st_));
    MFX_TRY(cntW_.alloc_zero(rows, st_));
    MFX_TRY(cntH_.alloc_zero(cols, st_));
    MFX_TRY(claimW_.alloc(rows));
    MFX_TRY(claimH_.alloc(cols));
    MFX_HIP(hipMemsetAsync(claimW_.get(), 0xFF, sizeof(uint32_t) * rows, st_));
    MFX_HIP(hipMemsetAsync(claimH_.get(), 0xFF, sizeof(uint32_t) * cols, st_));
    MFX_TRY(u_.alloc(batch));
    MFX_TRY(i_.alloc(batch));
    MFX_TRY(j_.alloc(batch));
    MFX_TRY(g_.alloc(batch));
    MFX_TRY(skip_.alloc(batch));
    MFX_TRY(state_.alloc(batch));
    MFX_TRY(stats_.alloc_zero(4, st_));
    for (auto& e : ev_) MFX_HIP(hipEventCreate(&e));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int BprCore::upload(const float* W, const float* H, mfx_memspace space) {
    MFX_TRY(use_device(device_));
    MFX_TRY(W_.upload(W, (size_t) rows_ * k_, space, st_));
    MFX_TRY(H_.upload(H, (size_t) cols_ * k_, space, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int BprCore::download(float* W, float* H, mfx_memspace space) {
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (W) MFX_HIP(hipMemcpyAsync(W, W_.get(), sizeof(float) * rows_ * k_, kind, st_));
    if (H) MFX_HIP(hipMemcpyAsync(H, H_.get(), sizeof(float) * cols_ * k_, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

namespace {
BprArgs args_of(const BprCore& c, uint32_t n, float lr, float lambda) {
    BprArgs a{};
    a.W = c.W_.get(); a.H = c.H_.get();
    a.accW = c.accW_.get(); a.accH = c.accH_.get();
    a.cntW = c.cntW_.get(); a.cntH = c.cntH_.get();
    a.claimW = c.claimW_.get(); a.claimH = c.claimH_.get();
    a.u = c.u_.get(); a.i = c.i_.get(); a.j = c.j_.get();
    a.skipped = c.skip_.get(); a.g = c.g_.get(); a.state = c.state_.get();
    a.stats = c.stats_.get();
    a.n = n; a.k = (int) c.k_; a.gs = c.gs_; a.gsh = __builtin_ctz((unsigned) c.gs_);
    a.lr = lr; a.lambda = lambda;
    return a;
}
}  // namespace

int BprCore::grad_scatter(uint32_t n) {
    if (n == 0) return MFX_OK;
    MFX_REQUIRE((int64_t) n <= batch_, "bpr: a step of %u slots on a handle made for %lld", n, (long long) batch_);
    const BprArgs a = args_of(*this, n, 0.f, 0.f);
    if (profile_) MFX_HIP(hipEventRecord(ev_[1], st_));
    if (neg_mode_ != MFX_BPR_NEG_WARP) {  // (WARP: k_bpr_trials has written g and the state, its weight is no sigmoid)
        hipLaunchKernelGGL(k_bpr_grad, dim3(grid_of(n)), dim3(kBprThreads), 0, st_, a);
        MFX_LAUNCH_CHECK();
    }
    if (profile_) MFX_HIP(hipEventRecord(ev_[2], st_));
    hipLaunchKernelGGL(k_bpr_scatter, dim3(grid_of((uint64_t) n * gs_)), dim3(kBprThreads), 0, st_, a);
    MFX_LAUNCH_CHECK();
    if (profile_) MFX_HIP(hipEventRecord(ev_[3], st_));
    return MFX_OK;
}

int BprCore::apply(uint32_t n, float lr, float lambda) {
    if (n == 0) return MFX_OK;
    const BprArgs a = args_of(*this, n, lr, lambda);
    hipLaunchKernelGGL(k_bpr_apply, dim3(grid_of((uint64_t) n * 3 * gs_)), dim3(kBprThreads), 0, st_, a);
    MFX_LAUNCH_CHECK();
    if (profile_) {
        MFX_HIP(hipEventRecord(ev_[4], st_));
        MFX_HIP(hipEventSynchronize(ev_[4]));
        for (int p = 0; p < 4; ++p) {
            float ms = 0.f;
            MFX_HIP(hipEventElapsedTime(&ms, ev_[p], ev_[p + 1]));
            phase_s_[p] += 1e-3 * ms;
        }
    }
    return MFX_OK;
}

int BprCore::step(uint32_t n, float lr, float lambda) {
    MFX_TRY(grad_scatter(n));
    return apply(n, lr, lambda);
}

int BprCore::sample(uint64_t s0, uint64_t base, uint32_t n, const uint32_t* ptr, const uint32_t* idx, uint32_t nnz) {
    hipLaunchKernelGGL(k_bpr_sample, dim3(grid_of(n)), dim3(kBprThreads), 0, st_, s0, base, n, ptr, idx, (uint32_t) rows_, (uint32_t) cols_, nnz,
                       u_.get(), i_.get(), j_.get(), skip_.get());
    MFX_LAUNCH_CHECK();
    return MFX_OK;
}

int BprCore::set_slots(const char* fn, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j, const uint8_t* skipped) {
    MFX_TRY(u_.upload(u, (size_t) n, MFX_HOST, st_));
    MFX_TRY(i_.upload(i, (size_t) n, MFX_HOST, st_));
    MFX_TRY(j_.upload(j, (size_t) n, MFX_HOST, st_));
    if (skipped) MFX_TRY(skip_.upload(skipped, (size_t) n, MFX_HOST, st_));
    else MFX_HIP(hipMemsetAsync(skip_.get(), 0, (size_t) n, st_));
    DevBuf<uint32_t> bad;
    MFX_TRY(bad.alloc(1));
    MFX_HIP(hipMemsetAsync(bad.get(), 0xFF, sizeof(uint32_t), st_));
    hipLaunchKernelGGL(k_bpr_check_ids, dim3(grid_of((uint64_t) n)), dim3(kBprThreads), 0, st_, u_.get(), i_.get(), j_.get(), (uint32_t) n,
                       (uint32_t) rows_, (uint32_t) cols_, bad.get());
    MFX_LAUNCH_CHECK();
    uint32_t first_bad = kNoClaim;
    MFX_HIP(hipMemcpyAsync(&first_bad, bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    MFX_REQUIRE(first_bad == kNoClaim, "%s: slot %u names a user >= rows or an item >= cols", fn, first_bad);
    return MFX_OK;
}

// The rows of one side of a matrix on the device (k_bpr_check): *first_bad = the first row that breaks the rules, or 2^32 - 1.
int bpr_check_rows(const uint32_t* ptr, const uint32_t* idx, uint32_t rows, uint32_t cols, uint32_t nnz, hipStream_t st, uint32_t* first_bad) {
    DevBuf<uint32_t> bad;
    MFX_TRY(bad.alloc(1));
    MFX_HIP(hipMemsetAsync(bad.get(), 0xFF, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_bpr_check, dim3(std::min<uint32_t>(grid_of(rows), 65536u)), dim3(kBprThreads), 0, st, ptr, idx, rows, cols, nnz, bad.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipMemcpyAsync(first_bad, bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the solver
int BprSolver::create(BprSolver** out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed, mfx_memspace space,
                      const char* fn, int mode, int64_t negatives, const float* rank_weight) {
    MFX_REQUIRE(out && R && p, "%s: null argument", fn);
    *out = nullptr;
    MFX_TRY(check_space(fn, space));
    MFX_TRY(bpr_check_neg(fn, mode, negatives, rank_weight));
    MFX_REQUIRE(p->k >= 1 && p->k <= 1024, "%s: k must be in [1, 1024] (got %u)", fn, p->k);
    MFX_REQUIRE(batch >= 1 && batch <= kBprMaxBatch, "%s: batch must be in [1, 2^20] (got %lld)", fn, (long long) batch);
    MFX_REQUIRE(std::isfinite(lr) && lr >= 0.f, "%s: lr must be finite and >= 0 (got %g)", fn, (double) lr);
    MFX_REQUIRE(std::isfinite(p->lambda) && p->lambda >= 0.f, "%s: lambda must be finite and >= 0 (got %g)", fn, (double) p->lambda);
    MFX_REQUIRE(R->nnz >= 1, "%s: the matrix has no entries", fn);
    MFX_REQUIRE(R->cols >= 2, "%s: cols must be at least 2 (got %lld)", fn, (long long) R->cols);
    MFX_REQUIRE(R->rows >= 1 && R->rows < 0xFFFFFFFFll && R->cols < 0xFFFFFFFFll && R->nnz < 0xFFFFFFFFll,
                "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    MFX_REQUIRE(R->csr_row_ptr && R->csr_col_idx, "%s: the CSR side of R is NULL", fn);
    std::unique_ptr<BprSolver> s(new BprSolver());
    s->nnz_ = R->nnz; s->lr_ = lr; s->lambda_ = p->lambda; s->seed_ = seed;
    MFX_TRY(s->core_.init(R->rows, R->cols, p->k, std::min<int64_t>(batch, R->nnz), p->device));
    s->core_.batch_ = batch;  // (a step never has more than nnz slots: the slot arrays are sized for min(batch, nnz))
    s->core_.profile_ = p->profile != 0;
    if (mode != MFX_BPR_NEG_UNIFORM) MFX_TRY(s->core_.init_neg(mode, (int) negatives, rank_weight));
    hipStream_t st = s->core_.st_;
    const uint32_t rows = (uint32_t) R->rows;
    MFX_TRY(s->ptr_.alloc((size_t) rows + 1));
    MFX_TRY(s->idx_.alloc((size_t) R->nnz));
    MFX_TRY(s->ptr_.upload(R->csr_row_ptr, (size_t) rows + 1, space, st));
    MFX_TRY(s->idx_.upload(R->csr_col_idx, (size_t) R->nnz, space, st));
    uint32_t first_bad = kNoClaim;
    MFX_TRY(bpr_check_rows(s->ptr_.get(), s->idx_.get(), rows, (uint32_t) R->cols, (uint32_t) R->nnz, st, &first_bad));
    MFX_REQUIRE(first_bad == kNoClaim,
                "%s: row %u of the CSR side: its pointers must ascend from 0 to nnz and its ids be strictly ascending and below cols", fn,
                first_bad);
    *out = s.release();
    return MFX_OK;
}

int BprSolver::set_factors(const float* W, const float* H, mfx_memspace space) {
    MFX_REQUIRE(W && H, "mfx_bpr_set_factors: W or H is NULL");
    MFX_TRY(check_space("mfx_bpr_set_factors", space));
    MFX_TRY(core_.upload(W, H, space));
    have_factors_ = true;
    return MFX_OK;
}

int BprSolver::get_factors(float* W, float* H, mfx_memspace space) {
    MFX_REQUIRE(have_factors_, "mfx_bpr_get_factors: no factors were set");
    MFX_TRY(check_space("mfx_bpr_get_factors", space));
    return core_.download(W, H, space);
}

void BprSolver::times(double seconds[4]) const {
    for (int p = 0; p < 4; ++p) seconds[p] = core_.phase_s_[p];
}

// n_steps steps from the current slot, or (to_epoch_end) the steps up to the end of the epoch that holds it.
int BprSolver::run(int64_t n_steps, bool to_epoch_end, int64_t stats[4], double* seconds) {
    MFX_TRY(use_device(core_.device_));
    hipStream_t st = core_.st_;
    MFX_HIP(hipMemsetAsync(core_.stats_.get(), 0, 4 * sizeof(unsigned long long), st));
    hipEvent_t t0 = core_.ev_[5], t1 = core_.ev_[6];
    MFX_HIP(hipEventRecord(t0, st));
    const uint64_t s0 = bpr_stream(seed_), s1 = bpr_trial_stream(seed_), nnz = (uint64_t) nnz_;
    const bool neg = core_.neg_mode_ != MFX_BPR_NEG_UNIFORM;
    if (neg) MFX_HIP(hipMemsetAsync(core_.tstats_.get(), 0, 2 * sizeof(unsigned long long), st));
    int64_t slots = 0;
    for (int64_t s = 0; to_epoch_end || s < n_steps; ++s) {
        const uint32_t n = (uint32_t) std::min<uint64_t>((uint64_t) core_.batch_, nnz - pos_ % nnz);
        if (core_.profile_) MFX_HIP(hipEventRecord(core_.ev_[0], st));
        MFX_TRY(core_.sample(s0, pos_, n, ptr_.get(), idx_.get(), (uint32_t) nnz_));
        if (neg) MFX_TRY(core_.trials(n, nullptr, nullptr, s1, pos_, ptr_.get(), idx_.get()));
        MFX_TRY(core_.step(n, lr_, lambda_));
        pos_ += n;
        slots += n;
        if (to_epoch_end && pos_ % nnz == 0) break;
    }
    MFX_HIP(hipEventRecord(t1, st));
    unsigned long long h[4] = {0, 0, 0, 0}, ht[2] = {0, 0};
    MFX_HIP(hipMemcpyAsync(h, core_.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    if (neg) MFX_HIP(hipMemcpyAsync(ht, core_.tstats_.get(), sizeof(ht), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    // (uniform: the one trial is chosen unless it is in the row)
    tstat_[0] += neg ? (int64_t) ht[0] : (int64_t) h[1];
    tstat_[1] += neg ? (int64_t) ht[1] : slots - (int64_t) h[1];
    float ms = 0.f;
    MFX_HIP(hipEventElapsedTime(&ms, t0, t1));
    if (seconds) *seconds = 1e-3 * ms;
    if (stats) {
        stats[0] = slots;
        for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    }
    return MFX_OK;
}

int BprSolver::steps(int64_t n_steps, int64_t stats[4], double* seconds) {
    MFX_REQUIRE(n_steps >= 0, "mfx_bpr_steps: n_steps must not be negative (got %lld)", (long long) n_steps);
    MFX_REQUIRE(have_factors_, "mfx_bpr_steps: no factors were set (mfx_bpr_set_factors)");
    return run(n_steps, false, stats, seconds);
}

int BprSolver::epochs(int32_t n_epochs, int64_t* stats, double* seconds) {
    MFX_REQUIRE(n_epochs >= 0, "mfx_bpr_epochs: n_epochs must not be negative (got %d)", n_epochs);
    MFX_REQUIRE(have_factors_, "mfx_bpr_epochs: no factors were set (mfx_bpr_set_factors)");
    for (int32_t e = 0; e < n_epochs; ++e) MFX_TRY(run(0, true, stats ? stats + 4 * e : nullptr, seconds ? seconds + e : nullptr));
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- host-only sampler
int bpr_triples(uint64_t seed, int64_t first_slot, int64_t count, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* j, uint8_t* skipped) {
    const char* fn = "mfx_bpr_triples";
    MFX_REQUIRE(R && R->csr_row_ptr && R->csr_col_idx, "%s: R or its CSR side is NULL", fn);
    MFX_REQUIRE(count >= 0 && first_slot >= 0, "%s: first_slot and count must not be negative", fn);
    MFX_REQUIRE(R->nnz >= 1 && R->cols >= 2 && R->rows >= 1, "%s: the matrix needs an entry and two columns", fn);
    MFX_REQUIRE(R->rows < 0xFFFFFFFFll && R->cols < 0xFFFFFFFFll && R->nnz < 0xFFFFFFFFll, "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    if (count == 0) return MFX_OK;
    MFX_REQUIRE(u && i && j && skipped, "%s: an output array is NULL", fn);
    const uint32_t* ptr = R->csr_row_ptr;
    MFX_REQUIRE(ptr[0] == 0 && ptr[R->rows] == (uint64_t) R->nnz, "%s: csr_row_ptr must run from 0 to nnz", fn);
    for (int64_t r = 0; r < R->rows; ++r) MFX_REQUIRE(ptr[r] <= ptr[r + 1], "%s: csr_row_ptr decreases at row %lld", fn, (long long) r);
    const uint64_t s0 = bpr_stream(seed);
    for (int64_t t = 0; t < count; ++t)
        bpr_sample(s0, (uint64_t) first_slot + (uint64_t) t, ptr, R->csr_col_idx, (uint32_t) R->rows, (uint32_t) R->cols, (uint32_t) R->nnz,
                   u + t, i + t, j + t, skipped + t);
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the single operator
int bpr_apply(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
              const uint8_t* skipped, float lr, float lambda, int64_t stats[4], int device) {
    const char* fn = "mfx_bpr_apply";
    MFX_REQUIRE(k >= 1 && k <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k);
    MFX_REQUIRE(n >= 0 && n <= kBprMaxBatch, "%s: n must be in [0, 2^20] (got %lld)", fn, (long long) n);
    MFX_REQUIRE(std::isfinite(lr) && lr >= 0.f, "%s: lr must be finite and >= 0 (got %g)", fn, (double) lr);
    MFX_REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "%s: lambda must be finite and >= 0 (got %g)", fn, (double) lambda);
    MFX_REQUIRE(rows >= 1 && cols >= 1 && rows < 0xFFFFFFFFll && cols < 0xFFFFFFFFll, "%s: rows and cols must be in [1, 2^32 - 1)", fn);
    MFX_REQUIRE(W && H && stats, "%s: W, H or stats is NULL", fn);
    MFX_REQUIRE(n == 0 || (u && i && j), "%s: u, i or j is NULL", fn);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return MFX_OK;
    BprCore core;
    MFX_TRY(core.init(rows, cols, k, n, device));
    hipStream_t st = core.st_;
    MFX_TRY(core.set_slots(fn, n, u, i, j, skipped));
    MFX_TRY(core.upload(W, H, MFX_HOST));
    MFX_TRY(core.step((uint32_t) n, lr, lambda));
    unsigned long long h[4] = {0, 0, 0, 0};
    MFX_HIP(hipMemcpyAsync(h, core.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    MFX_TRY(core.download(W, H, MFX_HOST));
    stats[0] = n;
    for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    return MFX_OK;
}

}  // namespace mfx
