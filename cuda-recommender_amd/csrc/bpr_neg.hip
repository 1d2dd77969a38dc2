// bpr_neg.hip -- negative sampling by trials for BPR training (mfx_bpr_create_neg, mfx_bpr_apply_neg, mfx_bpr_trials) on
// gfx950: hardest of M and WARP.  The contract is in include/mfx.h ("Negative sampling by trials"), DESIGN 5.17 has the shape
// of the kernel and the measurements.  Everything here happens BEFORE the step of bpr.hip, whose kernels are unchanged: a
// slot still enters k_bpr_scatter / k_bpr_apply as (u, i, j) with a weight g and a state.
//
//   k_bpr_trials   L lanes per slot (a power of two <= 64, so a group lies inside one wave), one trial per lane, in rounds
//                  of L.  A lane hashes its own trial item (or reads it from the caller's array), searches row u for it, and
//                  owns the FMA chain of W[u] . H[c_t] (16-byte row loads when k % 4 == 0): W[u] is one address across the
//                  group, the H rows are the gather.  No sum crosses lanes, so no bit depends on L.
//                  HARDEST: a lane keeps the greatest key (score order, then the smaller t) of its trials, the group takes the
//                  maximum by xor shuffles, its first lane writes j, the skip flag and t; k_bpr_grad follows as ever.
//                  WARP: every lane has the chain of the positive item; a round ends with a ballot of the violators masked
//                  to the group, and the first round that holds one ends the slot (the factors are frozen, so this is the
//                  sequential definition).  The group then takes max |d_c| and max |W[u][c]| across its lanes (a maximum has
//                  no order) for the limit on the terms, and its first lane writes j, g = the rank weight, the state and t.
//                  The slots are walked with a grid stride and the counts stay in registers: a wave adds each of them once.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bpr.hpp"
#include "bpr_device.hpp"

#ifndef MFX_LAUNCH_CHECK
#define MFX_LAUNCH_CHECK() MFX_HIP(hipGetLastError())
#endif

namespace mfx {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr int64_t kBprMaxBatch = 1 << 20;
constexpr int64_t kMaxNegatives = 1024;
constexpr int kThreads = 256;
constexpr uint32_t kMaxBlocks = 8192;  // of k_bpr_trials: 32 waves for each of the 1 024 SIMDs

struct TrialArgs {
    const float* W;             // [rows][k]
    const float* H;             // [cols][k]
    const uint32_t* u;          // [n]
    const uint32_t* i;          // [n]
    uint32_t* j;                // [n] in: trial 1 (stream); out: the chosen item
    uint8_t* skip;              // [n] in: member_1 (stream); out (HARDEST): no eligible trial
    float* g;                   // [n] out (WARP)
    uint8_t* state;             // [n] out (WARP)
    uint32_t* t;                // [n] out: the chosen trial, 0 = none
    unsigned long long* stats;  // [4] slots, skipped, bad, correct (WARP adds to the last three)
    unsigned long long* tstats; // [2] slots without a chosen trial, the sum of the chosen t
    const float* rw;            // [M] (WARP)
    const uint32_t* items;      // [n][M] the caller's trials, or NULL: the stream
    const uint8_t* member;      // [n][M] or NULL: none
    const uint32_t* ptr;        // the matrix (stream)
    const uint32_t* idx;
    uint64_t s1, base;          // the stream of the trials, the number of slot 0 of the step
    uint32_t n, cols;
    int k, M, L, lsh;           // L = 1 << lsh lanes share a slot
};

// acc = fmaf(w[c], h[c], acc) over c ascending from +0: the chain of mfx_rec_score, all of it in this lane.
__device__ __forceinline__ float score_chain(const float* __restrict__ w, const float* __restrict__ h, int k) {
    float x = 0.f;
    int c = 0;
    if ((k & 3) == 0) {
        // (eight row loads in flight per lane: the gather is bound by latency, not by registers -- DESIGN 5.17)
#pragma unroll 8
        for (; c + 4 <= k; c += 4) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + c);
            const f32x4 hv = *reinterpret_cast<const f32x4*>(h + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) x = __builtin_fmaf(wv[e], hv[e], x);
        }
    }
    for (; c < k; ++c) x = __builtin_fmaf(w[c], h[c], x);
    return x;
}

// Trial t (1-based) of slot s.
__device__ __forceinline__ void trial_of(const TrialArgs& a, uint32_t s, uint32_t t, uint64_t base, uint32_t u, uint32_t* c, uint8_t* member) {
    if (a.items) {
        const size_t o = (size_t) s * a.M + (t - 1);
        *c = a.items[o];
        *member = a.member ? a.member[o] != 0 : 0;
    } else if (t == 1) {
        *c = a.j[s];
        *member = a.skip[s];
    } else {
        bpr_trial(base, t, a.ptr, a.idx, u, a.cols, c, member);
    }
}

// The order of HARDEST as an integer: 0 is kept for "no eligible trial", a NaN is 1, the numbers ascend above it with
// -0 = +0; the low word prefers the smaller t.
__device__ __forceinline__ unsigned long long hardest_key(float score, uint32_t t) {
    uint32_t b = __float_as_uint(score), ord;
    if (score != score) ord = 1u;
    else {
        if (b == 0x80000000u) b = 0u;
        ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // (-inf becomes 0x007FFFFF, above the NaN)
    }
    return ((unsigned long long) ord << 32) | (0xFFFFFFFFu - t);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_bpr_trials(TrialArgs a) {
    const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = ((uint64_t) gridDim.x * blockDim.x) >> a.lsh;  // groups of the grid
    const int L = a.L, gl = (int) (gid & (uint32_t) (L - 1));
    const int g0 = (int) (threadIdx.x & 63) - gl;  // the group's first lane in its wave
    const unsigned long long gmask = (L == 64 ? ~0ull : (1ull << L) - 1ull) << g0;
    const int k = a.k;
    const uint32_t M = (uint32_t) a.M;
    uint32_t nskip = 0, nbad = 0, ncor = 0, nnone = 0, tsum = 0;  // of this lane's slots, kept by the group's first lane
    for (uint64_t s64 = gid >> a.lsh; s64 < a.n; s64 += stride) {  // (the lanes of a group leave together)
        const uint32_t s = (uint32_t) s64;
        const uint32_t u = a.u[s], pi = a.i[s];
        const float* w = a.W + (size_t) u * k;
        const uint64_t base = a.items ? 0ull : bpr_trial_base(a.s1, a.base + s);
        uint32_t chosen_t = 0, chosen_c = 0;
        if (MODE == MFX_BPR_NEG_HARDEST) {
            unsigned long long best = 0ull;
            for (uint32_t r0 = 0; r0 < M; r0 += L) {
                const uint32_t t = r0 + gl + 1;
                if (t <= M) {
                    uint32_t c;
                    uint8_t mem;
                    trial_of(a, s, t, base, u, &c, &mem);
                    if (!mem) {
                        const unsigned long long key = hardest_key(score_chain(w, a.H + (size_t) c * k, k), t);
                        best = key > best ? key : best;
                    }
                }
            }
            for (int o = L >> 1; o; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o);
                best = other > best ? other : best;
            }
            if (gl == 0) {
                if (best) {
                    uint8_t mem;
                    chosen_t = 0xFFFFFFFFu - (uint32_t) best;
                    trial_of(a, s, chosen_t, base, u, &chosen_c, &mem);
                    a.j[s] = chosen_c;
                }
                a.skip[s] = best == 0ull;
                a.t[s] = chosen_t;
            }
        } else {
            const float* hi = a.H + (size_t) pi * k;
            const float si = score_chain(w, hi, k);
            uint8_t st = kSkipped;
            bool correct = false;
            float g = 0.f;
            if (!(fabsf(si) < INFINITY)) st = kBad;
            else {
                float chosen_s = 0.f;
                for (uint32_t r0 = 0; r0 < M; r0 += L) {
                    const uint32_t t = r0 + gl + 1;
                    uint32_t c = 0;
                    float sc = 0.f;
                    bool viol = false;
                    if (t <= M) {
                        uint8_t mem;
                        trial_of(a, s, t, base, u, &c, &mem);
                        if (!mem) {
                            sc = score_chain(w, a.H + (size_t) c * k, k);
                            viol = !(sub_rn(si, sc) >= 1.0f);
                        }
                    }
                    const unsigned long long b = __ballot(viol) & gmask;
                    if (b) {
                        const int src = __builtin_ctzll(b);  // (a lane of this group: it is here)
                        chosen_t = r0 + (uint32_t) (src - g0) + 1;
                        chosen_c = __shfl(c, src);
                        chosen_s = __shfl(sc, src);
                        break;
                    }
                }
                if (chosen_t) {
                    // (s_i finite: W[u] and H[i] are finite; with s_t finite so is H[j], and d_c is a number or an infinity)
                    const float* hj = a.H + (size_t) chosen_c * k;
                    float md = 0.f, mw = 0.f;
                    for (int c = gl; c < k; c += L) {
                        md = fmaxf(md, fabsf(sub_rn(hi[c], hj[c])));
                        mw = fmaxf(mw, fabsf(w[c]));
                    }
                    for (int o = L >> 1; o; o >>= 1) {
                        md = fmaxf(md, __shfl_xor(md, o));
                        mw = fmaxf(mw, __shfl_xor(mw, o));
                    }
                    g = a.rw[chosen_t - 1];
                    // (|fp32(g * y)| is monotone in |y| for g >= 0: the greatest |d_c| and |W[u][c]| decide; 0 * inf is a NaN)
                    const bool ok = fabsf(chosen_s) < INFINITY && fabsf(mul_rn(g, md)) < 64.f && fabsf(mul_rn(g, mw)) < 64.f;
                    st = ok ? kCounted : kBad;
                    correct = ok && sub_rn(si, chosen_s) > 0.f;
                }
            }
            if (gl == 0) {
                if (chosen_t) a.j[s] = chosen_c;
                a.g[s] = g;
                a.state[s] = st;
                a.t[s] = chosen_t;
                nskip += st == kSkipped;
                nbad += st == kBad;
                ncor += correct;
            }
        }
        if (gl == 0) {
            nnone += chosen_t == 0;
            tsum += chosen_t;  // (at most 2^20 slots of at most 1 024: no overflow, not even of the wave's sum)
        }
    }
    nnone = wave_sum(nnone);
    tsum = wave_sum(tsum);
    if (MODE == MFX_BPR_NEG_WARP) {
        nskip = wave_sum(nskip);
        nbad = wave_sum(nbad);
        ncor = wave_sum(ncor);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nnone) atomicAdd(a.tstats + 0, (unsigned long long) nnone);
        if (tsum) atomicAdd(a.tstats + 1, (unsigned long long) tsum);
        if (MODE == MFX_BPR_NEG_WARP) {
            if (nskip) atomicAdd(a.stats + 1, (unsigned long long) nskip);
            if (nbad) atomicAdd(a.stats + 2, (unsigned long long) nbad);
            if (ncor) atomicAdd(a.stats + 3, (unsigned long long) ncor);
        }
    }
}

// Thread e looks at trial e of the [n][M] array, the first thread of a slot at its user and positive item as well.
__global__ void k_bpr_check_trials(const uint32_t* u, const uint32_t* i, const uint32_t* items, uint32_t n, uint32_t M, uint32_t rows,
                                   uint32_t cols, uint32_t* first_bad) {
    const uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t s = e / M;
    if (s >= n) return;
    bool bad = items[e] >= cols;
    if (e - s * M == 0) bad = bad || u[s] >= rows || i[s] >= cols;
    if (bad) atomicMin(first_bad, (uint32_t) s);
}

inline uint32_t grid_of(uint64_t threads) { return (uint32_t) ((threads + kThreads - 1) / kThreads); }

// The lanes per slot.  HARDEST scores every trial: the smallest power of two that holds them in one round, so W[u] is read
// once per slot by as few wave-instructions as can be.  WARP stops at the first violator, mostly among the first trials:
// rounds of 4 (measured against 2, 8, 16 and 32: DESIGN 5.17).  MFX_BPR_TRIAL_GROUP overrides both, for measuring; no bit
// depends on it.
int group_width(int mode, int M) {
    int L = 1;
    while (L < 64 && L < M) L *= 2;
    if (mode == MFX_BPR_NEG_WARP) L = std::min(L, 4);
    if (const char* e = std::getenv("MFX_BPR_TRIAL_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) L = v;
    }
    return L;
}

}  // namespace

// ---------------------------------------------------------------------------------------------- host: checks and tables
int bpr_check_neg(const char* fn, int mode, int64_t negatives, const float* rank_weight) {
    MFX_REQUIRE(mode == MFX_BPR_NEG_UNIFORM || mode == MFX_BPR_NEG_HARDEST || mode == MFX_BPR_NEG_WARP, "%s: mode must be 0, 1 or 2 (got %d)", fn,
                mode);
    MFX_REQUIRE(negatives >= 1 && negatives <= kMaxNegatives, "%s: negatives must be in [1, 1024] (got %lld)", fn, (long long) negatives);
    MFX_REQUIRE(mode != MFX_BPR_NEG_UNIFORM || negatives == 1, "%s: the uniform mode takes one negative (got %lld)", fn, (long long) negatives);
    if (rank_weight)
        for (int64_t t = 0; t < negatives; ++t)
            MFX_REQUIRE(std::isfinite(rank_weight[t]) && rank_weight[t] >= 0.f, "%s: rank_weight[%lld] must be finite and >= 0 (got %g)", fn,
                        (long long) t, (double) rank_weight[t]);
    return MFX_OK;
}

int bpr_rank_weights(int64_t cols, int64_t negatives, float* out) {
    const char* fn = "mfx_bpr_rank_weights";
    MFX_REQUIRE(cols >= 1, "%s: cols must be at least 1 (got %lld)", fn, (long long) cols);
    MFX_REQUIRE(negatives >= 1 && negatives <= kMaxNegatives, "%s: negatives must be in [1, 1024] (got %lld)", fn, (long long) negatives);
    MFX_REQUIRE(out, "%s: out is NULL", fn);
    for (int64_t t = 1; t <= negatives; ++t) out[t - 1] = (float) std::log((double) std::max<int64_t>(1, (cols - 1) / t));
    return MFX_OK;
}

int bpr_trials(uint64_t seed, int64_t first_slot, int64_t count, int64_t negatives, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* items,
               uint8_t* member) {
    const char* fn = "mfx_bpr_trials";
    MFX_REQUIRE(R && R->csr_row_ptr && R->csr_col_idx, "%s: R or its CSR side is NULL", fn);
    MFX_REQUIRE(count >= 0 && first_slot >= 0, "%s: first_slot and count must not be negative", fn);
    MFX_REQUIRE(negatives >= 1 && negatives <= kMaxNegatives, "%s: negatives must be in [1, 1024] (got %lld)", fn, (long long) negatives);
    MFX_REQUIRE(R->nnz >= 1 && R->cols >= 2 && R->rows >= 1, "%s: the matrix needs an entry and two columns", fn);
    MFX_REQUIRE(R->rows < 0xFFFFFFFFll && R->cols < 0xFFFFFFFFll && R->nnz < 0xFFFFFFFFll, "%s: rows, cols and nnz must be below 2^32 - 1", fn);
    if (count == 0) return MFX_OK;
    MFX_REQUIRE(u && i && items && member, "%s: an output array is NULL", fn);
    const uint32_t* ptr = R->csr_row_ptr;
    MFX_REQUIRE(ptr[0] == 0 && ptr[R->rows] == (uint64_t) R->nnz, "%s: csr_row_ptr must run from 0 to nnz", fn);
    for (int64_t r = 0; r < R->rows; ++r) MFX_REQUIRE(ptr[r] <= ptr[r + 1], "%s: csr_row_ptr decreases at row %lld", fn, (long long) r);
    const uint64_t s0 = bpr_stream(seed), s1 = bpr_trial_stream(seed);
    for (int64_t s = 0; s < count; ++s) {
        const uint64_t n = (uint64_t) first_slot + (uint64_t) s;
        uint32_t* it = items + s * negatives;
        uint8_t* mem = member + s * negatives;
        bpr_sample(s0, n, ptr, R->csr_col_idx, (uint32_t) R->rows, (uint32_t) R->cols, (uint32_t) R->nnz, u + s, i + s, it, mem);
        const uint64_t base = bpr_trial_base(s1, n);
        for (int64_t t = 2; t <= negatives; ++t) bpr_trial(base, (uint32_t) t, ptr, R->csr_col_idx, u[s], (uint32_t) R->cols, it + t - 1, mem + t - 1);
    }
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- BprCore: the trials
int BprCore::init_neg(int mode, int negatives, const float* rank_weight) {
    neg_mode_ = mode;
    negatives_ = negatives;
    group_ = group_width(mode, negatives);
    MFX_TRY(use_device(device_));
    MFX_TRY(t_.alloc(u_.size()));
    MFX_TRY(tstats_.alloc_zero(2, st_));
    if (mode == MFX_BPR_NEG_WARP) {
        std::vector<float> table((size_t) negatives);
        if (rank_weight) std::copy(rank_weight, rank_weight + negatives, table.begin());
        else MFX_TRY(bpr_rank_weights(cols_, negatives, table.data()));
        MFX_TRY(rw_.alloc((size_t) negatives));
        MFX_TRY(rw_.upload(table.data(), (size_t) negatives, MFX_HOST, st_));
    }
    MFX_HIP(hipStreamSynchronize(st_));  // (the table is a local)
    return MFX_OK;
}

int BprCore::trials(uint32_t n, const uint32_t* items, const uint8_t* member, uint64_t s1, uint64_t base, const uint32_t* ptr, const uint32_t* idx) {
    if (n == 0) return MFX_OK;
    TrialArgs a{};
    a.W = W_.get(); a.H = H_.get();
    a.u = u_.get(); a.i = i_.get(); a.j = j_.get();
    a.skip = skip_.get(); a.g = g_.get(); a.state = state_.get(); a.t = t_.get();
    a.stats = stats_.get(); a.tstats = tstats_.get();
    a.rw = rw_.get();
    a.items = items; a.member = member;
    a.ptr = ptr; a.idx = idx; a.s1 = s1; a.base = base;
    a.n = n; a.cols = (uint32_t) cols_;
    a.k = (int) k_; a.M = negatives_; a.L = group_; a.lsh = __builtin_ctz((unsigned) group_);
    const uint32_t grid = std::min(grid_of((uint64_t) n * group_), kMaxBlocks);
    if (neg_mode_ == MFX_BPR_NEG_WARP) hipLaunchKernelGGL(k_bpr_trials<MFX_BPR_NEG_WARP>, dim3(grid), dim3(kThreads), 0, st_, a);
    else hipLaunchKernelGGL(k_bpr_trials<MFX_BPR_NEG_HARDEST>, dim3(grid), dim3(kThreads), 0, st_, a);
    MFX_LAUNCH_CHECK();
    return MFX_OK;
}

// ---------------------------------------------------------------------------------------------- the single operator
int bpr_apply_neg(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i, int64_t negatives,
                  const uint32_t* items, const uint8_t* member, int mode, const float* rank_weight, float lr, float lambda, int64_t stats[4],
                  uint32_t* j_out, uint32_t* t_out, int device) {
    const char* fn = "mfx_bpr_apply_neg";
    MFX_REQUIRE(k >= 1 && k <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k);
    MFX_REQUIRE(n >= 0 && n <= kBprMaxBatch, "%s: n must be in [0, 2^20] (got %lld)", fn, (long long) n);
    MFX_REQUIRE(std::isfinite(lr) && lr >= 0.f, "%s: lr must be finite and >= 0 (got %g)", fn, (double) lr);
    MFX_REQUIRE(std::isfinite(lambda) && lambda >= 0.f, "%s: lambda must be finite and >= 0 (got %g)", fn, (double) lambda);
    MFX_REQUIRE(rows >= 1 && cols >= 1 && rows < 0xFFFFFFFFll && cols < 0xFFFFFFFFll, "%s: rows and cols must be in [1, 2^32 - 1)", fn);
    MFX_REQUIRE(mode == MFX_BPR_NEG_HARDEST || mode == MFX_BPR_NEG_WARP, "%s: mode must be 1 (hardest) or 2 (WARP) (got %d)", fn, mode);
    MFX_TRY(bpr_check_neg(fn, mode, negatives, rank_weight));
    MFX_REQUIRE(W && H && stats, "%s: W, H or stats is NULL", fn);
    MFX_REQUIRE(n == 0 || (u && i && items), "%s: u, i or items is NULL", fn);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (n == 0) return MFX_OK;
    BprCore core;
    MFX_TRY(core.init(rows, cols, k, n, device));
    MFX_TRY(core.init_neg(mode, (int) negatives, rank_weight));
    hipStream_t st = core.st_;
    const size_t nt = (size_t) n * (size_t) negatives;
    DevBuf<uint32_t> d_items, bad;
    DevBuf<uint8_t> d_member;
    MFX_TRY(d_items.alloc(nt));
    MFX_TRY(core.u_.upload(u, (size_t) n, MFX_HOST, st));
    MFX_TRY(core.i_.upload(i, (size_t) n, MFX_HOST, st));
    MFX_TRY(d_items.upload(items, nt, MFX_HOST, st));
    if (member) {
        MFX_TRY(d_member.alloc(nt));
        MFX_TRY(d_member.upload(member, nt, MFX_HOST, st));
    }
    MFX_HIP(hipMemsetAsync(core.j_.get(), 0, sizeof(uint32_t) * (size_t) n, st));
    MFX_TRY(bad.alloc(1));
    MFX_HIP(hipMemsetAsync(bad.get(), 0xFF, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_bpr_check_trials, dim3(grid_of((uint64_t) nt)), dim3(kThreads), 0, st, core.u_.get(), core.i_.get(), d_items.get(),
                       (uint32_t) n, (uint32_t) negatives, (uint32_t) rows, (uint32_t) cols, bad.get());
    MFX_LAUNCH_CHECK();
    uint32_t first_bad = kNoSlot;
    MFX_HIP(hipMemcpyAsync(&first_bad, bad.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_REQUIRE(first_bad == kNoSlot, "%s: slot %u names a user >= rows or an item >= cols", fn, first_bad);
    MFX_TRY(core.upload(W, H, MFX_HOST));
    MFX_TRY(core.trials((uint32_t) n, d_items.get(), member ? d_member.get() : nullptr, 0, 0, nullptr, nullptr));
    MFX_TRY(core.step((uint32_t) n, lr, lambda));
    unsigned long long h[4] = {0, 0, 0, 0};
    MFX_HIP(hipMemcpyAsync(h, core.stats_.get(), sizeof(h), hipMemcpyDeviceToHost, st));
    if (j_out) MFX_HIP(hipMemcpyAsync(j_out, core.j_.get(), sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
    if (t_out) MFX_HIP(hipMemcpyAsync(t_out, core.t_.get(), sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost, st));
    MFX_TRY(core.download(W, H, MFX_HOST));
    stats[0] = n;
    for (int q = 1; q < 4; ++q) stats[q] = (int64_t) h[q];
    return MFX_OK;
}

}  // namespace mfx
