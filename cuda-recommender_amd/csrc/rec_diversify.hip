// rec_diversify.hip -- diversity re-ranking of given candidate lists by greedy maximal marginal relevance
// (mfx_rec_diversify) on gfx950.  The rule is in include/mfx.h; DESIGN 5.14 has the measurements.
//
// Slot q names a user (or brings its own query vector) and a strictly ascending list of at most kCandChunk item ids.
// Every number of the rule is an explicit fp32 operation in a fixed order, so the picks are determined bit for bit:
// the relevance is the lane-owned FMA chain of mfx_cand_topn, the similarity the same chain between two rows of hq_.
//
//   mfx_div_maxlen   the longest list of the batch: it sizes the workgroups and the LDS of the two kernels below.
//   mfx_div_pack_wq  query vectors [nu][k] into rows of kt floats, +0 behind k: the shape of a packed row of W.
//   mfx_div_rel      one workgroup per slot: scores the list (one candidate per lane and step), drops the excluded,
//                    filtered and NaN candidates and leaves (rel, id) of the eligible ones compacted, in list order, at the
//                    list's own place in a workspace, and their number.
//   mfx_div_select   one workgroup per slot: rel, D, c and the ids of the eligible candidates in LDS (16 bytes each), then
//                    min(n_top, eligible) dependent steps: every thread takes the best of the candidates it owns
//                    (e = tid, tid + T, ...) under the total order (value, rel, position), a shuffle reduction and one
//                    barrier make the workgroup's pick known to all, the owner of the pick writes it out and retires it
//                    (D = NaN marks a picked candidate: D is never NaN otherwise), and every other candidate runs one chain
//                    against the picked row and raises its D.  A thread is the only reader and writer of its candidates'
//                    D, and the reduction scratch alternates between two halves, so a step has one barrier.
//                    FORM 1: the eligible rows are staged once into LDS (row stride kt + 4 floats: the 16-byte reads of
//                    16 consecutive rows hit 64 distinct banks) and both operands of a chain come from there.
//                    FORM 2: the candidate's row is re-read from hq_ at every step, the picked row is a uniform address.
//
// A workgroup of either kernel has one wave per 64 candidates of the batch's longest list, four at most: at 100 candidates
// two waves, and a barrier joins two waves instead of four (DESIGN 5.14 has the measurement against a fixed 256 threads).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "rec_cand.hpp"
#include "recommend.hpp"

namespace mfx {

namespace {

constexpr int kDivMaxTop = 128;
// Dynamic LDS of a workgroup of mfx_div_select: with its 96 static bytes, what a kernel may use without raising the limit
// of the function (64 KiB).  A CU has 160 KiB, so a workgroup that uses all of the budget leaves room for a second one;
// FORM 1 at 100 candidates takes 29 KiB at k = 64 (five workgroups per CU) and 54 KiB at k = 128 (two).
constexpr size_t kDivLdsBudget = 64 * 1024 - 256;

struct DivArgs {
    const float* wq;           // [rows][kt] the packed W, or the packed query vectors [nu][kt]
    const float* hq;           // [cols][kt]
    const float* cnorm;        // [cols] 1 / sqrt(n2) (cosine), NULL: dot
    const uint32_t* users;     // NULL: slot q takes row q of wq
    const uint32_t* ptr;       // [nu + 1]
    const uint32_t* idx;
    const uint32_t* ex_ptr;    // NULL: no exclusion
    const uint32_t* ex_idx;
    const float* fac;          // NULL, or [nblk * 32]: 1 / NaN per item (the item filter)
    int k, kt, n_top;
    int cap;                   // entries of each LDS array of mfx_div_select: the longest list rounded up to 64
    int ks;                    // FORM 1: floats between two staged rows
    float a, b;                // tradeoff and fp32(1 - tradeoff)
    uint32_t q0;               // first slot of this launch
    float* ws_rel;             // [total]: the eligible candidates of slot q from ptr[q] on
    uint32_t* ws_id;
    uint32_t* nel;             // [nu]
    uint32_t* out_items;       // [nu][n_top]
    float* out_scores;         // may be NULL
    float* out_values;         // may be NULL
};

__device__ __forceinline__ float div_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// The total order of a step: the greater value (NaN already taken as -inf), then the greater rel, then the earlier position
// in the list, which is the smaller item id.  (kPad as the position: nothing yet; a real candidate wins the tie against it.)
__device__ __forceinline__ bool div_better(float av, float ar, uint32_t ap, float bv, float br, uint32_t bp) {
    return (av > bv) | ((av == bv) & ((ar > br) | ((ar == br) & (ap < bp))));
}

// lane_chain with both rows in LDS (FORM 1): the same operations in the same order, eight 16-byte reads of each row in flight
// instead of four -- a workgroup that holds its rows in LDS leaves few waves per SIMD to hide their latency.
__device__ __forceinline__ float lds_chain(const float* hj, const float* hi, int k, int ks) {
    float acc = 0.f;
    int t = 0;
    if ((ks & 3) == 0) {
#pragma unroll 8
        for (; t + 4 <= k; t += 4) {
            const f32x4 h = *reinterpret_cast<const f32x4*>(hi + t);
            const f32x4 w = *reinterpret_cast<const f32x4*>(hj + t);
            acc = __builtin_fmaf(h.x, w.x, acc);
            acc = __builtin_fmaf(h.y, w.y, acc);
            acc = __builtin_fmaf(h.z, w.z, acc);
            acc = __builtin_fmaf(h.w, w.w, acc);
        }
    }
    for (; t < k; ++t) acc = __builtin_fmaf(hi[t], hj[t], acc);
    return acc;
}

__global__ void mfx_div_maxlen(const uint32_t* ptr, uint32_t nu, uint32_t* out) {
    uint32_t m = 0;
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < nu; q += (size_t) gridDim.x * blockDim.x)
        m = max(m, ptr[q + 1] - ptr[q]);  // (a decreasing pair wraps to a long list; the check of the pointers refuses it first)
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t) __shfl_xor((int) m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

__global__ void mfx_div_pack_wq(const float* src, size_t n, int k, int kt, float* dst) {
    for (size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t) gridDim.x * blockDim.x) {
        const size_t q = p / kt;
        const int t = (int) (p - q * kt);
        dst[p] = t < k ? src[q * k + t] : 0.f;
    }
}

__global__ __launch_bounds__(kCandThreads) void mfx_div_rel(DivArgs a) {
    __shared__ int wcnt[kCandWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = blockDim.x >> 6;
    const uint32_t q = a.q0 + blockIdx.x;
    const uint32_t lo = a.ptr[q], n = a.ptr[q + 1] - lo;
    const uint32_t u = __builtin_amdgcn_readfirstlane(a.users ? a.users[q] : q);  // (one slot per workgroup: the query row is a scalar operand)
    const float* wr = a.wq + (size_t) u * a.kt;
    uint32_t elo = 0, ehi = 0;
    if (a.ex_ptr) { elo = a.ex_ptr[u]; ehi = a.ex_ptr[u + 1]; }
    uint32_t done = 0;  // eligible candidates before this round (uniform)
    for (uint32_t base = 0; base < n; base += blockDim.x) {  // (uniform in the workgroup)
        const uint32_t c = base + tid;
        const bool valid = c < n;
        const uint32_t item = valid ? a.idx[lo + c] : 0;
        const float s = lane_chain(wr, a.hq + (size_t) item * a.kt, a.k, a.kt);
        const float key = a.fac ? s * a.fac[item] : s;
        const bool ok = valid && key == key && !(ehi > elo && excluded(a.ex_idx, elo, ehi, item));
        const unsigned long long m = __ballot(ok);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        uint32_t pos = done + __popcll(m & ((1ull << lane) - 1));
        for (int w = 0; w < nw; ++w) {
            const uint32_t cw = (uint32_t) wcnt[w];
            if (w < wave) pos += cw;
            done += cw;
        }
        if (ok) {
            a.ws_rel[lo + pos] = s;
            a.ws_id[lo + pos] = item;
        }
        __syncthreads();  // (wcnt is rewritten)
    }
    if (tid == 0) a.nel[q] = done;
}

template <int FORM>
__global__ __launch_bounds__(kCandThreads) void mfx_div_select(DivArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float red_v[2][kCandWaves], red_r[2][kCandWaves];
    __shared__ uint32_t red_p[2][kCandWaves];
    float* rel = lds;
    float* D = rel + a.cap;
    float* cn = D + a.cap;
    uint32_t* ids = reinterpret_cast<uint32_t*>(cn + a.cap);
    float* rows = reinterpret_cast<float*>(ids + a.cap);  // FORM 1: [ne][ks]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, T = blockDim.x, nw = T >> 6;
    const uint32_t q = a.q0 + blockIdx.x;
    const uint32_t lo = a.ptr[q];
    const int ne = (int) a.nel[q];
    const int k = a.k, kt = a.kt, ks = FORM == 1 ? a.ks : a.kt;
    for (int e = tid; e < ne; e += T) {
        const uint32_t item = a.ws_id[lo + e];
        rel[e] = a.ws_rel[lo + e];
        ids[e] = item;
        D[e] = 0.f;
        cn[e] = a.cnorm ? a.cnorm[item] : 0.f;
    }
    if (FORM == 1) {
        __syncthreads();
        if ((kt & 3) == 0) {
            // eight lanes per 128-byte line of a row, T / 8 rows per pass, four passes in flight per thread
            const int v = kt >> 2, sub = tid & 7, rpp = T >> 3;
            for (int e0 = tid >> 3; e0 < ne; e0 += 4 * rpp) {
                const float* src[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) src[i] = a.hq + (size_t) ids[min(e0 + i * rpp, ne - 1)] * kt;
                for (int j = sub; j < v; j += 8) {
                    f32x4 x[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const f32x4*>(src[i] + 4 * j);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (e0 + i * rpp < ne) *reinterpret_cast<f32x4*>(rows + (size_t) (e0 + i * rpp) * ks + 4 * j) = x[i];
                }
            }
        } else {
            for (int x = tid; x < ne * kt; x += T) {
                const int e = x / kt, j = x - e * kt;
                rows[(size_t) e * ks + j] = a.hq[(size_t) ids[e] * kt + j];
            }
        }
    }
    __syncthreads();

    const size_t o = (size_t) q * a.n_top;
    const int steps = ne < a.n_top ? ne : a.n_top;
    const float nb = -a.b;
    for (int s = 0; s < steps; ++s) {
        float bv = -INFINITY, br = -INFINITY;
        uint32_t bp = kPad;
        for (int e = tid; e < ne; e += T) {
            const float d = D[e];
            if (d != d) continue;  // picked before
            const float r = rel[e];
            const float raw = __builtin_fmaf(nb, d, div_mul(a.a, r));
            const float v = raw == raw ? raw : -INFINITY;
            if (div_better(v, r, (uint32_t) e, bv, br, bp)) { bv = v; br = r; bp = (uint32_t) e; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off), orr = __shfl_xor(br, off);
            const uint32_t op = (uint32_t) __shfl_xor((int) bp, off);
            if (div_better(ov, orr, op, bv, br, bp)) { bv = ov; br = orr; bp = op; }
        }
        const int h = s & 1;
        if (lane == 0) { red_v[h][wave] = bv; red_r[h][wave] = br; red_p[h][wave] = bp; }
        __syncthreads();
        for (int w = 0; w < nw; ++w) {
            const float ov = red_v[h][w], orr = red_r[h][w];
            const uint32_t op = red_p[h][w];
            if (div_better(ov, orr, op, bv, br, bp)) { bv = ov; br = orr; bp = op; }
        }
        const int p = (int) __builtin_amdgcn_readfirstlane(bp);  // (steps <= ne: there is an unpicked candidate, so p is one)
        const uint32_t pj = __builtin_amdgcn_readfirstlane(ids[p]);
        const float cj = cn[p];
        const float* hj = FORM == 1 ? rows + (size_t) p * ks : a.hq + (size_t) pj * kt;
        const bool last = s + 1 == steps;
        for (int e = tid; e < ne; e += T) {
            const float d = D[e];
            if (d != d) continue;
            if (e == p) {
                const float r = rel[e];
                a.out_items[o + s] = pj;
                if (a.out_scores) a.out_scores[o + s] = r;
                if (a.out_values) a.out_values[o + s] = __builtin_fmaf(nb, d, div_mul(a.a, r));
                D[e] = __builtin_nanf("");
                continue;
            }
            if (last) continue;
            const float* hi = FORM == 1 ? rows + (size_t) e * ks : a.hq + (size_t) ids[e] * kt;
            float sim = FORM == 1 ? lds_chain(hj, hi, k, ks) : lane_chain(hj, hi, k, ks);
            if (a.cnorm) sim = div_mul(div_mul(sim, cn[e]), cj);
            if (sim > d) D[e] = sim;  // (a NaN similarity leaves D as it was)
        }
    }
    for (int e = steps + tid; e < a.n_top; e += T) {
        a.out_items[o + e] = kPad;
        if (a.out_scores) a.out_scores[o + e] = -INFINITY;
        if (a.out_values) a.out_values[o + e] = -INFINITY;
    }
}

// Threads of a workgroup: one wave per 64 candidates of the longest list, unless MFX_DIV_THREADS = 64 / 128 / 192 / 256
// forces a size -- the hook of tools/diversify_bench.py, which records what the rule is worth; the results are the same bits.
int div_threads(uint32_t longest) {
    const char* v = std::getenv("MFX_DIV_THREADS");
    const int forced = v ? std::atoi(v) : 0;
    if (forced == 64 || forced == 128 || forced == 192 || forced == 256) return forced;
    return (int) std::min<uint32_t>(kCandThreads, std::max<uint32_t>(64, (longest + 63) / 64 * 64));
}

}  // namespace

int Recommender::diversify(int64_t nusers, const uint32_t* users, const float* Wq, const uint32_t* cand_ptr, const uint32_t* cand_idx,
                           int32_t flags, int metric, float tradeoff, int32_t n_top, uint32_t* items, float* scores, float* values,
                           uint32_t* n_eligible, mfx_memspace space, int form) {
    const char* fn = "mfx_rec_diversify";
    MFX_REQUIRE(n_top >= 1 && n_top <= kDivMaxTop, "%s: n_top must be in [1, %d] (got %d)", fn, kDivMaxTop, n_top);
    MFX_REQUIRE(nusers >= 0 && nusers < (int64_t) 0xFFFFFFFFll, "%s: bad nusers %lld", fn, (long long) nusers);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    MFX_REQUIRE((flags & ~MFX_DIV_NO_EXCLUDE) == 0, "%s: unknown flag bits 0x%x", fn, (unsigned) flags);
    MFX_REQUIRE(metric == MFX_SIM_DOT || metric == MFX_SIM_COSINE, "%s: unknown metric %d", fn, metric);
    MFX_REQUIRE(std::isfinite(tradeoff) && tradeoff >= 0.f && tradeoff <= 1.f, "%s: tradeoff must be in [0, 1] (got %g)", fn, (double) tradeoff);
    MFX_REQUIRE(form >= 0 && form <= 2, "%s: form must be 0, 1 or 2 (got %d)", fn, form);
    MFX_REQUIRE(k_ >= 1 && k_ <= 1024, "%s: k must be in [1, 1024] (got %lld)", fn, (long long) k_);
    MFX_REQUIRE(!Wq || !users, "%s: Wq takes the place of the rows of W: users must be NULL with it", fn);
    MFX_REQUIRE(!Wq || (flags & MFX_DIV_NO_EXCLUDE), "%s: Wq has no exclusion rows: it needs the flag MFX_DIV_NO_EXCLUDE", fn);
    MFX_REQUIRE(users || Wq || nusers <= rows_, "%s: users = NULL needs nusers <= rows (%lld > %lld)", fn, (long long) nusers, (long long) rows_);
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(cand_ptr, "%s: cand_ptr is NULL", fn);
    MFX_REQUIRE(items, "%s: items is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const uint32_t nu = (uint32_t) nusers;
    const bool host = space == MFX_HOST;
    div_s_[0] = div_s_[1] = div_s_[2] = 0.0;
    Events ev;
    MFX_TRY(ev.create());
    MFX_HIP(hipEventRecord(ev.e[0], st));

    DevBuf<uint32_t> d_users, d_longest, ws_id, d_nel, d_items;
    DevBuf<float> wq_in, wq, ws_rel, d_scores, d_values;
    CandLists lists;
    const uint32_t* du = nullptr;
    MFX_TRY(stage_ids(users, nu, space, (uint32_t) rows_, "mfx_rec_diversify: user id", d_users, &du));
    MFX_TRY(cand_stage(fn, nu, cand_ptr, cand_idx, space, lists));
    uint32_t longest = 0;  // (arrives with the read-back of the checks, on the same stream)
    MFX_TRY(d_longest.alloc_zero(1, st));
    hipLaunchKernelGGL(mfx_div_maxlen, dim3(grid_for(nu)), dim3(256), 0, st, lists.ptr, nu, d_longest.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipMemcpyAsync(&longest, d_longest.get(), sizeof(longest), hipMemcpyDeviceToHost, st));
    const int checked = cand_check(fn, nu, lists);
    if (checked != MFX_OK) {
        (void) hipStreamSynchronize(st);  // (the copy into `longest` may be under way)
        return checked;
    }
    if (lists.nlong) {
        std::vector<uint32_t> slots(lists.nlong);
        MFX_HIP(hipMemcpy(slots.data(), lists.long_list.get(), sizeof(uint32_t) * lists.nlong, hipMemcpyDeviceToHost));
        return fail(MFX_ERR_INVALID, "%s: the list of slot %u holds more than %d candidates", fn, *std::min_element(slots.begin(), slots.end()),
                    kCandChunk);
    }
    const uint32_t total = lists.total;
    const int cap = (int) std::max<uint32_t>(64, (longest + 63) / 64 * 64);
    const int ks = (kt_ & 3) == 0 ? kt_ + 4 : kt_;
    const size_t lds2 = (size_t) cap * 16, lds1 = lds2 + (size_t) longest * ks * sizeof(float);
    MFX_REQUIRE(form != 1 || lds1 <= kDivLdsBudget,
                "%s: form 1 stages the rows in LDS: lists of %u candidates at k = %lld need %zu bytes, the budget is %zu", fn, longest,
                (long long) k_, lds1, kDivLdsBudget);
    if (form == 0) form = lds1 <= kDivLdsBudget ? 1 : 2;
    MFX_TRY(similar_setup());  // (idempotent) hq_ and the inverse norms

    const float* dwq = wp_.get();
    if (Wq) {
        const float* src = Wq;
        if (host) {
            MFX_TRY(wq_in.alloc((size_t) nu * k_));
            MFX_TRY(wq_in.upload(Wq, (size_t) nu * k_, MFX_HOST, st));
            src = wq_in.get();
        }
        const size_t n = (size_t) nu * kt_;
        MFX_TRY(wq.alloc(n));
        hipLaunchKernelGGL(mfx_div_pack_wq, dim3(grid_for(n)), dim3(256), 0, st, src, n, (int) k_, kt_, wq.get());
        MFX_LAUNCH_CHECK();
        dwq = wq.get();
    }
    MFX_TRY(ws_rel.alloc(total));
    MFX_TRY(ws_id.alloc(total));
    MFX_TRY(d_nel.alloc(nu));
    uint32_t* oi = items;
    float* os = scores;
    float* ov = values;
    if (host) {
        MFX_TRY(d_items.alloc((size_t) nu * n_top));
        oi = d_items.get();
        if (scores) { MFX_TRY(d_scores.alloc((size_t) nu * n_top)); os = d_scores.get(); }
        if (values) { MFX_TRY(d_values.alloc((size_t) nu * n_top)); ov = d_values.get(); }
    }
    MFX_HIP(hipEventRecord(ev.e[1], st));

    DivArgs a{};
    a.wq = dwq; a.hq = hq_.get();
    a.cnorm = metric == MFX_SIM_COSINE ? sim_c_.get() : nullptr;
    a.users = du; a.ptr = lists.ptr; a.idx = lists.idx;
    const bool ex = has_ex_ && !(flags & MFX_DIV_NO_EXCLUDE);
    a.ex_ptr = ex ? ex_ptr_.get() : nullptr; a.ex_idx = ex_idx_.get();
    a.fac = fac_keep_.get();
    a.k = (int) k_; a.kt = kt_; a.n_top = n_top;
    a.cap = cap; a.ks = ks;
    a.a = tradeoff; a.b = 1.f - tradeoff;
    a.ws_rel = ws_rel.get(); a.ws_id = ws_id.get(); a.nel = d_nel.get();
    a.out_items = oi; a.out_scores = os; a.out_values = ov;
    const dim3 block((uint32_t) div_threads(longest));
    for (uint64_t q0 = 0; q0 < nu; q0 += 1u << 30) {  // (grid.x stays below 2^31)
        a.q0 = (uint32_t) q0;
        hipLaunchKernelGGL(mfx_div_rel, dim3((uint32_t) std::min<uint64_t>(nu - q0, 1u << 30)), block, 0, st, a);
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipEventRecord(ev.e[2], st));
    for (uint64_t q0 = 0; q0 < nu; q0 += 1u << 30) {
        a.q0 = (uint32_t) q0;
        const dim3 grid((uint32_t) std::min<uint64_t>(nu - q0, 1u << 30));
        if (form == 1) hipLaunchKernelGGL((mfx_div_select<1>), grid, block, lds1, st, a);
        else hipLaunchKernelGGL((mfx_div_select<2>), grid, block, lds2, st, a);
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipEventRecord(ev.e[3], st));
    const hipMemcpyKind back = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (host) {
        MFX_HIP(hipMemcpyAsync(items, oi, sizeof(uint32_t) * nu * n_top, back, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, os, sizeof(float) * nu * n_top, back, st));
        if (values) MFX_HIP(hipMemcpyAsync(values, ov, sizeof(float) * nu * n_top, back, st));
    }
    if (n_eligible) MFX_HIP(hipMemcpyAsync(n_eligible, d_nel.get(), sizeof(uint32_t) * nu, back, st));
    MFX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        MFX_HIP(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        div_s_[i] = 1e-3 * ms;
    }
    return MFX_OK;
}

}  // namespace mfx
