// rec_rank.hip -- exact catalogue ranks of given (user, item) pairs (mfx_rec_rank) and full-rank evaluation
// (mfx_rec_evaluate) on gfx950.
//
// The rank of pair (u, i) is the number of items eligible for u that order before i in the total order of mfx_rec_query
// (key descending, then item ascending; -0 == +0; NaN keys are never eligible), so it is the position at which a query
// for u returns i.  Three kernels, no list, no sort:
//
//   mfx_rec_target_keys   one thread per pair: the score of (u, i) as the explicit fp32 FMA chain over t ascending from
//                         the packed W and the rows of H read back from the tiles (the bits the MFMA chain gives, as
//                         mfx_rec_item_norms relies on), times the item's factor when a filter is set: the pair's key.
//   mfx_rec_count         the tile pass of rec_tiles.hpp that mfx_rec_topn runs (128 slots x one item slice per
//                         workgroup), with a count in the place of the selection.  A slot is a pair; its lane carries
//                         the target's key and id and two counters, and every score costs a NaN test and the order
//                         compare: how many items with a non-NaN key, how many of them before the target.  Item slices
//                         add into the pair's counters with integer atomics, which no order can change.
//   mfx_rec_rank_fix      one wave per pair walks the user's exclusion row: every distinct id with a non-NaN key leaves
//                         the eligible count, every one that orders before the target leaves the rank, and the target
//                         found in the row, or a NaN target key, makes the pair ineligible (rank 0xFFFFFFFF).
//
// A slot per pair rather than per user with several targets in registers: the pass is then independent of how the
// batch groups its users, and the per-score work stays two compares; a user with t targets costs t slots.
//
// mfx_rec_evaluate builds the distinct (user, item) pairs of the held-out set on the host, ranks them in one
// mfx_rec_rank, and forms every metric in fp64 on the host from the ranks and eligible counts alone.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rec_tiles.hpp"
#include "recommend.hpp"

namespace mfx {

namespace {

struct RankArgs : TileArgs {
    const uint32_t* users;   // [np]
    const uint32_t* items;   // [np]
    const float* tkey;       // [np] key of the pair's target
    uint32_t np;
    uint32_t* cnt;           // [np][2]: items with a non-NaN key, items ordered before the target (zeroed; slices add)
};

// The score chain of a packed W row and a row of H read back from the tiles (hq: [cols][kt], the bits of the tiles): fma over
// t = 0 .. k-1 ascending from +0.  A row is contiguous, so a lane's gather is k / 4 16-byte loads from two or three cache
// lines rather than k lines of the tile layout.
__device__ inline float chain_score(const float* wr, const float* hr, int k, int kt) {
    float acc = 0.f;
    int t = 0;
    if ((kt & 3) == 0) {  // (rows are 16-byte aligned)
        for (; t + 4 <= k; t += 4) {
            const float4 h = *reinterpret_cast<const float4*>(hr + t);
            acc = __builtin_fmaf(h.x, wr[t], acc);
            acc = __builtin_fmaf(h.y, wr[t + 1], acc);
            acc = __builtin_fmaf(h.z, wr[t + 2], acc);
            acc = __builtin_fmaf(h.w, wr[t + 3], acc);
        }
    }
    for (; t < k; ++t) acc = __builtin_fmaf(hr[t], wr[t], acc);
    return acc;
}

__global__ void mfx_rec_target_keys(const float* wp, const float* hq, const uint32_t* users, const uint32_t* items, uint32_t np,
                                    int k, int kt, const float* fac, float* tkey, float* scores) {
    for (size_t p = (size_t) blockIdx.x * blockDim.x + threadIdx.x; p < np; p += (size_t) gridDim.x * blockDim.x) {
        const uint32_t item = items[p];
        const float s = chain_score(wp + (size_t) users[p] * kt, hq + (size_t) item * kt, k, kt);
        if (scores) scores[p] = s;
        tkey[p] = fac ? s * fac[item] : s;
    }
}

template <int KC, bool FAC>
__global__ __launch_bounds__(kRecThreads) void mfx_rec_count(RankArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const uint32_t q = blockIdx.x * kRecUsers + wave * 32 + j;
    const bool valid = q < a.np;
    const uint32_t u = valid ? a.users[q] : 0;
    const uint32_t ti = valid ? a.items[q] : 0;
    const float tk = valid ? a.tkey[q] : 0.f;
    uint32_t elig = 0, before = 0;
    rec_tile_pass<KC, FAC>(a, (int) blockIdx.y, u, valid, [&](uint32_t ibase, const f32x16& acc) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t item = acc_item(ibase, r);
            const float key = acc[r];
            const bool in = item < a.cols;  // (the packed padding past cols scores 0, not NaN)
            elig += (uint32_t) (in & (key == key));  // (&: no branch per entry)
            before += (uint32_t) (in & beats(key, item, tk, ti));
        }
    });
    elig += __shfl_xor(elig, 32);
    before += __shfl_xor(before, 32);
    if (valid && h == 0) {
        atomicAdd(a.cnt + 2 * (size_t) q, elig);
        atomicAdd(a.cnt + 2 * (size_t) q + 1, before);
    }
}

// One wave per pair: the exclusion row of the pair's user comes off the counts, and the pair's results are written.
__global__ __launch_bounds__(kRecThreads) void mfx_rec_rank_fix(const float* wp, const float* hq, const uint32_t* users,
                                                                const uint32_t* items, const float* tkey, const uint32_t* cnt,
                                                                uint32_t np, int k, int kt, const uint32_t* ex_ptr,
                                                                const uint32_t* ex_idx, const float* fac, uint32_t* ranks,
                                                                uint32_t* n_eligible) {
    const int lane = threadIdx.x & 63;
    const size_t p = (size_t) blockIdx.x * kRecWaves + (threadIdx.x >> 6);
    if (p >= np) return;
    const uint32_t u = __builtin_amdgcn_readfirstlane(users[p]), ti = items[p];  // (one pair per wave: the W row is a scalar operand)
    const float tk = tkey[p];
    int de = 0, db = 0, hit = 0;
    if (ex_ptr) {
        const uint32_t lo = ex_ptr[u], hi = ex_ptr[u + 1];
        const float* wr = wp + (size_t) u * kt;
        for (uint32_t x = lo + lane; x < hi; x += 64) {
            const uint32_t e = ex_idx[x];
            if (x > lo && ex_idx[x - 1] == e) continue;  // (ids are non-decreasing within a row: a repeated id counts once)
            float key = chain_score(wr, hq + (size_t) e * kt, k, kt);
            if (fac) key *= fac[e];
            de += key == key;
            db += beats(key, e, tk, ti);
            hit |= e == ti;
        }
    }
    de = wave_sum(de);
    db = wave_sum(db);
    hit = wave_sum(hit);
    if (lane == 0) {
        ranks[p] = (hit || tk != tk) ? kPad : cnt[2 * p + 1] - (uint32_t) db;
        if (n_eligible) n_eligible[p] = cnt[2 * p] - (uint32_t) de;
    }
}

struct Events {  // four stream events around the three phases
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    int create() {
        for (auto& x : e) MFX_HIP(hipEventCreate(&x));
        return MFX_OK;
    }
    ~Events() {
        for (auto x : e)
            if (x) (void) hipEventDestroy(x);
    }
};

}  // namespace

int Recommender::rank(int64_t npairs, const uint32_t* users, const uint32_t* items, uint32_t* ranks, float* scores,
                      uint32_t* n_eligible, mfx_memspace space, int item_slices) {
    MFX_REQUIRE(npairs >= 0 && npairs < (int64_t) 0xFFFFFFFFll, "mfx_rec_rank: bad npairs %lld", (long long) npairs);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_rank: bad memory space");
    MFX_REQUIRE(item_slices >= 0, "mfx_rec_rank: item_slices must be >= 0 (got %d)", item_slices);
    if (npairs == 0) return MFX_OK;
    MFX_REQUIRE(users && items, "mfx_rec_rank: users or items is NULL");
    MFX_REQUIRE(ranks, "mfx_rec_rank: ranks is NULL");
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const uint32_t np = (uint32_t) npairs;
    const bool host = space == MFX_HOST;

    DevBuf<uint32_t> d_users, d_items, d_ranks, d_nel, cnt;
    DevBuf<float> d_scores, tkey;
    const uint32_t* du = nullptr;
    const uint32_t* di = nullptr;
    MFX_TRY(stage_ids(users, np, space, (uint32_t) rows_, "mfx_rec_rank: user id", d_users, &du));
    MFX_TRY(stage_ids(items, np, space, (uint32_t) cols_, "mfx_rec_rank: item id", d_items, &di));
    uint32_t* orank = ranks;
    float* oscore = scores;
    uint32_t* onel = n_eligible;
    if (host) {
        MFX_TRY(d_ranks.alloc(np));
        orank = d_ranks.get();
        if (scores) { MFX_TRY(d_scores.alloc(np)); oscore = d_scores.get(); }
        if (n_eligible) { MFX_TRY(d_nel.alloc(np)); onel = d_nel.get(); }
    }
    MFX_TRY(ensure_hq());
    MFX_TRY(tkey.alloc(np));
    MFX_TRY(cnt.alloc_zero((size_t) np * 2, st));
    Events ev;
    MFX_TRY(ev.create());

    const int slices = pick_slices(item_slices, ((int64_t) np + kRecUsers - 1) / kRecUsers, 65535);  // (grid.y)
    const int bps = (nblk_ + slices - 1) / slices;
    const float* fac = fac_keep_.get();

    MFX_HIP(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(mfx_rec_target_keys, dim3(grid_for(np)), dim3(256), 0, st, wp_.get(), hq_.get(), du, di, np, (int) k_, kt_, fac,
                       tkey.get(), oscore);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev.e[1], st));
    RankArgs a{};
    a.wp = wp_.get(); a.hp = hp_.get();
    a.users = du; a.items = di; a.tkey = tkey.get();
    a.np = np; a.cols = (uint32_t) cols_;
    a.kt = kt_; a.nch = nch_; a.nblk = nblk_; a.bps = bps;
    a.cnt = cnt.get();
    a.fac = fac;
    MFX_TRY(dispatch_kc(kc_, [&](auto kc) {
        const dim3 grid((np + kRecUsers - 1) / kRecUsers, slices);
        if (fac) hipLaunchKernelGGL((mfx_rec_count<decltype(kc)::value, true>), grid, dim3(kRecThreads), 0, st, a);
        else hipLaunchKernelGGL((mfx_rec_count<decltype(kc)::value, false>), grid, dim3(kRecThreads), 0, st, a);
        MFX_LAUNCH_CHECK();
        return (int) MFX_OK;
    }));
    MFX_HIP(hipEventRecord(ev.e[2], st));
    hipLaunchKernelGGL(mfx_rec_rank_fix, dim3((np + kRecWaves - 1) / kRecWaves), dim3(kRecThreads), 0, st, wp_.get(), hq_.get(), du, di,
                       tkey.get(), cnt.get(), np, (int) k_, kt_, has_ex_ ? ex_ptr_.get() : nullptr, ex_idx_.get(), fac,
                       orank, onel);
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipEventRecord(ev.e[3], st));
    if (host) {
        MFX_HIP(hipMemcpyAsync(ranks, orank, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, oscore, sizeof(float) * np, hipMemcpyDeviceToHost, st));
        if (n_eligible) MFX_HIP(hipMemcpyAsync(n_eligible, onel, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        MFX_HIP(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
        rank_s_[i] = 1e-3 * ms;
    }
    return MFX_OK;
}

int Recommender::evaluate(const mfx_coo* T, float min_rating, int32_t n_cut, const int32_t* cutoffs, double* out, double* mrr,
                          double* auc, int64_t* users_evaluated, int64_t* auc_users, mfx_memspace space) {
    MFX_REQUIRE(T && T->nnz >= 0 && T->nnz < (int64_t) 0xFFFFFFFFll, "mfx_rec_evaluate: bad test set");
    MFX_REQUIRE(T->nnz == 0 || (T->row && T->col && T->val), "mfx_rec_evaluate: null test array");
    MFX_REQUIRE(!std::isnan(min_rating), "mfx_rec_evaluate: min_rating is NaN");
    MFX_REQUIRE(n_cut >= 0 && (n_cut == 0 || (cutoffs && out)), "mfx_rec_evaluate: n_cut = %d needs cutoffs and out", n_cut);
    for (int32_t c = 0; c < n_cut; ++c) MFX_REQUIRE(cutoffs[c] >= 1, "mfx_rec_evaluate: cutoff %d is %d (>= 1 required)", c, cutoffs[c]);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_evaluate: bad memory space");
    MFX_TRY(use_device(device_));
    const size_t nnz = (size_t) T->nnz;
    std::vector<uint32_t> hr, hc;
    std::vector<float> hv;
    const uint32_t* row = T->row;
    const uint32_t* col = T->col;
    const float* val = T->val;
    if (space == MFX_DEVICE && nnz) {
        hr.resize(nnz); hc.resize(nnz); hv.resize(nnz);
        MFX_HIP(hipMemcpyAsync(hr.data(), T->row, sizeof(uint32_t) * nnz, hipMemcpyDeviceToHost, st_));
        MFX_HIP(hipMemcpyAsync(hc.data(), T->col, sizeof(uint32_t) * nnz, hipMemcpyDeviceToHost, st_));
        MFX_HIP(hipMemcpyAsync(hv.data(), T->val, sizeof(float) * nnz, hipMemcpyDeviceToHost, st_));
        MFX_HIP(hipStreamSynchronize(st_));
        row = hr.data(); col = hc.data(); val = hv.data();
    }
    // the distinct (user, item) pairs with value >= min_rating, by user: R_u is one run
    std::vector<uint64_t> pairs;
    pairs.reserve(nnz);
    for (size_t p = 0; p < nnz; ++p)
        if (val[p] >= min_rating) pairs.push_back((uint64_t) row[p] << 32 | col[p]);
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const size_t np = pairs.size();
    std::vector<uint32_t> pu(np), pi(np), ranks(np), nel(np);
    for (size_t p = 0; p < np; ++p) { pu[p] = (uint32_t) (pairs[p] >> 32); pi[p] = (uint32_t) pairs[p]; }
    MFX_TRY(rank((int64_t) np, pu.data(), pi.data(), ranks.data(), nullptr, nel.data(), MFX_HOST, 0));

    std::vector<TopnAcc> acc((size_t) n_cut);
    double mrr_sum = 0, auc_sum = 0;
    int64_t kept = 0, auc_kept = 0;
    std::vector<uint32_t> rk;
    for (size_t lo = 0; lo < np;) {
        size_t hi = lo + 1;
        while (hi < np && pu[hi] == pu[lo]) ++hi;
        const size_t nrel = hi - lo;
        rk.clear();
        for (size_t p = lo; p < hi; ++p)
            if (ranks[p] != kPad) rk.push_back(ranks[p]);
        std::sort(rk.begin(), rk.end());  // the eligible targets in ranking order: a_p is the index
        ++kept;
        for (int32_t c = 0; c < n_cut; ++c) {
            const size_t nh = std::lower_bound(rk.begin(), rk.end(), (uint32_t) cutoffs[c]) - rk.begin();
            acc[c].add(rk.data(), nh, nrel, cutoffs[c]);
        }
        if (!rk.empty()) {
            mrr_sum += 1.0 / (1.0 + (double) rk[0]);
            const double neg = (double) nel[lo] - (double) rk.size();
            if (neg > 0) {
                double s = 0;
                for (size_t x = 0; x < rk.size(); ++x) s += (neg - ((double) rk[x] - (double) x)) / neg;
                auc_sum += s / (double) rk.size();
                ++auc_kept;
            }
        }
        lo = hi;
    }
    for (int32_t c = 0; c < n_cut; ++c) acc[c].mean(out + 4 * (size_t) c);
    if (mrr) *mrr = kept ? mrr_sum / (double) kept : 0.0;
    if (auc) *auc = auc_kept ? auc_sum / (double) auc_kept : 0.0;
    if (users_evaluated) *users_evaluated = kept;
    if (auc_users) *auc_users = auc_kept;
    return MFX_OK;
}

}  // namespace mfx
