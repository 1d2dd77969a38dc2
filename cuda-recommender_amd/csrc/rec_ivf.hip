// rec_ivf.hip -- inverted-file retrieval for the recommender on gfx950 (mfx_rec_ivf_*, mfx_rec_query_ivf): the first stage
// that mfx_rec_query_candidates is the second stage of.
//
// The items are partitioned into nlist lists, each with a centroid (the caller's clustering: mfx_rec_ivf_setup takes any
// assignment).  A query scores the user against the centroids, takes the best nprobe lists, and ranks only the items of
// those lists; its result is by definition that of mfx_rec_query_candidates on the ascending union of the probed lists.
//
// State (IvfIndex): a second packed copy of H in list order, every list starting on a tile and padded to whole tiles, so a
// tile never holds items of two lists and a list is a contiguous run of tiles that rec_tile_pass of rec_tiles.hpp walks
// unchanged; the position -> item id table; the first tile of every list; the centroids packed like H.  The copy is built
// from the handle's own tiles, so a score has the bits mfx_rec_query gives it.
//
// A query is five steps on the stream:
//   probe             mfx_rec_topn of recommend.hip with the centroids as the items: [slot][nprobe] list ids.
//   mfx_ivf_count     the number of (slot, probe position) pairs per list.  A pair without a list to pass (fewer than
//                     nprobe lists had a score, or the list is empty) writes its padding here: no work item will.
//   mfx_ivf_scan      work items per list, ceil(pairs / 128), and their prefix sum (one workgroup; nlist <= 65536).
//   mfx_ivf_scatter   every pair takes a place in a work item of its list by an integer atomic.  Which place it gets
//                     differs from run to run; no result depends on it, a slot's candidate list is its own.
//   mfx_ivf_topn      one workgroup per work item (list l, up to 128 pairs): the tile pass over the tiles of l with the
//                     lane's row its slot's user, and the selection of mfx_rec_topn (threshold, admission by >=, flush with
//                     the exclusion by binary search, bitonic sort) with the item id read from the id table where an entry
//                     is admitted: the candidate lists carry ids, so ties across lists order by id.  The pair's sorted
//                     best n_top go to [probe position][slot][L] of the workspace,
//   mfx_rec_merge     of recommend.hip with slices = nprobe finishes (nprobe = 1 writes the output from the pass).
// The grid of mfx_ivf_topn is the upper bound pairs / 128 + min(nlist, pairs) on the work items, so the count stays on the
// device; a workgroup past the count returns at once.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "ccd_kernels.hpp"  // check_index_range
#include "rec_tiles.hpp"
#include "recommend.hpp"

namespace mfx {

namespace {

constexpr int kScr = 256;                    // per-wave LDS sort scratch (entries), as in recommend.hip
constexpr int kMaxMerge = 8192;              // nprobe * n_top of one merge (mfx_rec_merge: 64 KiB of LDS)
constexpr int kMaxTop = 1024, kMaxList = 65536;
constexpr size_t kWorkspaceCap = size_t(1) << 30;  // candidate lists of one launch (users are chunked under this)
constexpr int kPosBits = 10;                 // a pair is slot << 10 | probe position: nprobe <= 1024, slots of a launch < 2^21

struct IvfArgs : TileArgs {   // hp / fac: the index's, whole; cols / nblk / bps are set per work item
    const uint32_t* users;    // NULL: slot q is user q0 + q
    uint32_t q0, nq;
    const uint32_t* ex_ptr;   // NULL: no exclusion
    const uint32_t* ex_idx;
    int n_top, L, nprobe;
    float* ls;                // [nprobe][nq][L] candidate lists
    uint32_t* li;
    uint32_t* out_items;      // [q0 + q][n_top], written by the pass when nprobe = 1
    float* out_scores;        // may be NULL
    const uint32_t* ids;      // [tiles * 32] position -> item id
    const uint32_t* blk_ptr;  // [nlist + 1]
    const uint32_t* list_ptr; // [nlist + 1]
    const uint32_t* wi_list;  // [work items]
    const uint32_t* wi_slot;  // [work items][128] pairs, kPad: none
    const uint32_t* nwi;      // work items built
};

__device__ inline void wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// wave_bitonic / excluded of recommend.hip
__device__ void wave_bitonic(float* ks, uint32_t* is, int P, int lane) {
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = lane; x < (P >> 1); x += 64) {
                const int a = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                const int b = a + j;
                const float sa = ks[a], sb = ks[b];
                const uint32_t ia = is[a], ib = is[b];
                const bool sw = (a & k) == 0 ? beats(sb, ib, sa, ia) : beats(sa, ia, sb, ib);
                if (sw) {
                    ks[a] = sb; ks[b] = sa;
                    is[a] = ib; is[b] = ia;
                }
            }
            wave_sync();
        }
    }
}

__device__ inline bool excluded(const uint32_t* ex, uint32_t lo, uint32_t hi, uint32_t item) {
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ex[mid] < item) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && ex[lo] == item;
}

// The list pass.  The sibling of mfx_rec_topn: the same list state and flush, with the slot and the probe position per lane
// instead of per workgroup, and positions turned into item ids on admission.  The positions of a list are valid below its
// item count (the padding of its last tile lies above), which is what `cols` is to mfx_rec_topn; the id table is read for
// admitted entries only, so the tile loop holds no more registers than mfx_rec_topn's.  waves_per_eu per KC:
// profiles/r23_ivf_resources.txt.
template <int KC, bool FAC>
__global__ __launch_bounds__(kRecThreads) __attribute__((amdgpu_waves_per_eu(KC <= 16 ? 4 : KC == 32 ? 3 : 1)))
void mfx_ivf_topn(IvfArgs a) {
    __shared__ float scs[kRecWaves][kScr];
    __shared__ uint32_t sci[kRecWaves][kScr];

    const uint32_t wi = blockIdx.x;
    if (wi >= *a.nwi) return;  // (uniform)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const uint32_t l = a.wi_list[wi];
    const uint32_t blk0 = a.blk_ptr[l];
    const uint32_t e = a.wi_slot[(size_t) wi * kRecUsers + wave * 32 + j];
    const bool uvalid = e != kPad;
    const uint32_t q = uvalid ? e >> kPosBits : 0, p = uvalid ? e & ((1u << kPosBits) - 1) : 0;
    const uint32_t u = uvalid ? (a.users ? a.users[a.q0 + q] : a.q0 + q) : 0;
    const size_t lbase = ((size_t) p * a.nq + q) * (size_t) a.L;
    const bool single = a.nprobe == 1;
    const bool lds_sort = a.L <= kScr;
    const uint32_t* idp = a.ids + (size_t) blk0 * kTile;

    const uint32_t nitems = a.list_ptr[l + 1] - a.list_ptr[l];
    TileArgs t = a;
    t.hp = a.hp + (size_t) blk0 * a.kt * kTile;
    t.cols = nitems;
    t.nblk = t.bps = (int) (a.blk_ptr[l + 1] - blk0);
    if (FAC) t.fac = a.fac + (size_t) blk0 * kTile;

    float thr = -INFINITY;  // score of the pair's N-th entry once it has N; admission is score >= thr
    int cnt = 0;            // entries in the pair's list
    int clean = 0;          // leading entries already checked against the exclusion row (the sorted top)

    // Filters, sorts and truncates the list of the pair on lane uj (the whole wave works on it).  fin: write the final N
    // entries (padded) to the output (nprobe = 1) or to the head of the list (merge input).
    auto flush = [&](int uj, bool fin) __attribute__((always_inline)) {
        const int c_u = __shfl(cnt, uj), cl_u = __shfl(clean, uj);
        const uint32_t uid = __shfl(u, uj), qu = __shfl(q, uj), pu = __shfl(p, uj);
        const size_t base = ((size_t) pu * a.nq + qu) * (size_t) a.L;
        int P = 1;
        while (P < c_u) P <<= 1;
        float* ks = lds_sort ? scs[wave] : a.ls + base;
        uint32_t* is = lds_sort ? sci[wave] : a.li + base;
        uint32_t elo = 0, ehi = 0;
        if (a.ex_ptr) { elo = a.ex_ptr[uid]; ehi = a.ex_ptr[uid + 1]; }
        wave_sync();
        int kept = 0;
        for (int x = lane; x < P; x += 64) {
            float s = -INFINITY;
            uint32_t it = kPad;
            if (x < c_u) {
                s = a.ls[base + x];
                it = a.li[base + x];
                if (x >= cl_u && ehi > elo && excluded(a.ex_idx, elo, ehi, it)) { s = -INFINITY; it = kPad; }
                else ++kept;
            }
            ks[x] = s;
            is[x] = it;
        }
        kept = wave_sum(kept);
        wave_sync();
        wave_bitonic(ks, is, P, lane);
        const int m = min(a.n_top, kept);
        if (fin) {
            for (int x = lane; x < a.n_top; x += 64) {
                float s = -INFINITY;
                uint32_t it = kPad;
                if (x < m) { s = ks[x]; it = is[x]; }
                if (single) {
                    const size_t o = (size_t) (a.q0 + qu) * a.n_top + x;
                    a.out_items[o] = it;
                    if (a.out_scores) a.out_scores[o] = s;
                } else {
                    a.ls[base + x] = s;
                    a.li[base + x] = it;
                }
            }
        } else if (lds_sort) {
            for (int x = lane; x < m; x += 64) { a.ls[base + x] = ks[x]; a.li[base + x] = is[x]; }
        }
        wave_sync();
        const float nthr = (!fin && m == a.n_top) ? ks[a.n_top - 1] : -INFINITY;
        if (j == uj) { cnt = m; clean = m; thr = nthr; }
        wave_sync();
    };

    rec_tile_pass<KC, FAC>(t, 0, u, uvalid, [&](uint32_t ibase, const f32x16& acc) __attribute__((always_inline)) {
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) mask |= (uint32_t) (uvalid && acc_item(ibase, r) < nitems && acc[r] >= thr) << r;
        if (__ballot(mask != 0)) {
            const int n = __popc(mask);
            const int n_o = __shfl_xor(n, 32);
            const int tot = n + n_o;
            uint64_t fm = __ballot(uvalid && h == 0 && cnt + tot > a.L);
            while (fm) {
                const int uj = __ffsll((unsigned long long) fm) - 1;
                fm &= fm - 1;
                flush(uj, false);
            }
            if (mask) {
                size_t pos = lbase + cnt + (h ? n_o : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (mask >> r & 1) {
                        a.ls[pos] = acc[r];
                        a.li[pos] = idp[acc_item(ibase, r)];
                        ++pos;
                    }
                }
            }
            cnt += tot;
        }
    });
    uint64_t fm = __ballot(uvalid && h == 0);
    while (fm) {
        const int uj = __ffsll((unsigned long long) fm) - 1;
        fm &= fm - 1;
        flush(uj, true);
    }
}

// What the three kernels that build the work items share.  pl: the probes of the whole batch [.][nprobe].
struct IvfBuild {
    const uint32_t* pl;
    const uint32_t* blk_ptr;
    uint32_t q0, nq;
    int nprobe, nlist;
    uint32_t* cnt;      // [nlist] pairs per list
    uint32_t* fill;     // [nlist] pairs placed so far
    uint32_t* wi_off;   // [nlist] first work item of the list
    uint32_t* nwi;
    uint32_t* wi_list;
    uint32_t* wi_slot;
    // the padding of a pair that no work item passes
    int n_top, L;
    float* ls;
    uint32_t* li;
    uint32_t* out_items;
    float* out_scores;
};

// the list of pair x = q * nprobe + p, or kPad where there is nothing to pass (no list, or an empty one)
__device__ inline uint32_t pair_list(const IvfBuild& b, size_t x) {
    const uint32_t l = b.pl[(size_t) b.q0 * b.nprobe + x];
    if (l == kPad) return kPad;
    return b.blk_ptr[l + 1] > b.blk_ptr[l] ? l : kPad;
}

__global__ void mfx_ivf_count(IvfBuild b) {
    const size_t total = (size_t) b.nq * b.nprobe;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const uint32_t l = pair_list(b, x);
        if (l != kPad) {
            atomicAdd(b.cnt + l, 1u);
            continue;
        }
        const uint32_t q = (uint32_t) (x / b.nprobe), p = (uint32_t) (x % b.nprobe);
        if (b.nprobe == 1) {
            const size_t o = (size_t) (b.q0 + q) * b.n_top;
            for (int e = 0; e < b.n_top; ++e) {
                b.out_items[o + e] = kPad;
                if (b.out_scores) b.out_scores[o + e] = -INFINITY;
            }
        } else {
            const size_t o = ((size_t) p * b.nq + q) * (size_t) b.L;
            for (int e = 0; e < b.n_top; ++e) { b.ls[o + e] = -INFINITY; b.li[o + e] = kPad; }
        }
    }
}

__global__ __launch_bounds__(256) void mfx_ivf_scan(IvfBuild b) {
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    const int per = (b.nlist + 255) / 256;
    const int l0 = min(b.nlist, tid * per), l1 = min(b.nlist, l0 + per);
    uint32_t s = 0;
    for (int l = l0; l < l1; ++l) s += (b.cnt[l] + kRecUsers - 1) / kRecUsers;
    part[tid] = s;
    __syncthreads();
    uint32_t off = 0;
    for (int x = 0; x < tid; ++x) off += part[x];
    for (int l = l0; l < l1; ++l) {
        b.wi_off[l] = off;
        off += (b.cnt[l] + kRecUsers - 1) / kRecUsers;
    }
    if (tid == 255) *b.nwi = off;
}

__global__ void mfx_ivf_scatter(IvfBuild b) {
    const size_t total = (size_t) b.nq * b.nprobe;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const uint32_t l = pair_list(b, x);
        if (l == kPad) continue;
        const uint32_t q = (uint32_t) (x / b.nprobe), p = (uint32_t) (x % b.nprobe);
        const uint32_t r = atomicAdd(b.fill + l, 1u);  // r < cnt[l]: the same pairs were counted
        const uint32_t wi = b.wi_off[l] + r / kRecUsers;
        b.wi_slot[(size_t) wi * kRecUsers + r % kRecUsers] = q << kPosBits | p;
        if (r % kRecUsers == 0) b.wi_list[wi] = l;
    }
}

// hp2[b][c][tt][jj] = the handle's tile value of item ids[b * 32 + jj]; at the padding positions what mfx_rec_pack_h
// writes past cols (+0, and -0 for t >= k).
__global__ void mfx_ivf_pack_h(const float* hp, const uint32_t* ids, int k, int kc2, int nch, int nblk, float* hp2) {
    const size_t total = (size_t) nblk * nch * kc2 * kTile;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const uint32_t jj = x % kTile;
        size_t rest = x / kTile;
        const int tt = rest % kc2;
        rest /= kc2;
        const int c = rest % nch;
        const size_t b = rest / nch;
        const uint32_t item = ids[b * kTile + jj];
        float v = c * kc2 + tt < k ? 0.f : -0.f;
        if (item != kPad) v = hp[((((size_t) item / kTile) * nch + c) * kc2 + tt) * kTile + item % kTile];
        hp2[x] = v;
    }
}

// fac2[pos] = fac[ids[pos]], NaN at the padding
__global__ void mfx_ivf_fac(const float* fac, const uint32_t* ids, size_t n, float* fac2) {
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (size_t) gridDim.x * blockDim.x) {
        const uint32_t item = ids[x];
        fac2[x] = item == kPad ? __builtin_nanf("") : fac[item];
    }
}

struct EventSet {  // four stream events around the three phases of a launch
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    int create() {
        for (auto& x : e) MFX_HIP(hipEventCreate(&x));
        return MFX_OK;
    }
    ~EventSet() {
        for (auto x : e)
            if (x) (void) hipEventDestroy(x);
    }
};

}  // namespace

int Recommender::ivf_setup(int32_t nlist, const uint32_t* assign, const float* centroids, mfx_memspace space) {
    const char* fn = "mfx_rec_ivf_setup";
    MFX_REQUIRE(nlist >= 1 && nlist <= kMaxList, "%s: nlist must be in [1, %d] (got %d)", fn, kMaxList, nlist);
    MFX_REQUIRE(assign && centroids, "%s: assign and centroids are required", fn);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const size_t cols = (size_t) cols_;

    // the assignment: checked on the device, sorted into lists on the host (once per model; a counting sort keeps the ids
    // of a list ascending)
    DevBuf<uint32_t> d_assign;
    const uint32_t* da = assign;
    if (space == MFX_HOST) {
        MFX_TRY(d_assign.alloc(cols));
        MFX_TRY(d_assign.upload(assign, cols, MFX_HOST, st));
        da = d_assign.get();
    }
    MFX_TRY(check_index_range(da, cols, (uint32_t) nlist, "mfx_rec_ivf_setup: assign entry", st));
    std::vector<uint32_t> h_assign;
    const uint32_t* ha = assign;
    if (space == MFX_DEVICE) {
        h_assign.resize(cols);
        MFX_HIP(hipMemcpyAsync(h_assign.data(), assign, sizeof(uint32_t) * cols, hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        ha = h_assign.data();
    }
    std::vector<uint32_t> list_ptr((size_t) nlist + 1, 0), blk_ptr((size_t) nlist + 1, 0), list_idx(cols);
    for (size_t i = 0; i < cols; ++i) {
        MFX_REQUIRE(ha[i] < (uint32_t) nlist, "%s: assign entry changed during the call", fn);  // (host memory is the caller's)
        ++list_ptr[ha[i] + 1];
    }
    for (int32_t l = 0; l < nlist; ++l) {
        blk_ptr[l + 1] = blk_ptr[l] + (list_ptr[l + 1] + kTile - 1) / kTile;
        list_ptr[l + 1] += list_ptr[l];
    }
    const size_t nblk = blk_ptr[nlist], npos = nblk * kTile;
    std::vector<uint32_t> ids(npos, kPad), at(list_ptr.begin(), list_ptr.end() - 1);
    for (size_t i = 0; i < cols; ++i) {
        const uint32_t l = ha[i], r = at[l]++;
        list_idx[r] = (uint32_t) i;
        ids[(size_t) blk_ptr[l] * kTile + (r - list_ptr[l])] = (uint32_t) i;
    }

    IvfIndex n;
    n.nlist = nlist;
    n.nblk = (int) nblk;
    n.nblkc = (nlist + kTile - 1) / kTile;
    MFX_TRY(n.ids.alloc(npos));            MFX_TRY(n.ids.upload(ids.data(), npos, MFX_HOST, st));
    MFX_TRY(n.blk_ptr.alloc(blk_ptr.size()));   MFX_TRY(n.blk_ptr.upload(blk_ptr.data(), blk_ptr.size(), MFX_HOST, st));
    MFX_TRY(n.list_ptr.alloc(list_ptr.size())); MFX_TRY(n.list_ptr.upload(list_ptr.data(), list_ptr.size(), MFX_HOST, st));
    MFX_TRY(n.list_idx.alloc(cols));       MFX_TRY(n.list_idx.upload(list_idx.data(), cols, MFX_HOST, st));
    MFX_TRY(n.hp.alloc(npos * kt_));
    hipLaunchKernelGGL(mfx_ivf_pack_h, dim3(grid_for(npos * kt_)), dim3(256), 0, st, (const float*) hp_.get(), (const uint32_t*) n.ids.get(),
                       (int) k_, 2 * kc_, nch_, (int) nblk, n.hp.get());
    MFX_LAUNCH_CHECK();
    DevBuf<float> d_cent;
    const float* dc = centroids;
    if (space == MFX_HOST) {
        MFX_TRY(d_cent.alloc((size_t) nlist * k_));
        MFX_TRY(d_cent.upload(centroids, (size_t) nlist * k_, MFX_HOST, st));
        dc = d_cent.get();
    }
    MFX_TRY(n.cp.alloc((size_t) n.nblkc * kTile * kt_));
    MFX_TRY(pack_h_launch(dc, 1, (uint32_t) nlist, n.nblkc, n.cp.get()));
    MFX_HIP(hipStreamSynchronize(st));  // (the host vectors and d_cent go here)
    ivf_ = std::move(n);
    return ivf_refresh_fac();
}

int Recommender::ivf_refresh_fac() {
    if (!ivf_.nlist) return MFX_OK;
    if (!fac_keep_.get()) {
        ivf_.fac.release();
        return MFX_OK;
    }
    const size_t npos = (size_t) ivf_.nblk * kTile;
    if (!ivf_.fac.get()) MFX_TRY(ivf_.fac.alloc(npos));
    hipLaunchKernelGGL(mfx_ivf_fac, dim3(grid_for(npos)), dim3(256), 0, st_, (const float*) fac_keep_.get(), (const uint32_t*) ivf_.ids.get(),
                       npos, ivf_.fac.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Recommender::ivf_lists(uint32_t* list_ptr, uint32_t* list_idx, mfx_memspace space) {
    const char* fn = "mfx_rec_ivf_lists";
    MFX_REQUIRE(ivf_.nlist, "%s: call mfx_rec_ivf_setup first", fn);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    MFX_REQUIRE(list_ptr && list_idx, "%s: list_ptr and list_idx are required", fn);
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    MFX_HIP(hipMemcpyAsync(list_ptr, ivf_.list_ptr.get(), sizeof(uint32_t) * ((size_t) ivf_.nlist + 1), kind, st_));
    MFX_HIP(hipMemcpyAsync(list_idx, ivf_.list_idx.get(), sizeof(uint32_t) * (size_t) cols_, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

// The probe of nu staged slots: the top-N pass with the packed centroids as the items, no exclusion and no filter.  The
// slices are chosen here for the centroids' tiles (about two workgroups per CU, no fewer than four tiles a slice).
int Recommender::ivf_probe_dev(uint32_t nu, const uint32_t* du, int32_t nprobe, uint32_t* lists, float* scores, mfx_memspace space) {
    const TileSet ts{ivf_.cp.get(), (uint32_t) ivf_.nlist, ivf_.nblkc};
    const int64_t blocks = ((int64_t) nu + kRecUsers - 1) / kRecUsers, want = 2 * cus_;
    int slices = blocks >= want ? 1 : (int) ((want + blocks - 1) / blocks);
    slices = std::max(1, std::min({slices, std::max(1, ivf_.nblkc / 4), kMaxMerge / nprobe}));
    return topn(wp_.get(), nu, du, nullptr, nullptr, nprobe, lists, scores, space, slices, nullptr, nullptr, &ts);
}

namespace {
// the ranges mfx_rec_ivf_probe and mfx_rec_query_ivf share
int check_ivf_batch(const char* fn, const IvfIndex& ivf, int64_t nusers, const uint32_t* users, int64_t rows, int32_t nprobe, mfx_memspace space) {
    MFX_REQUIRE(ivf.nlist, "%s: call mfx_rec_ivf_setup first", fn);
    MFX_REQUIRE(nprobe >= 1 && nprobe <= ivf.nlist, "%s: nprobe must be in [1, nlist = %d] (got %d)", fn, ivf.nlist, nprobe);
    MFX_REQUIRE(nprobe <= kMaxTop, "%s: nprobe must be <= %d (got %d)", fn, kMaxTop, nprobe);
    MFX_REQUIRE(nusers >= 0 && nusers < (int64_t) 0xFFFFFFFFll, "%s: bad nusers %lld", fn, (long long) nusers);
    MFX_REQUIRE(users || nusers <= rows, "%s: users = NULL needs nusers <= rows (%lld > %lld)", fn, (long long) nusers, (long long) rows);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    return MFX_OK;
}
}  // namespace

int Recommender::ivf_probe(int64_t nusers, const uint32_t* users, int32_t nprobe, uint32_t* lists, float* scores, mfx_memspace space) {
    const char* fn = "mfx_rec_ivf_probe";
    MFX_TRY(check_ivf_batch(fn, ivf_, nusers, users, rows_, nprobe, space));
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(lists, "%s: lists is NULL", fn);
    MFX_TRY(use_device(device_));
    DevBuf<uint32_t> d_users;
    const uint32_t* du = nullptr;
    MFX_TRY(stage_ids(users, (uint32_t) nusers, space, (uint32_t) rows_, "mfx_rec_ivf_probe: user id", d_users, &du));
    return ivf_probe_dev((uint32_t) nusers, du, nprobe, lists, scores, space);
}

int Recommender::query_ivf(int64_t nusers, const uint32_t* users, int32_t nprobe, int32_t n_top, uint32_t* items, float* scores,
                           mfx_memspace space) {
    const char* fn = "mfx_rec_query_ivf";
    MFX_TRY(check_ivf_batch(fn, ivf_, nusers, users, rows_, nprobe, space));
    MFX_REQUIRE(n_top >= 1 && n_top <= kMaxTop, "%s: n_top must be in [1, %d] (got %d)", fn, kMaxTop, n_top);
    MFX_REQUIRE((int64_t) nprobe * n_top <= kMaxMerge, "%s: nprobe * n_top must be <= %d (got %d * %d)", fn, kMaxMerge, nprobe, n_top);
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(items, "%s: items is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    const uint32_t nu = (uint32_t) nusers;
    for (double& s : ivf_s_) s = 0.0;
    DevBuf<uint32_t> d_users;
    const uint32_t* du = nullptr;
    MFX_TRY(stage_ids(users, nu, space, (uint32_t) rows_, "mfx_rec_query_ivf: user id", d_users, &du));

    EventSet pe;
    MFX_TRY(pe.create());
    DevBuf<uint32_t> pl;
    MFX_TRY(pl.alloc((size_t) nu * nprobe));
    MFX_HIP(hipEventRecord(pe.e[0], st));
    MFX_TRY(ivf_probe_dev(nu, du, nprobe, pl.get(), nullptr, MFX_DEVICE));
    MFX_HIP(hipEventRecord(pe.e[1], st));

    int L = 64;
    while (L < n_top + 32) L <<= 1;
    size_t qmax = kWorkspaceCap / ((size_t) nprobe * L * 8);  // <= 2^21 slots: a pair fits 32 bits
    qmax = std::max<size_t>(kRecUsers, qmax / kRecUsers * kRecUsers);
    const uint32_t qc = (uint32_t) std::min<size_t>(nu, qmax);
    const size_t pairs_max = (size_t) qc * nprobe;
    const size_t nwi_max = pairs_max / kRecUsers + std::min<size_t>((size_t) ivf_.nlist, pairs_max);

    DevBuf<uint32_t> d_items, li, counters, wi_list, wi_slot;
    DevBuf<float> d_scores, ls;
    uint32_t* oi = items;
    float* os = scores;
    if (space == MFX_HOST) {
        MFX_TRY(d_items.alloc((size_t) nu * n_top));
        oi = d_items.get();
        if (scores) {
            MFX_TRY(d_scores.alloc((size_t) nu * n_top));
            os = d_scores.get();
        }
    }
    MFX_TRY(ls.alloc((size_t) nprobe * qc * L));
    MFX_TRY(li.alloc((size_t) nprobe * qc * L));
    const size_t nl = (size_t) ivf_.nlist;
    MFX_TRY(counters.alloc(3 * nl + 1));  // cnt, fill, wi_off, nwi
    MFX_TRY(wi_list.alloc(nwi_max));
    MFX_TRY(wi_slot.alloc(nwi_max * kRecUsers));

    IvfBuild b{};
    b.pl = pl.get(); b.blk_ptr = ivf_.blk_ptr.get();
    b.nprobe = nprobe; b.nlist = ivf_.nlist;
    b.cnt = counters.get(); b.fill = b.cnt + nl; b.wi_off = b.fill + nl; b.nwi = b.wi_off + nl;
    b.wi_list = wi_list.get(); b.wi_slot = wi_slot.get();
    b.n_top = n_top; b.L = L; b.ls = ls.get(); b.li = li.get(); b.out_items = oi; b.out_scores = os;

    IvfArgs a{};
    a.wp = wp_.get(); a.hp = ivf_.hp.get(); a.fac = ivf_.fac.get();
    a.kt = kt_; a.nch = nch_;
    a.users = du;
    a.ex_ptr = has_ex_ ? ex_ptr_.get() : nullptr; a.ex_idx = ex_idx_.get();
    a.n_top = n_top; a.L = L; a.nprobe = nprobe;
    a.ls = ls.get(); a.li = li.get(); a.out_items = oi; a.out_scores = os;
    a.ids = ivf_.ids.get(); a.blk_ptr = ivf_.blk_ptr.get(); a.list_ptr = ivf_.list_ptr.get();
    a.wi_list = wi_list.get(); a.wi_slot = wi_slot.get(); a.nwi = b.nwi;

    std::vector<std::unique_ptr<EventSet>> evs;
    for (uint32_t q0 = 0; q0 < nu; q0 += qc) {
        const uint32_t nq = std::min(qc, nu - q0);
        const size_t pairs = (size_t) nq * nprobe;
        const size_t nwi_cap = pairs / kRecUsers + std::min<size_t>(nl, pairs);
        b.q0 = a.q0 = q0;
        b.nq = a.nq = nq;
        evs.emplace_back(new EventSet());
        EventSet& ev = *evs.back();
        MFX_TRY(ev.create());
        MFX_HIP(hipEventRecord(ev.e[0], st));
        MFX_HIP(hipMemsetAsync(counters.get(), 0, sizeof(uint32_t) * (3 * nl + 1), st));
        MFX_HIP(hipMemsetAsync(wi_slot.get(), 0xFF, sizeof(uint32_t) * nwi_cap * kRecUsers, st));
        hipLaunchKernelGGL(mfx_ivf_count, dim3(grid_for(pairs)), dim3(256), 0, st, b);
        MFX_LAUNCH_CHECK();
        hipLaunchKernelGGL(mfx_ivf_scan, dim3(1), dim3(256), 0, st, b);
        MFX_LAUNCH_CHECK();
        hipLaunchKernelGGL(mfx_ivf_scatter, dim3(grid_for(pairs)), dim3(256), 0, st, b);
        MFX_LAUNCH_CHECK();
        MFX_HIP(hipEventRecord(ev.e[1], st));
        MFX_TRY(dispatch_kc(kc_, [&](auto kc) {
            constexpr int KC = decltype(kc)::value;
            const dim3 grid((uint32_t) nwi_cap);
            if (a.fac) hipLaunchKernelGGL((mfx_ivf_topn<KC, true>), grid, dim3(kRecThreads), 0, st, a);
            else hipLaunchKernelGGL((mfx_ivf_topn<KC, false>), grid, dim3(kRecThreads), 0, st, a);
            MFX_LAUNCH_CHECK();
            return (int) MFX_OK;
        }));
        MFX_HIP(hipEventRecord(ev.e[2], st));
        if (nprobe > 1) MFX_TRY(merge_launch(ls.get(), li.get(), q0, nq, nprobe, L, n_top, oi, os));
        MFX_HIP(hipEventRecord(ev.e[3], st));
    }
    if (space == MFX_HOST) {
        MFX_HIP(hipMemcpyAsync(items, oi, sizeof(uint32_t) * nu * n_top, hipMemcpyDeviceToHost, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, os, sizeof(float) * nu * n_top, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    MFX_HIP(hipEventElapsedTime(&ms, pe.e[0], pe.e[1]));
    ivf_s_[0] = 1e-3 * ms;
    for (const auto& ev : evs)
        for (int i = 0; i < 3; ++i) {
            MFX_HIP(hipEventElapsedTime(&ms, ev->e[i], ev->e[i + 1]));
            ivf_s_[i + 1] += 1e-3 * ms;
        }
    return MFX_OK;
}

}  // namespace mfx
