// recommend.hip -- fused top-N recommendation on gfx950 (mfx_rec_*), plus the host-side ranking metrics.
//
// A query never materialises the users x items score matrix.  One workgroup (four waves) owns 128 users of the batch
// and one slice of the items.  H is repacked at create time into 32-item tiles, [tile][t chunk][2*KC t values][32
// items], so that one LDS stage is a contiguous copy that every wave of the workgroup shares (double-buffered, one
// barrier per stage).  Each wave keeps the W rows of its 32 users in registers as the B operand of
// v_mfma_f32_32x32x2_f32 (lane l: W[user l&31][t = 2s + (l>>5)]) and reads the H tile as the A operand
// (H[item l&31][t = 2s + (l>>5)]), so the accumulator has the user on the lane (column = lane & 31) and 16 items in
// the registers (row = (r&3) + 8*(r>>2) + 4*(lane>>5)).  Every score is the fp32 FMA chain over t = 0, 1, 2, ... in
// ascending order (one MFMA = two chained FMAs), whatever the tile, slice, batch or factor layout; k is padded to
// the MFMA step with steps that leave the accumulator bitwise unchanged (W +0, H -0; see mfx_rec_pack_h), and k > 128
// runs several t chunks into the same accumulator, same order.  That pass is rec_tile_pass of rec_tiles.hpp, which the
// rank count of rec_rank.hip runs too; mfx_rec_topn adds the selection as its per-tile callback.
//
// Selection: each lane holds the running threshold of its user (the N-th best score so far) and compares its 16
// scores against it -- one VALU compare per score.  Scores that pass are appended to the user's candidate list
// (L = pow2 >= N + 32 entries in the workspace).  When a list would overflow, the wave filters the new entries
// against the user's exclusion row (binary search, candidates only), sorts the list (bitonic, in LDS for L <= 256,
// in place in the workspace otherwise), keeps the best N and raises the threshold.  Items of one slice are visited
// in ascending order, so admitting ties (score >= threshold) is only ever extra work, never a wrong answer.
// Total order: score descending, then item ascending; -0 == +0; NaN scores are never admitted.
//
// Small batches split the items over `slices` (grid.y); each slice leaves its sorted top N in the workspace and
// mfx_rec_merge selects the final N from slices * N entries.  The scores are the same numbers, so the result is
// bitwise the one of the unsplit pass.
//
// Fold-in (mfx_rec_fold_in) solves the query rows with the ALS half-sweep launchers against H unpacked from the tiles
// (the same bits the scores use), packs the solved rows like W and runs the same top-N pass with the query's own rows
// as the exclusion.  Above rank 128 (mfx_rec_fold_in_block_setup) the rows are solved by the block subspace sweeps of
// ials_block.hip instead, repeated up to a sweep count with a stop per row (ialsb_fold_launch); the explicit objectives of
// MFX_FOLD_ALS / MFX_FOLD_CCD the same way after mfx_rec_fold_in_block_setup_als (alsb_fold_launch).  After
// mfx_rec_fold_in_cg_setup the rows are solved by conjugate gradients preconditioned by the inverse of the base Gramian
// (rec_foldin_cg.hip, foldcg_launch), at any rank up to 1024: a solve with a residual bound, not a sweep.
// Explanations (mfx_rec_explain) take Z = A^-1 h_target from the factor of a closed-form solve (k <= 128); after the cg
// setup mfx_rec_explain_cg takes it from the same conjugate gradients over the pairs (rec_explain_cg.hip, explaincg_launch).
//
// Item-to-item similarity (mfx_rec_similar) and the item filter (mfx_rec_set_item_filter) are one per-item fp32 factor on
// the accumulator before the compare (mfx_rec_topn<KC, true>): an inverse norm for the cosine, 1 / NaN for kept / dropped
// items.  The query operand is H itself packed like W, self-exclusion an identity exclusion CSR, and the cosine's second
// factor c[q] is applied once per output slot where the final N are written (flush or mfx_rec_merge), so the order is
// the keys'.
//
// IVF retrieval (mfx_rec_query_ivf, rec_ivf.hip) runs the same top-N pass over the centroids of its item lists as the probe
// (topn with another tile set) and sends its per-probe partial lists through mfx_rec_merge (merge_launch).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <unordered_map>

#include "als_solver.hpp"   // AlsHalf and the half-sweep launchers (fold-in)
#include "ccd_kernels.hpp"  // check_index_range
#include "rec_tiles.hpp"   // the tile pass, the workgroup shape, the total order
#include "recommend.hpp"
#include "rec_foldin_cg.hpp"

namespace mfx {

namespace {

constexpr int kScr = 256;                    // per-wave LDS sort scratch (entries); longer lists sort in the workspace
constexpr int kMaxMerge = 8192;              // slices * N of one merge (64 KiB of LDS)
constexpr int kMaxTop = 1024, kMaxK = 1024;
constexpr size_t kWorkspaceCap = size_t(1) << 30;  // candidate lists of one launch (users are chunked under this)

struct RecArgs : TileArgs {
    const uint32_t* users;  // NULL: slot q is user q0 + q
    uint32_t q0, nq;        // first batch slot of this launch, slots in this launch
    const uint32_t* ex_ptr; // NULL: no exclusion
    const uint32_t* ex_idx;
    int n_top, L;
    float* ls;              // [slices][nq][L] candidate lists
    uint32_t* li;
    uint32_t* out_items;    // [q0 + q][n_top], written here when there is one slice
    float* out_scores;      // may be NULL
    const float* qfac;      // NULL, or [query id]: factor of a slot's returned scores, applied where its final N leave
};

// Every lane of the wave sees the memory operations every other lane issued before (LDS and global).
__device__ inline void wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// Bitonic sort of P (power of two) entries, best first, by one wave.  ks / is are flat pointers (LDS or global).
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

// FAC: the ranking key of (slot, item) is fp32(score * a.fac[item]) instead of the score (cosine keys, item filter).
// KC <= 16 fits four waves per SIMD (109 to 125 VGPRs), but only when the allocator is asked for four: left to itself it
// adds 16 AGPRs, which costs KC = 16 (and KC = 8 with the factors) the fourth wave.  KC = 32 / 64 get the default (3 / 2).
// KC = 16 is three registers from the 128 at which the request turns into spills: whoever adds per-lane state to the
// callback or to flush checks -Rpass-analysis=kernel-resource-usage for scratch (DESIGN 5.4 has the table).
//
// The kernel is the slot's list state, flush, and the tile pass of rec_tiles.hpp with the admission as its callback.
template <int KC, bool FAC>
__global__ __launch_bounds__(kRecThreads) __attribute__((amdgpu_waves_per_eu(KC <= 16 ? 4 : 1)))
void mfx_rec_topn(RecArgs a) {
    __shared__ float scs[kRecWaves][kScr];
    __shared__ uint32_t sci[kRecWaves][kScr];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, j = lane & 31;
    const uint32_t slice = blockIdx.y;
    const uint32_t qw0 = blockIdx.x * kRecUsers + wave * 32;
    const uint32_t q = qw0 + j;
    const bool uvalid = q < a.nq;
    const uint32_t u = uvalid ? (a.users ? a.users[a.q0 + q] : a.q0 + q) : 0;
    const bool single = gridDim.y == 1;
    const bool lds_sort = a.L <= kScr;

    float thr = -INFINITY;  // score of the user's N-th entry once it has N; admission is score >= thr
    int cnt = 0;            // entries in the user's list
    int clean = 0;          // leading entries already checked against the exclusion row (the sorted top)

    // Filters, sorts and truncates the list of user slot qw0 + uj (the whole wave works on it).  fin: write the
    // final N entries (padded) to the output (one slice) or to the head of the list (merge input).
    auto flush = [&](int uj, bool fin) __attribute__((always_inline)) {
        const int c_u = __shfl(cnt, uj), cl_u = __shfl(clean, uj);
        const uint32_t uid = __shfl(u, uj);
        const uint32_t qu = qw0 + uj;
        const size_t base = ((size_t) slice * a.nq + qu) * (size_t) a.L;
        int P = 1;
        while (P < c_u) P <<= 1;
        float* ks = lds_sort ? scs[wave] : a.ls + base;
        uint32_t* is = lds_sort ? sci[wave] : a.li + base;
        uint32_t elo = 0, ehi = 0;
        if (a.ex_ptr) { elo = a.ex_ptr[uid]; ehi = a.ex_ptr[uid + 1]; }
        wave_sync();
        int kept = 0;
        for (int e = lane; e < P; e += 64) {
            float s = -INFINITY;
            uint32_t it = kPad;
            if (e < c_u) {
                s = a.ls[base + e];
                it = a.li[base + e];
                if (e >= cl_u && ehi > elo && excluded(a.ex_idx, elo, ehi, it)) { s = -INFINITY; it = kPad; }
                else ++kept;
            }
            ks[e] = s;
            is[e] = it;
        }
        kept = wave_sum(kept);
        wave_sync();
        wave_bitonic(ks, is, P, lane);
        const int m = min(a.n_top, kept);
        if (fin) {
            for (int e = lane; e < a.n_top; e += 64) {
                float s = -INFINITY;
                uint32_t it = kPad;
                if (e < m) { s = ks[e]; it = is[e]; }
                if (single) {
                    const size_t o = (size_t) (a.q0 + qu) * a.n_top + e;
                    if (FAC && a.qfac && e < m) s *= a.qfac[uid];
                    a.out_items[o] = it;
                    if (a.out_scores) a.out_scores[o] = s;
                } else {
                    a.ls[base + e] = s;
                    a.li[base + e] = it;
                }
            }
        } else if (lds_sort) {
            for (int e = lane; e < m; e += 64) { a.ls[base + e] = ks[e]; a.li[base + e] = is[e]; }
        }
        wave_sync();
        const float nthr = (!fin && m == a.n_top) ? ks[a.n_top - 1] : -INFINITY;
        if (j == uj) { cnt = m; clean = m; thr = nthr; }
        wave_sync();
    };

    rec_tile_pass<KC, FAC>(a, (int) slice, u, uvalid, [&](uint32_t ibase, const f32x16& acc) __attribute__((always_inline)) {
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) mask |= (uint32_t) (uvalid && acc_item(ibase, r) < a.cols && acc[r] >= thr) << r;
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
                size_t pos = ((size_t) slice * a.nq + q) * (size_t) a.L + cnt + (h ? n_o : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (mask >> r & 1) {
                        a.ls[pos] = acc[r];
                        a.li[pos] = acc_item(ibase, r);
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

// Final N of one batch slot from the slices' sorted heads (one wave per slot).
// qfac (NULL: none) scales the scores on the way out, indexed by the slot's query id; the order is the keys'.
__global__ __launch_bounds__(64) void mfx_rec_merge(const float* ls, const uint32_t* li, uint32_t q0, uint32_t nq,
                                                    int slices, int L, int n_top, int P, uint32_t* out_items,
                                                    float* out_scores, const uint32_t* users, const float* qfac) {
    extern __shared__ float smem[];
    float* ks = smem;
    uint32_t* is = reinterpret_cast<uint32_t*>(smem + P);
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const int n_in = slices * n_top;
    for (int e = lane; e < P; e += 64) {
        float s = -INFINITY;
        uint32_t it = kPad;
        if (e < n_in) {
            const size_t src = ((size_t) (e / n_top) * nq + q) * (size_t) L + (e % n_top);
            s = ls[src];
            it = li[src];
        }
        ks[e] = s;
        is[e] = it;
    }
    wave_sync();
    wave_bitonic(ks, is, P, lane);
    const float qf = qfac ? qfac[users ? users[q0 + q] : q0 + q] : 1.f;
    for (int e = lane; e < n_top; e += 64) {
        const size_t o = (size_t) (q0 + q) * n_top + e;
        out_items[o] = is[e];
        if (out_scores) out_scores[o] = (qfac && is[e] != kPad) ? ks[e] * qf : ks[e];
    }
}

// hp[b][c][tt][jj] = H[item b*32 + jj][t c*2KC + tt], zero outside cols x k.  The padding t >= k is -0: with the
// +0 padding of W its products are -0, and fma(+0, -0, acc) == acc for every acc, a -0 score included (a +0 product
// would turn an underflowed -0 score into +0).
__global__ void mfx_rec_pack_h(const float* H, int layout, uint32_t cols, int k, int kc2, int nch, int nblk, float* hp) {
    const size_t total = (size_t) nblk * nch * kc2 * kTile;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const uint32_t jj = x % kTile;
        size_t rest = x / kTile;
        const int tt = rest % kc2;
        rest /= kc2;
        const int c = rest % nch;
        const size_t b = rest / nch;
        const size_t item = b * kTile + jj;
        const int t = c * kc2 + tt;
        float v = t < k ? 0.f : -0.f;
        if (item < cols && t < k) v = layout == 0 ? H[(size_t) t * cols + item] : H[item * k + t];
        hp[x] = v;
    }
}

// wp[u][t] = W[u][t], zero for t >= k.
__global__ void mfx_rec_pack_w(const float* W, int layout, uint32_t rows, int k, int kt, float* wp) {
    const size_t total = (size_t) rows * kt;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const size_t uu = x / kt;
        const int t = x % kt;
        float v = 0.f;
        if (t < k) v = layout == 0 ? W[(size_t) t * rows + uu] : W[uu * k + t];
        wp[x] = v;
    }
}

// hx[item][t] = H[item][t] read back from the tiles of mfx_rec_pack_h (t < k only: the padding never leaks in), row
// `cols` all zeros: the gather target of the half-sweep kernels past a segment's end.
__global__ void mfx_rec_unpack_h(const float* hp, uint32_t cols, int k, int kc2, int nch, float* hx) {
    const size_t total = ((size_t) cols + 1) * k;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const size_t item = x / k;
        const int t = x % k;
        float v = 0.f;
        if (item < cols) v = hp[(((item / kTile) * nch + t / kc2) * kc2 + t % kc2) * kTile + item % kTile];
        hx[x] = v;
    }
}

// hq[item][t] = H[item][t] from the tiles, +0 for t >= k: the rows of H as a query operand, laid out as mfx_rec_pack_w lays W.
__global__ void mfx_rec_pack_hq(const float* hp, uint32_t cols, int k, int kc2, int nch, int kt, float* hq) {
    const size_t total = (size_t) cols * kt;
    for (size_t x = (size_t) blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t) gridDim.x * blockDim.x) {
        const size_t item = x / kt;
        const int t = x % kt;
        float v = 0.f;
        if (t < k) v = hp[(((item / kTile) * nch + t / kc2) * kc2 + t % kc2) * kTile + item % kTile];
        hq[x] = v;
    }
}

// n2[i] = the score chain of (H[i], H[i]); c[i] = fp32(1 / sqrt(n2[i])) through fp64, +0 where n2 is 0 or not finite.
// id[i] = i for i <= cols: row pointers and column indices of the identity exclusion (an item is not its own neighbour).
__global__ void mfx_rec_item_norms(const float* hq, uint32_t cols, int k, int kt, float* n2, float* c, uint32_t* id) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i <= cols; i += (size_t) gridDim.x * blockDim.x) {
        id[i] = (uint32_t) i;
        if (i == cols) continue;
        const float* h = hq + i * kt;
        float acc = 0.f;
        for (int t = 0; t < k; ++t) acc = __builtin_fmaf(h[t], h[t], acc);
        n2[i] = acc;
        c[i] = (acc > 0.f && acc < INFINITY) ? (float) (1.0 / sqrt((double) acc)) : 0.f;
    }
}

// fac[i] = (c ? c[i] : 1) for the items that may be returned, NaN for the others and for the padding past cols.
__global__ void mfx_rec_build_fac(const uint8_t* keep, const float* c, uint32_t cols, size_t npad, float* fac) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < npad; i += (size_t) gridDim.x * blockDim.x) {
        float v = __builtin_nanf("");
        if (i < cols && (!keep || keep[i])) v = c ? c[i] : 1.f;
        fac[i] = v;
    }
}

// bad |= 1: row pointers not a valid prefix sum of nnz; 2: column index >= cols; 4: a row not non-decreasing.
__global__ void mfx_rec_check_exclude(const uint32_t* rp, const uint32_t* ci, uint32_t rows, uint32_t cols,
                                      uint64_t nnz, int* bad) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const uint32_t lo = rp[r], hi = rp[r + 1];
        if (lo > hi || hi > nnz || (r == 0 && lo != 0) || (r == rows - 1 && hi != nnz)) {
            atomicOr(bad, 1);
            continue;
        }
        uint32_t prev = 0;
        int f = 0;
        for (uint32_t p = lo; p < hi; ++p) {
            const uint32_t c = ci[p];
            if (c >= cols) f |= 2;
            if (p > lo && c < prev) f |= 4;
            prev = c;
        }
        if (f) atomicOr(bad, f);
    }
}

// mfx_rec_check_exclude over a CSR on the device and its three refusals.  `who` opens every message ("mfx_rec_create:
// exclusion "), `ptr` is what the caller calls the row pointers.
int check_csr(const uint32_t* rp, const uint32_t* ci, uint32_t rows, uint32_t cols, uint64_t nnz, const char* who, const char* ptr,
              hipStream_t st) {
    DevBuf<int> bad;
    MFX_TRY(bad.alloc_zero(1, st));
    hipLaunchKernelGGL(mfx_rec_check_exclude, dim3(grid_for((size_t) rows)), dim3(256), 0, st, rp, ci, rows, cols, nnz, bad.get());
    MFX_LAUNCH_CHECK();
    int hb = 0;
    MFX_HIP(hipMemcpyAsync(&hb, bad.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    MFX_REQUIRE(!(hb & 1), "%s%s is not a non-decreasing prefix sum from 0 to nnz", who, ptr);
    MFX_REQUIRE(!(hb & 2), "%scolumn index out of range [0, %lld)", who, (long long) cols);
    MFX_REQUIRE(!(hb & 4), "%scolumn indices must be non-decreasing within every row", who);
    return MFX_OK;
}

// What mfx_rec_query and mfx_rec_similar check alike: fn is the entry point, ids / n / bound its names for the batch's
// ids, their number and what bounds a batch without ids.
int check_batch(const char* fn, const char* ids_name, const char* n_name, const char* bound_name, int64_t n, const uint32_t* ids,
                int64_t bound, int32_t n_top, mfx_memspace space, int item_slices) {
    MFX_REQUIRE(n_top >= 1 && n_top <= kMaxTop, "%s: n_top must be in [1, %d] (got %d)", fn, kMaxTop, n_top);
    MFX_REQUIRE(n >= 0 && n < (int64_t) 0xFFFFFFFFll, "%s: bad %s %lld", fn, n_name, (long long) n);
    MFX_REQUIRE(ids || n <= bound, "%s: %s = NULL needs %s <= %s (%lld > %lld)", fn, ids_name, n_name, bound_name, (long long) n,
                (long long) bound);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    MFX_REQUIRE(item_slices >= 0, "%s: item_slices must be >= 0 (got %d)", fn, item_slices);
    MFX_REQUIRE(item_slices * (int64_t) n_top <= kMaxMerge, "%s: item_slices * n_top must be <= %d", fn, kMaxMerge);
    return MFX_OK;
}

// What the block setups of fold-in check last (fold_setup): block / sweeps / tol.  fn is the entry point's name.
int check_fold_sweeps(const char* fn, int32_t block, int32_t sweeps, float tol) {
    MFX_REQUIRE(block >= 0 && block <= (int32_t) kIalsBlockMaxBlock, "%s: block = %d (0 = chosen from k, else 1 <= block <= %u)", fn,
                block, kIalsBlockMaxBlock);
    MFX_REQUIRE(sweeps >= 1 && sweeps <= 1024, "%s: sweeps = %d (1 <= sweeps <= 1024)", fn, sweeps);
    MFX_REQUIRE(std::isfinite(tol) && tol >= 0.f, "%s: tol = %g (finite and >= 0 required)", fn, (double) tol);
    return MFX_OK;
}

}  // namespace

Recommender::~Recommender() {
    if (st_) {
        (void) hipSetDevice(device_);
        (void) hipStreamSynchronize(st_);
        (void) hipStreamDestroy(st_);
    }
}

int Recommender::create(Recommender** out, const float* W, const float* H, int64_t rows, int64_t cols, int64_t k,
                        int layout, const mfx_csx* ex, mfx_memspace space, int device) {
    *out = nullptr;
    MFX_REQUIRE(W && H, "mfx_rec_create: W and H are required");
    MFX_REQUIRE(rows >= 1 && cols >= 1 && rows < (int64_t) 0xFFFFFFFFll && cols < (int64_t) 0xFFFFFFFFll,
                "mfx_rec_create: rows / cols out of range (%lld x %lld)", (long long) rows, (long long) cols);
    MFX_REQUIRE(k >= 1 && k <= kMaxK, "mfx_rec_create: k must be in [1, %d] (got %lld)", kMaxK, (long long) k);
    MFX_REQUIRE(layout == 0 || layout == 1, "mfx_rec_create: layout must be 0 (CCD++) or 1 (ALS), got %d", layout);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_create: bad memory space");
    if (ex) {
        MFX_REQUIRE(ex->rows == rows && ex->cols == cols,
                    "mfx_rec_create: exclusion matrix is %lld x %lld, the factors are %lld x %lld", (long long) ex->rows,
                    (long long) ex->cols, (long long) rows, (long long) cols);
        MFX_REQUIRE(ex->csr_row_ptr && ex->nnz >= 0 && ex->nnz < (int64_t) 0xFFFFFFFFll && (ex->nnz == 0 || ex->csr_col_idx),
                    "mfx_rec_create: exclusion matrix lacks csr_row_ptr / csr_col_idx");
    }
    MFX_TRY(use_device(device));
    std::unique_ptr<Recommender> r(new Recommender());
    r->device_ = device;
    r->rows_ = rows; r->cols_ = cols; r->k_ = k;
    const int steps = (int) ((k + 1) / 2);
    int kc = 1;
    while (kc < steps && kc < 64) kc <<= 1;
    r->kc_ = kc;
    r->nch_ = (steps + kc - 1) / kc;
    r->kt_ = r->nch_ * 2 * kc;
    r->nblk_ = (int) ((cols + kTile - 1) / kTile);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) r->cus_ = cus;
    MFX_HIP(hipStreamCreateWithFlags(&r->st_, hipStreamNonBlocking));
    hipStream_t st = r->st_;

    DevBuf<float> tw, th;
    const float* dW = W;
    const float* dH = H;
    if (space == MFX_HOST) {
        MFX_TRY(tw.alloc((size_t) rows * k)); MFX_TRY(tw.upload(W, (size_t) rows * k, MFX_HOST, st));
        MFX_TRY(th.alloc((size_t) cols * k)); MFX_TRY(th.upload(H, (size_t) cols * k, MFX_HOST, st));
        dW = tw.get();
        dH = th.get();
    }
    MFX_TRY(r->wp_.alloc((size_t) rows * r->kt_));
    MFX_TRY(r->hp_.alloc((size_t) r->nblk_ * kTile * r->kt_));
    hipLaunchKernelGGL(mfx_rec_pack_w, dim3(grid_for((size_t) rows * r->kt_)), dim3(256), 0, st, dW, layout,
                       (uint32_t) rows, (int) k, r->kt_, r->wp_.get());
    MFX_LAUNCH_CHECK();
    hipLaunchKernelGGL(mfx_rec_pack_h, dim3(grid_for((size_t) r->nblk_ * kTile * r->kt_)), dim3(256), 0, st, dH, layout,
                       (uint32_t) cols, (int) k, 2 * kc, r->nch_, r->nblk_, r->hp_.get());
    MFX_LAUNCH_CHECK();

    if (ex) {
        uint32_t nnz_ptr = 0;
        MFX_TRY(r->ex_ptr_.alloc((size_t) rows + 1));
        MFX_TRY(r->ex_ptr_.upload(ex->csr_row_ptr, (size_t) rows + 1, space, st));
        MFX_HIP(hipMemcpyAsync(&nnz_ptr, r->ex_ptr_.get() + rows, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        MFX_REQUIRE((int64_t) nnz_ptr == ex->nnz, "mfx_rec_create: exclusion csr_row_ptr[rows] = %u but nnz = %lld", nnz_ptr,
                    (long long) ex->nnz);
        if (ex->nnz > 0) {
            MFX_TRY(r->ex_idx_.alloc((size_t) ex->nnz));
            MFX_TRY(r->ex_idx_.upload(ex->csr_col_idx, (size_t) ex->nnz, space, st));
        }
        MFX_TRY(check_csr(r->ex_ptr_.get(), r->ex_idx_.get(), (uint32_t) rows, (uint32_t) cols, (uint64_t) ex->nnz,
                          "mfx_rec_create: exclusion ", "csr_row_ptr", st));
        r->has_ex_ = true;
    }
    MFX_HIP(hipStreamSynchronize(st));
    *out = r.release();
    return MFX_OK;
}

int Recommender::query(int64_t nusers, const uint32_t* users, int32_t n_top, uint32_t* items, float* scores,
                       mfx_memspace space, int item_slices) {
    MFX_TRY(check_batch("mfx_rec_query", "users", "nusers", "rows", nusers, users, rows_, n_top, space, item_slices));
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(items, "mfx_rec_query: items is NULL");
    MFX_TRY(use_device(device_));
    const uint32_t nu = (uint32_t) nusers;
    DevBuf<uint32_t> d_users;
    const uint32_t* du = nullptr;
    MFX_TRY(stage_ids(users, nu, space, (uint32_t) rows_, "mfx_rec_query: user id", d_users, &du));
    return topn(wp_.get(), nu, du, has_ex_ ? ex_ptr_.get() : nullptr, ex_idx_.get(), n_top, items, scores, space, item_slices,
                fac_keep_.get(), nullptr);
}

int Recommender::stage_ids(const uint32_t* ids, uint32_t n, mfx_memspace space, uint32_t bound, const char* what, DevBuf<uint32_t>& buf,
                           const uint32_t** dev) {
    *dev = ids;
    if (!ids) return MFX_OK;
    if (space == MFX_HOST) {
        MFX_TRY(buf.alloc(n));
        MFX_TRY(buf.upload(ids, n, MFX_HOST, st_));
        *dev = buf.get();
    }
    return check_index_range(*dev, n, bound, what, st_);
}

int Recommender::pick_slices(int forced, int64_t blocks, int cap) const {
    int slices = forced;
    if (slices == 0) {  // enough workgroups for about two per CU
        const int64_t want = 2 * cus_;
        slices = blocks >= want ? 1 : (int) ((want + blocks - 1) / blocks);
        slices = std::max(1, std::min(slices, std::max(1, nblk_ / 4)));
    }
    slices = std::min(slices, cap);
    const int bps = (nblk_ + slices - 1) / slices;
    return (nblk_ + bps - 1) / bps;  // no empty slices
}

int Recommender::build_facs(const uint8_t* keep) {
    const size_t npad = (size_t) nblk_ * kTile;
    if (keep) {
        if (!fac_keep_.get()) MFX_TRY(fac_keep_.alloc(npad));
        hipLaunchKernelGGL(mfx_rec_build_fac, dim3(grid_for(npad)), dim3(256), 0, st_, keep, (const float*) nullptr, (uint32_t) cols_,
                           npad, fac_keep_.get());
        MFX_LAUNCH_CHECK();
    }
    if (sim_c_.get()) {
        if (!fac_cos_.get()) MFX_TRY(fac_cos_.alloc(npad));
        hipLaunchKernelGGL(mfx_rec_build_fac, dim3(grid_for(npad)), dim3(256), 0, st_, keep, (const float*) sim_c_.get(),
                           (uint32_t) cols_, npad, fac_cos_.get());
        MFX_LAUNCH_CHECK();
    }
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Recommender::set_item_filter(const uint8_t* keep, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_set_item_filter: bad memory space");
    MFX_TRY(use_device(device_));
    if (!keep) {
        keep_.release();
        fac_keep_.release();
        MFX_TRY(build_facs(nullptr));
        return ivf_refresh_fac();
    }
    DevBuf<uint8_t> nk;  // (the handle keeps its filter if this one cannot be taken)
    MFX_TRY(nk.alloc((size_t) cols_));
    MFX_TRY(nk.upload(keep, (size_t) cols_, space, st_));
    MFX_TRY(build_facs(nk.get()));
    keep_ = std::move(nk);
    return ivf_refresh_fac();
}

int Recommender::similar_setup() {
    if (sim_c_.get()) return MFX_OK;
    MFX_TRY(use_device(device_));
    MFX_TRY(ensure_hq());
    DevBuf<float> n2, c;
    DevBuf<uint32_t> id;
    MFX_TRY(n2.alloc((size_t) cols_));
    MFX_TRY(c.alloc((size_t) cols_));
    MFX_TRY(id.alloc((size_t) cols_ + 1));
    hipLaunchKernelGGL(mfx_rec_item_norms, dim3(grid_for((size_t) cols_ + 1)), dim3(256), 0, st_, hq_.get(), (uint32_t) cols_, (int) k_,
                       kt_, n2.get(), c.get(), id.get());
    MFX_LAUNCH_CHECK();
    MFX_HIP(hipStreamSynchronize(st_));
    sim_n2_ = std::move(n2); sim_id_ = std::move(id);
    sim_c_ = std::move(c);
    const int rc = build_facs(keep_.get());
    if (rc != MFX_OK) sim_c_.release();  // (not set up)
    return rc;
}

int Recommender::ensure_hq() {
    if (hq_.get()) return MFX_OK;
    DevBuf<float> hq;
    MFX_TRY(hq.alloc((size_t) cols_ * kt_));
    hipLaunchKernelGGL(mfx_rec_pack_hq, dim3(grid_for((size_t) cols_ * kt_)), dim3(256), 0, st_, hp_.get(), (uint32_t) cols_, (int) k_,
                       2 * kc_, nch_, kt_, hq.get());
    MFX_LAUNCH_CHECK();
    hq_ = std::move(hq);
    return MFX_OK;
}

int Recommender::item_norms(float* n2, float* c, mfx_memspace space) {
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_item_norms: bad memory space");
    MFX_REQUIRE(sim_c_.get(), "mfx_rec_item_norms: call mfx_rec_similar_setup first");
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (n2) MFX_HIP(hipMemcpyAsync(n2, sim_n2_.get(), sizeof(float) * (size_t) cols_, kind, st_));
    if (c) MFX_HIP(hipMemcpyAsync(c, sim_c_.get(), sizeof(float) * (size_t) cols_, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int Recommender::similar(int64_t nq, const uint32_t* query_items, int metric, int exclude_self, int32_t n_top, uint32_t* items,
                         float* scores, mfx_memspace space, int item_slices) {
    MFX_REQUIRE(sim_c_.get(), "mfx_rec_similar: call mfx_rec_similar_setup first");
    MFX_REQUIRE(metric == MFX_SIM_DOT || metric == MFX_SIM_COSINE, "mfx_rec_similar: unknown metric %d", metric);
    MFX_TRY(check_batch("mfx_rec_similar", "query_items", "nq", "cols", nq, query_items, cols_, n_top, space, item_slices));
    if (nq == 0) return MFX_OK;
    MFX_REQUIRE(items, "mfx_rec_similar: items is NULL");
    MFX_TRY(use_device(device_));
    const uint32_t nu = (uint32_t) nq;
    DevBuf<uint32_t> d_q;
    const uint32_t* dq = nullptr;
    MFX_TRY(stage_ids(query_items, nu, space, (uint32_t) cols_, "mfx_rec_similar: query item", d_q, &dq));
    const bool cosine = metric == MFX_SIM_COSINE;
    return topn(hq_.get(), nu, dq, exclude_self ? sim_id_.get() : nullptr, sim_id_.get(), n_top, items, scores, space, item_slices,
                cosine ? fac_cos_.get() : fac_keep_.get(), cosine ? sim_c_.get() : nullptr);
}

int Recommender::topn(const float* wp, uint32_t nu, const uint32_t* du, const uint32_t* ex_ptr, const uint32_t* ex_idx,
                      int32_t n_top, uint32_t* items, float* scores, mfx_memspace space, int item_slices, const float* fac,
                      const float* qfac, const TileSet* tiles) {
    hipStream_t st = st_;
    const TileSet own{hp_.get(), (uint32_t) cols_, nblk_};
    const TileSet& ts = tiles ? *tiles : own;
    int L = 64;
    while (L < n_top + 32) L <<= 1;

    const auto per_launch = [&](int s) {
        size_t qmax = kWorkspaceCap / ((size_t) s * L * 8);
        qmax = std::max<size_t>(kRecUsers, qmax / kRecUsers * kRecUsers);
        return (uint32_t) std::min<size_t>(nu, qmax);
    };
    // slices: as forced, or chosen for the user blocks of one launch, at most what one merge takes
    const int slices = item_slices ? item_slices : pick_slices(0, (per_launch(1) + kRecUsers - 1) / kRecUsers, kMaxMerge / n_top);
    const int bps = (ts.nblk + slices - 1) / slices;
    const uint32_t qc = per_launch(slices);

    DevBuf<uint32_t> d_items;
    DevBuf<float> d_scores, ls;
    DevBuf<uint32_t> li;
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
    MFX_TRY(ls.alloc((size_t) slices * qc * L));
    MFX_TRY(li.alloc((size_t) slices * qc * L));

    RecArgs a{};
    a.wp = wp;
    a.hp = ts.hp;
    a.users = du;
    a.ex_ptr = ex_ptr;
    a.ex_idx = ex_idx;
    a.cols = ts.cols;
    a.kt = kt_; a.nch = nch_; a.nblk = ts.nblk; a.bps = bps; a.n_top = n_top; a.L = L;
    a.ls = ls.get(); a.li = li.get();
    a.out_items = oi; a.out_scores = os;
    a.fac = fac; a.qfac = qfac;
    int P = 1;
    while (P < slices * n_top) P <<= 1;
    for (uint32_t q0 = 0; q0 < nu; q0 += qc) {
        a.q0 = q0;
        a.nq = std::min(qc, nu - q0);
        MFX_TRY(dispatch_kc(kc_, [&](auto kc) {
            constexpr int KC = decltype(kc)::value;
            const dim3 grid((a.nq + kRecUsers - 1) / kRecUsers, slices);
            if (a.fac) hipLaunchKernelGGL((mfx_rec_topn<KC, true>), grid, dim3(kRecThreads), 0, st, a);
            else hipLaunchKernelGGL((mfx_rec_topn<KC, false>), grid, dim3(kRecThreads), 0, st, a);
            MFX_LAUNCH_CHECK();
            return (int) MFX_OK;
        }));
        if (slices > 1) {
            hipLaunchKernelGGL(mfx_rec_merge, dim3(a.nq), dim3(64), (size_t) P * 8, st, a.ls, a.li, q0, a.nq, slices, L,
                               n_top, P, oi, os, du, qfac);
            MFX_LAUNCH_CHECK();
        }
    }
    if (space == MFX_HOST) {
        MFX_HIP(hipMemcpyAsync(items, oi, sizeof(uint32_t) * nu * n_top, hipMemcpyDeviceToHost, st));
        if (scores) MFX_HIP(hipMemcpyAsync(scores, os, sizeof(float) * nu * n_top, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    return MFX_OK;
}

int Recommender::merge_launch(const float* ls, const uint32_t* li, uint32_t q0, uint32_t nq, int slices, int L, int n_top,
                              uint32_t* out_items, float* out_scores) {
    int P = 1;
    while (P < slices * n_top) P <<= 1;
    hipLaunchKernelGGL(mfx_rec_merge, dim3(nq), dim3(64), (size_t) P * 8, st_, ls, li, q0, nq, slices, L, n_top, P, out_items, out_scores,
                       (const uint32_t*) nullptr, (const float*) nullptr);
    MFX_LAUNCH_CHECK();
    return MFX_OK;
}

int Recommender::pack_h_launch(const float* H, int layout, uint32_t cols, int nblk, float* hp) {
    hipLaunchKernelGGL(mfx_rec_pack_h, dim3(grid_for((size_t) nblk * kTile * kt_)), dim3(256), 0, st_, H, layout, cols, (int) k_, 2 * kc_, nch_,
                       nblk, hp);
    MFX_LAUNCH_CHECK();
    return MFX_OK;
}

// Every fold-in setup: validate (nothing is touched before, so a refused call leaves the previous setup usable), begin (the
// old plan goes as a whole before anything new is allocated; hx_ from the tiles), build what (method, objective) needs, and
// commit the finished plan.  A failure after validation leaves the handle "not set up".
int Recommender::fold_setup(const char* fn, const FoldSpec& s) {
    using M = FoldPlan::Method;
    using O = FoldPlan::Objective;
    const bool direct = s.method == M::Direct || s.method == M::DirectExact, blocks = s.method == M::Blocks, cg = s.method == M::Cg;
    const bool reg = s.objective == O::ImplicitReg;
    FoldPlan p;
    p.method = s.method;
    p.objective = s.objective;
    p.lambda = s.lambda;
    p.alpha = p.implicit() ? s.alpha : 0.f;
    if (reg) { p.alpha0 = s.alpha0; p.nu = s.nu; }
    if (p.iterative()) { p.cap = s.cap; p.tol = s.tol; }

    // the checks of every entry point in its order, each with its text (an entry point without alpha passes 0)
    if (cg) MFX_REQUIRE(s.arg != MFX_FOLD_ALS_EXACT, "%s: model MFX_FOLD_ALS_EXACT is an order of operations, not an objective; set up MFX_FOLD_ALS", fn);
    if (!blocks)
        MFX_REQUIRE(s.arg == MFX_FOLD_ALS || s.arg == MFX_FOLD_ALS_EXACT || s.arg == MFX_FOLD_CCD || s.arg == MFX_FOLD_IMPLICIT,
                    "%s: unknown model %d", fn, s.arg);
    MFX_REQUIRE(k_ <= (direct ? 128 : (int64_t) kIalsBlockMaxRank), "%s: %s ranks k <= %u (the handle has k = %lld)", fn,
                direct ? "fold-in solves" : blocks ? "block sweeps solve" : "conjugate gradients solve", direct ? 128u : kIalsBlockMaxRank,
                (long long) k_);
    MFX_REQUIRE(std::isfinite(s.lambda) && s.lambda > 0.f, "%s: lambda = %g (finite and > 0 required)", fn, (double) s.lambda);
    MFX_REQUIRE(std::isfinite(s.alpha) && s.alpha >= 0.f, "%s: alpha = %g (finite and >= 0 required)", fn, (double) s.alpha);
    if (reg) MFX_TRY(ialsr_check_params(fn, s.lambda, s.alpha0, s.nu, cols_, cols_));
    if (blocks && !p.implicit()) MFX_REQUIRE(s.arg == 0 || s.arg == 1, "%s: reg = %d (0 = lambda, 1 = lambda * entries of the row)", fn, s.arg);
    if (blocks) MFX_TRY(check_fold_sweeps(fn, s.block, s.cap, s.tol));
    if (cg) {
        MFX_REQUIRE(s.cap >= 1 && s.cap <= 1024, "%s: steps = %d (1 <= steps <= 1024)", fn, s.cap);
        MFX_REQUIRE(std::isfinite(s.tol) && s.tol >= 0.f, "%s: tol = %g (finite and >= 0 required)", fn, (double) s.tol);
    }

    MFX_TRY(use_device(device_));
    plan_ = FoldPlan();  // not set up until the new plan is through; the old one's buffers go before the new ones come
    hipStream_t st = st_;
    const size_t nh = ((size_t) cols_ + 1) * k_;
    if (!hx_.get()) MFX_TRY(hx_.alloc(nh));
    hipLaunchKernelGGL(mfx_rec_unpack_h, dim3(grid_for(nh)), dim3(256), 0, st, hp_.get(), (uint32_t) cols_, (int) k_, 2 * kc_, nch_, hx_.get());
    MFX_LAUNCH_CHECK();

    const uint32_t k = (uint32_t) k_, cols = (uint32_t) cols_, d = std::min<uint32_t>(s.block ? (uint32_t) s.block : ialsb_default_block(k), k);
    DevBuf<float> part;
    if (direct && p.implicit()) {  // the base Gramian as the trainer builds it: H^T H + lambda I, or under ImplicitReg fp32(alpha0 H^T H)
        MFX_TRY(part.alloc(ials_base_ws_floats(cols, k)));
        MFX_TRY(p.g.alloc((size_t) k * k));
        if (reg) MFX_TRY(ialsr_base_gramian(hx_.get(), cols, k, s.alpha0, part.get(), p.g.get(), st));
        else MFX_TRY(ials_base_gramian(hx_.get(), cols, k, s.lambda, part.get(), p.g.get(), st));
    } else if (blocks && p.implicit()) {  // the Gramian as the block trainer and mfx_ials_block_half build it, and what they pack once per half
        MFX_TRY(p.b.alloc(k, d, cols, 0, 0, 0, st));
        if (reg) MFX_TRY(ialsrb_gramian(p.b, hx_.get(), cols, s.alpha0, st));
        else MFX_TRY(ialsb_gramian(p.b, hx_.get(), cols, s.lambda, st));
        MFX_TRY(ialsb_pack_launch(p.b, hx_.get(), cols, st));
    } else if (blocks) {  // no G, only H block-major
        MFX_TRY(p.b.alloc_explicit(k, d, cols, 0, 0, 0, st));
        MFX_TRY(alsb_pack_launch(p.b, hx_.get(), cols, st));
    } else if (cg && p.implicit()) {  // G as the block trainer builds it (ialsb_gramian); Minv ~ G^-1 in fp64 on the host, rounded
        IalsBlock gb;
        MFX_TRY(gb.alloc(k, d, cols, 0, 0, 0, st));
        MFX_TRY(ialsb_gramian(gb, hx_.get(), cols, s.lambda, st));
        std::vector<float> g((size_t) k * k), minv((size_t) k * k);
        MFX_HIP(hipMemcpyAsync(g.data(), gb.G.get(), sizeof(float) * g.size(), hipMemcpyDeviceToHost, st));
        MFX_HIP(hipStreamSynchronize(st));
        MFX_TRY(foldcg_inverse(g.data(), k, minv.data()));
        MFX_TRY(p.minv.alloc(minv.size()));
        MFX_TRY(p.minv.upload(minv.data(), minv.size(), MFX_HOST, st));
        p.g = std::move(gb.G);
    }  // (the explicit objectives of Direct, DirectExact and Cg need hx_ alone)

    MFX_HIP(hipStreamSynchronize(st));
    p.b.gpart.release();  // (the tile partials of the block Gramian)
    plan_ = std::move(p);
    return MFX_OK;
}

int Recommender::fold_in(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, float* W_out,
                         int32_t n_top, uint32_t* items, float* scores, mfx_memspace space) {
    return fold_solve(nusers, nnz, ptr, idx, val, nullptr, W_out, nullptr, n_top, items, scores, space);
}

int Recommender::fold_in_warm(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, const float* W_init,
                              float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space) {
    MFX_REQUIRE(plan_.iterative(),
                "mfx_rec_fold_in_warm: call mfx_rec_fold_in_block_setup, mfx_rec_fold_in_block_setup_als or mfx_rec_fold_in_cg_setup first");
    return fold_solve(nusers, nnz, ptr, idx, val, W_init, W_out, sweeps_done, n_top, items, scores, space);
}

// The query rows of mfx_rec_fold_in and mfx_rec_explain (fn) as one half-sweep over H, with the chunking of training, checked:
// build() checks the pointers on the host and every index < cols on the device; then the exclusion check of mfx_rec_create
// (ids non-decreasing in a row) and the value checks of the model that was set up.
int Recommender::fold_rows(const char* fn, uint32_t nu, uint64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                           mfx_memspace space, AlsHalf& h) {
    hipStream_t st = st_;
    const std::string who = std::string(fn) + ": ", what = who + "value";
    MFX_TRY(h.build(nu, nnz, (uint32_t) cols_, ptr, idx, val, space, kAlsChunk, st));
    MFX_TRY(check_csr(h.ptr.get(), h.idx.get(), nu, (uint32_t) cols_, nnz, who.c_str(), "ptr", st));
    if (plan_.implicit()) MFX_TRY(ials_check_values(h.val.get(), h.nnz, plan_.alpha, what.c_str(), st));
    else if (plan_.iterative()) MFX_TRY(als_check_finite(h.val.get(), h.nnz, what.c_str(), st));  // (the direct explicit methods: none)
    return MFX_OK;
}

int Recommender::fold_rho(const AlsHalf& h, DevBuf<float>& rho) {
    if (plan_.objective != FoldPlan::Objective::ImplicitReg) return MFX_OK;
    MFX_TRY(rho.alloc(h.nseg));
    return ialsr_rho_launch(h, (uint32_t) cols_, plan_.lambda, plan_.alpha0, plan_.nu, rho.get(), st_);
}

// mfx_rec_explain: the fold-in rows by the multi-right-hand-side families of als_solver.hip (Y as mfx_rec_fold_in's family
// computes it, and Z = A^-1 h_target per target), then the totals and the ranked contributions (rec_candidates.hip).
int Recommender::explain(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                         const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out,
                         float* Z_out, mfx_memspace space) {
    const char* fn = "mfx_rec_explain";
    using M = FoldPlan::Method;
    MFX_REQUIRE(plan_.method != M::None, "%s: call mfx_rec_fold_in_setup (MFX_FOLD_ALS, MFX_FOLD_CCD, MFX_FOLD_IMPLICIT) or mfx_rec_fold_in_setup_reg first", fn);
    MFX_REQUIRE(plan_.method != M::DirectExact,
                "%s: the rows of MFX_FOLD_ALS_EXACT are not the bits of the MFMA system whose factor the explanation uses; set up MFX_FOLD_ALS", fn);
    MFX_REQUIRE(plan_.method != M::Cg,
                "%s: not after mfx_rec_fold_in_cg_setup (the split over the entries needs the factor of a closed-form solve); set up "
                "mfx_rec_fold_in_setup or mfx_rec_fold_in_setup_reg on a handle of rank <= 128", fn);
    MFX_REQUIRE(plan_.explains(),
                "%s: not after a block setup (a sweep is not a solve, the split over the entries does not hold); set up mfx_rec_fold_in_setup "
                "or mfx_rec_fold_in_setup_reg on a handle of rank <= 128", fn);
    return explain_run(fn, nusers, nnz, ptr, idx, val, n_targets, targets, n_expl, expl_items, expl_contrib, totals, W_out, Z_out, nullptr,
                       nullptr, space);
}

// mfx_rec_explain_cg: the fold-in rows by foldcg_launch as mfx_rec_fold_in runs it (cold start), Z = the iterates of
// A z = h_target by the same method over the pairs (rec_explain_cg.hip), then the same totals and contributions.
int Recommender::explain_cg(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                            const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out,
                            float* Z_out, int32_t* row_steps, int32_t* target_steps, mfx_memspace space) {
    const char* fn = "mfx_rec_explain_cg";
    MFX_REQUIRE(plan_.method == FoldPlan::Method::Cg,
                "%s: call mfx_rec_fold_in_cg_setup first (after a closed-form setup mfx_rec_explain explains; a block sweep is not a solve)", fn);
    return explain_run(fn, nusers, nnz, ptr, idx, val, n_targets, targets, n_expl, expl_items, expl_contrib, totals, W_out, Z_out, row_steps,
                       target_steps, space);
}

// What the two have in common; row_steps / target_steps: mfx_rec_explain_cg only.
int Recommender::explain_run(const char* fn, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                             int32_t n_targets, const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib,
                             float* totals, float* W_out, float* Z_out, int32_t* row_steps, int32_t* target_steps, mfx_memspace space) {
    MFX_REQUIRE(nusers >= 0 && nusers < (int64_t) 0xFFFFFFFFll, "%s: bad nusers %lld", fn, (long long) nusers);
    MFX_REQUIRE(nnz >= 0 && nnz < (int64_t) 0xFFFF0000ll, "%s: bad nnz %lld", fn, (long long) nnz);
    MFX_REQUIRE(n_targets >= 1 && n_targets <= kMaxExplain, "%s: n_targets must be in [1, %d] (got %d)", fn, kMaxExplain, n_targets);
    MFX_REQUIRE(n_expl >= 0 && n_expl <= kMaxExplain, "%s: n_expl must be in [0, %d] (got %d)", fn, kMaxExplain, n_expl);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "%s: bad memory space", fn);
    expl_s_[0] = expl_s_[1] = expl_s_[2] = 0.0;
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(ptr && (nnz == 0 || (idx && val)), "%s: null ptr / idx / val", fn);
    MFX_REQUIRE(targets, "%s: targets is NULL", fn);
    MFX_REQUIRE(n_expl == 0 || (expl_items && expl_contrib), "%s: expl_items or expl_contrib is NULL", fn);
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const uint32_t nu = (uint32_t) nusers, k = (uint32_t) k_;
    const size_t npair = (size_t) nu * n_targets;
    const bool host = space == MFX_HOST;
    AlsHalf h;
    MFX_TRY(fold_rows(fn, nu, (uint64_t) nnz, ptr, idx, val, space, h));
    DevBuf<uint32_t> d_targets;
    const uint32_t* dt = targets;
    if (host) {
        MFX_TRY(d_targets.alloc(npair));
        MFX_TRY(d_targets.upload(targets, npair, MFX_HOST, st));
        dt = d_targets.get();
    }
    MFX_TRY(explain_check_targets(fn, dt, npair, n_targets));
    const auto t1 = clk::now();

    DevBuf<float> Y, Z, ws, rho, d_contrib, d_totals;
    DevBuf<uint32_t> spd_fail, d_items;
    MFX_TRY(Y.alloc_zero((size_t) nu * k, st));
    MFX_TRY(Z.alloc_zero(npair * k, st));
    MFX_TRY(spd_fail.alloc_zero(1, st));
    const FoldPlan& p = plan_;
    const bool by_cg = p.method == FoldPlan::Method::Cg;  // (else Direct: explain and explain_cg let nothing else through)
    if (!by_cg) MFX_TRY(ws.alloc(std::max<size_t>(1, als_ws_floats(h.nslots, k))));
    const uint32_t x_rows = (uint32_t) cols_;
    MFX_TRY(fold_rho(h, rho));
    AlsMrhs m;
    m.targets = dt; m.n_targets = (uint32_t) n_targets; m.Z = Z.get();
    m.lambda = p.lambda; m.alpha = p.alpha; m.G = p.g.get();
    m.alpha0 = p.alpha0; m.rho = rho.get();
    DevBuf<int32_t> counts, pair_counts;
    if (by_cg) {  // the row as fold_solve runs it from zero, then the pairs
        if (row_steps) MFX_TRY(counts.alloc(nu));
        if (target_steps) MFX_TRY(pair_counts.alloc(npair));
        const FoldCg cg = p.cg();
        MFX_TRY(foldcg_launch(h, hx_.get(), x_rows, k, cg, Y.get(), false, counts.get(), spd_fail.get(), st));
        MFX_TRY(explaincg_launch(h, hx_.get(), x_rows, k, cg, dt, (uint32_t) n_targets, Z.get(), pair_counts.get(), st));
    } else {
        switch (p.objective) {
            case FoldPlan::Objective::Als: MFX_TRY(als_half_mrhs_launch(h, hx_.get(), x_rows, Y.get(), k, m, ws.get(), spd_fail.get(), st)); break;
            case FoldPlan::Objective::Ccd: MFX_TRY(als_half_nreg_mrhs_launch(h, hx_.get(), x_rows, Y.get(), k, m, ws.get(), spd_fail.get(), st)); break;
            case FoldPlan::Objective::Implicit: MFX_TRY(ials_half_mrhs_launch(h, hx_.get(), x_rows, Y.get(), k, m, ws.get(), spd_fail.get(), st)); break;
            case FoldPlan::Objective::ImplicitReg: MFX_TRY(ialsr_half_mrhs_launch(h, hx_.get(), x_rows, Y.get(), k, m, ws.get(), spd_fail.get(), st)); break;
        }
    }
    MFX_HIP(hipStreamSynchronize(st));
    const auto t2 = clk::now();

    const hipMemcpyKind out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (W_out) MFX_HIP(hipMemcpyAsync(W_out, Y.get(), sizeof(float) * (size_t) nu * k, out, st));
    if (Z_out) MFX_HIP(hipMemcpyAsync(Z_out, Z.get(), sizeof(float) * npair * k, out, st));
    if (row_steps) MFX_HIP(hipMemcpyAsync(row_steps, counts.get(), sizeof(int32_t) * (size_t) nu, out, st));
    if (target_steps) MFX_HIP(hipMemcpyAsync(target_steps, pair_counts.get(), sizeof(int32_t) * npair, out, st));
    uint32_t* oi = expl_items;
    float* oc = expl_contrib;
    float* ot = totals;
    const size_t nlist = npair * (size_t) n_expl;
    if (host) {
        if (n_expl) {
            MFX_TRY(d_items.alloc(nlist));
            MFX_TRY(d_contrib.alloc(nlist));
            oi = d_items.get(); oc = d_contrib.get();
        }
        if (totals) { MFX_TRY(d_totals.alloc(npair)); ot = d_totals.get(); }
    }
    MFX_TRY(explain_lists(h, dt, n_targets, Z.get(), Y.get(), n_expl, oi, oc, ot));
    if (host) {
        if (n_expl) {
            MFX_HIP(hipMemcpyAsync(expl_items, oi, sizeof(uint32_t) * nlist, hipMemcpyDeviceToHost, st));
            MFX_HIP(hipMemcpyAsync(expl_contrib, oc, sizeof(float) * nlist, hipMemcpyDeviceToHost, st));
        }
        if (totals) MFX_HIP(hipMemcpyAsync(totals, ot, sizeof(float) * npair, hipMemcpyDeviceToHost, st));
    }
    MFX_HIP(hipStreamSynchronize(st));
    const auto t3 = clk::now();
    expl_s_[0] = std::chrono::duration<double>(t1 - t0).count();
    expl_s_[1] = std::chrono::duration<double>(t2 - t1).count();
    expl_s_[2] = std::chrono::duration<double>(t3 - t2).count();
    return MFX_OK;
}

int Recommender::fold_solve(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, const float* W_init,
                            float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space) {
    using M = FoldPlan::Method;
    using O = FoldPlan::Objective;
    FoldPlan& p = plan_;
    MFX_REQUIRE(p.method != M::None, "mfx_rec_fold_in: call mfx_rec_fold_in_setup, mfx_rec_fold_in_block_setup, mfx_rec_fold_in_block_setup_als or "
                "mfx_rec_fold_in_cg_setup first");
    MFX_REQUIRE(nusers >= 0 && nusers < (int64_t) 0xFFFFFFFFll, "mfx_rec_fold_in: bad nusers %lld", (long long) nusers);
    MFX_REQUIRE(nnz >= 0 && nnz < (int64_t) 0xFFFF0000ll, "mfx_rec_fold_in: bad nnz %lld", (long long) nnz);
    MFX_REQUIRE(n_top >= 0 && n_top <= kMaxTop, "mfx_rec_fold_in: n_top must be in [0, %d] (got %d)", kMaxTop, n_top);
    MFX_REQUIRE(space == MFX_HOST || space == MFX_DEVICE, "mfx_rec_fold_in: bad memory space");
    fold_s_[0] = fold_s_[1] = fold_s_[2] = 0.0;
    if (nusers == 0) return MFX_OK;
    MFX_REQUIRE(ptr && (nnz == 0 || (idx && val)), "mfx_rec_fold_in: null ptr / idx / val");
    MFX_REQUIRE(n_top == 0 || items, "mfx_rec_fold_in: items is NULL");
    MFX_TRY(use_device(device_));
    hipStream_t st = st_;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const uint32_t nu = (uint32_t) nusers, k = (uint32_t) k_;
    AlsHalf h;
    MFX_TRY(fold_rows("mfx_rec_fold_in", nu, (uint64_t) nnz, ptr, idx, val, space, h));
    const auto t1 = clk::now();

    DevBuf<float> Y, ws, wq, rho;
    DevBuf<uint32_t> spd_fail;
    DevBuf<int32_t> counts;
    MFX_TRY(Y.alloc_zero((size_t) nu * k, st));
    MFX_TRY(spd_fail.alloc_zero(1, st));
    if (p.method == M::Direct) MFX_TRY(ws.alloc(std::max<size_t>(1, als_ws_floats(h.nslots, k))));
    const uint32_t x_rows = (uint32_t) cols_;
    MFX_TRY(fold_rho(h, rho));
    struct QueryWs {  // the per-query part of the plan's block state goes when the call returns
        IalsBlock& b;
        ~QueryWs() { b.P.release(); b.Z.release(); b.score.release(); b.ws.release(); }
    } query_ws{p.b};
    if (W_init) MFX_TRY(Y.upload(W_init, (size_t) nu * k, space, st));  // (both given to an iterative method only: fold_in_warm)
    if (sweeps_done) MFX_TRY(counts.alloc(nu));
    switch (p.method) {
        case M::None: break;  // (refused above)
        case M::Blocks:
            MFX_TRY(p.b.alloc_half(nu, h.nnz, h.nslots, st));
            if (p.implicit())
                MFX_TRY(ialsb_fold_launch(p.b, h, hx_.get(), x_rows, Y.get(), p.alpha, p.cap, p.tol, counts.get(), spd_fail.get(), st, p.alpha0,
                                          rho.get()));
            else
                MFX_TRY(alsb_fold_launch(p.b, h, hx_.get(), x_rows, Y.get(), p.lambda, p.objective == O::Ccd ? 1 : 0, p.cap, p.tol, counts.get(),
                                         spd_fail.get(), st));
            break;
        case M::Cg:
            MFX_TRY(foldcg_launch(h, hx_.get(), x_rows, k, p.cg(), Y.get(), W_init != nullptr, counts.get(), spd_fail.get(), st));
            break;
        case M::DirectExact:
            MFX_TRY(als_half_exact_launch(h, hx_.get(), Y.get(), k, p.lambda, spd_fail.get(), st));
            break;
        case M::Direct:
            switch (p.objective) {
                case O::Als: MFX_TRY(als_half_launch(h, hx_.get(), x_rows, Y.get(), k, p.lambda, ws.get(), spd_fail.get(), st)); break;
                case O::Ccd: MFX_TRY(als_half_nreg_launch(h, hx_.get(), x_rows, Y.get(), k, p.lambda, ws.get(), spd_fail.get(), st)); break;
                case O::Implicit:
                    MFX_TRY(ials_half_launch(h, hx_.get(), x_rows, Y.get(), k, p.g.get(), p.alpha, ws.get(), spd_fail.get(), st));
                    break;
                case O::ImplicitReg:
                    MFX_TRY(ialsr_half_launch(h, hx_.get(), x_rows, Y.get(), k, p.g.get(), p.alpha, p.alpha0, rho.get(), ws.get(), spd_fail.get(), st));
                    break;
            }
            break;
    }
    MFX_HIP(hipStreamSynchronize(st));
    const auto t2 = clk::now();

    if (W_out)
        MFX_HIP(hipMemcpyAsync(W_out, Y.get(), sizeof(float) * (size_t) nu * k,
                               space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (sweeps_done)
        MFX_HIP(hipMemcpyAsync(sweeps_done, counts.get(), sizeof(int32_t) * (size_t) nu,
                               space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    if (n_top > 0) {
        MFX_TRY(wq.alloc((size_t) nu * kt_));
        hipLaunchKernelGGL(mfx_rec_pack_w, dim3(grid_for((size_t) nu * kt_)), dim3(256), 0, st, Y.get(), 1, nu, (int) k, kt_,
                           wq.get());
        MFX_LAUNCH_CHECK();
        MFX_TRY(topn(wq.get(), nu, nullptr, h.ptr.get(), h.idx.get(), n_top, items, scores, space, 0, fac_keep_.get(), nullptr));
    }
    MFX_HIP(hipStreamSynchronize(st));
    const auto t3 = clk::now();
    fold_s_[0] = std::chrono::duration<double>(t1 - t0).count();
    fold_s_[1] = std::chrono::duration<double>(t2 - t1).count();
    fold_s_[2] = std::chrono::duration<double>(t3 - t2).count();
    return MFX_OK;
}

void TopnAcc::add(const uint32_t* pos, size_t nhits, size_t nrel, int64_t n_top) {
    ++kept;
    double dcg = 0;
    for (size_t x = 0; x < nhits; ++x) dcg += 1.0 / std::log2((double) pos[x] + 2.0);
    double idcg = 0;
    const int64_t ideal = std::min<int64_t>(n_top, (int64_t) nrel);
    for (int64_t jj = 0; jj < ideal; ++jj) idcg += 1.0 / std::log2((double) jj + 2.0);
    const double hits = (double) nhits;
    hr += hits > 0 ? 1.0 : 0.0;
    prec += hits / n_top;
    rec += hits / (double) nrel;
    ndcg += dcg / idcg;
}

void TopnAcc::mean(double out[4]) const {
    const double d = kept ? (double) kept : 1.0;
    out[0] = kept ? hr / d : 0.0;
    out[1] = kept ? prec / d : 0.0;
    out[2] = kept ? rec / d : 0.0;
    out[3] = kept ? ndcg / d : 0.0;
}

int topn_metrics(int64_t nusers, const uint32_t* users, int32_t n_top, const uint32_t* items, const mfx_coo* T,
                 float min_rating, double out[4], int64_t* users_evaluated) {
    MFX_REQUIRE(nusers >= 0 && n_top >= 1 && (nusers == 0 || items) && T && out, "mfx_topn_metrics: bad argument");
    MFX_REQUIRE(T->nnz == 0 || (T->row && T->col && T->val), "mfx_topn_metrics: null test array");
    MFX_REQUIRE(!std::isnan(min_rating), "mfx_topn_metrics: min_rating is NaN");
    // R_u of the listed users: distinct test items with value >= min_rating
    std::unordered_map<uint32_t, std::vector<uint32_t>> rel;
    rel.reserve((size_t) nusers);
    for (int64_t s = 0; s < nusers; ++s) rel.emplace(users ? users[s] : (uint32_t) s, std::vector<uint32_t>());
    for (int64_t p = 0; p < T->nnz; ++p) {
        if (!(T->val[p] >= min_rating)) continue;
        auto it = rel.find(T->row[p]);
        if (it != rel.end()) it->second.push_back(T->col[p]);
    }
    for (auto& kv : rel) {
        std::sort(kv.second.begin(), kv.second.end());
        kv.second.erase(std::unique(kv.second.begin(), kv.second.end()), kv.second.end());
    }
    TopnAcc acc;
    std::vector<uint32_t> seen, pos;
    for (int64_t s = 0; s < nusers; ++s) {
        const std::vector<uint32_t>& R = rel[users ? users[s] : (uint32_t) s];
        if (R.empty()) continue;
        seen.clear();
        pos.clear();
        for (int32_t jj = 0; jj < n_top; ++jj) {
            const uint32_t it = items[(size_t) s * n_top + jj];
            if (it == kPad || !std::binary_search(R.begin(), R.end(), it)) continue;
            if (std::find(seen.begin(), seen.end(), it) != seen.end()) continue;  // a hit counts once
            seen.push_back(it);
            pos.push_back((uint32_t) jj);
        }
        acc.add(pos.data(), pos.size(), R.size(), n_top);
    }
    acc.mean(out);
    const int64_t kept = acc.kept;
    if (users_evaluated) *users_evaluated = kept;
    return MFX_OK;
}

}  // namespace mfx
