// als_host.hip -- host orchestration of the ALS solvers: the work items of an orientation (AlsHalf::build), the resident
// solver (AlsSolver) and the one-shot entry points.  The kernels and their launches are als_solver.hip and the files that
// compile it once more per family.
#include "als_solver.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>

#include "ccd_kernels.hpp"

namespace mfx {

size_t als_ws_floats(uint32_t nslots, uint32_t k) {
    const size_t nt = (k + 31) / 32;
    return (size_t) nslots * (nt * (nt + 1) / 2 * 1024 + nt * 64);
}

int AlsHalf::build(uint32_t nseg_, uint64_t nnz_, uint32_t G, const uint32_t* ptr_in, const uint32_t* idx_in,
                   const float* val_in, mfx_memspace space, uint32_t chunk, hipStream_t st) {
    MFX_REQUIRE(nnz_ == 0 || (idx_in && val_in), "null index / value array with %llu non-zeros", (unsigned long long) nnz_);
    nseg = nseg_;
    nnz = nnz_;
    std::vector<uint32_t> hp((size_t) nseg + 1);
    if (space == MFX_DEVICE) MFX_HIP(hipMemcpy(hp.data(), ptr_in, sizeof(uint32_t) * hp.size(), hipMemcpyDeviceToHost));
    else memcpy(hp.data(), ptr_in, sizeof(uint32_t) * hp.size());
    MFX_REQUIRE(hp[0] == 0 && hp[nseg] == nnz, "segment pointer array does not span [0, nnz]");
    std::vector<AlsItem> it;
    std::vector<AlsReduce> rd;
    it.reserve((size_t) nseg + nnz / chunk + 1);
    uint32_t slots = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        MFX_REQUIRE(hp[s] <= hp[s + 1], "segment pointer array is not monotone at %u", s);
        const uint32_t lo = hp[s], hi = hp[s + 1];
        if (hi - lo <= chunk) {
            it.push_back(AlsItem{s, lo, hi, -1});
        } else {
            const uint32_t pieces = (hi - lo + chunk - 1) / chunk;
            rd.push_back(AlsReduce{s, slots, pieces});
            for (uint32_t c = 0; c < pieces; ++c)
                it.push_back(AlsItem{s, lo + c * chunk, std::min(hi, lo + (c + 1) * chunk), (int32_t) (slots + c)});
            slots += pieces;
        }
    }
    nitems = (uint32_t) it.size();
    nreduces = (uint32_t) rd.size();
    nslots = slots;
    MFX_TRY(ptr.alloc(hp.size())); MFX_TRY(ptr.upload(hp.data(), hp.size(), MFX_HOST, st));
    // kAlsEntryPad extra entries each: entry nnz is (G, 0) = "the all-zero row of X, rating 0", the stand-in of k_als_gram<NT>
    // for positions past a segment's end; the rest is zero padding that k_als_gram16 may read (and ignore) past the
    // last segment
    MFX_TRY(idx.alloc(nnz + kAlsEntryPad)); MFX_TRY(idx.upload(idx_in, nnz, space, st));
    MFX_TRY(val.alloc(nnz + kAlsEntryPad)); MFX_TRY(val.upload(val_in, nnz, space, st));
    MFX_HIP(hipMemsetAsync(idx.get() + nnz, 0, sizeof(uint32_t) * kAlsEntryPad, st));
    MFX_HIP(hipMemsetAsync(val.get() + nnz, 0, sizeof(float) * kAlsEntryPad, st));
    MFX_HIP(hipMemcpyAsync(idx.get() + nnz, &G, sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MFX_TRY(items.alloc(nitems ? nitems : 1)); MFX_TRY(items.upload(it.data(), nitems, MFX_HOST, st));
    MFX_TRY(reduces.alloc(nreduces ? nreduces : 1)); MFX_TRY(reduces.upload(rd.data(), nreduces, MFX_HOST, st));
    MFX_HIP(hipStreamSynchronize(st));
    // the Gramian kernels use idx[q] as a row of X without further checks
    MFX_TRY(check_index_range(idx.get(), nnz, G, "ALS gather index", st));
    return MFX_OK;
}


// ------------------------------------------------------------------------------------------------
// The pairs that exist: the family's name in the texts, the names of kernel_times (the two half-sweeps, the base Gramians of H
// and W, their inverses; what a pair never times is never read).  A new (method, objective) pair is a row here, a case in
// als_plan_half and, where it keeps buffers of its own, in AlsPlan::alloc.
struct AlsPair {
    AlsPlan::Method method;
    AlsPlan::Objective objective;
    const char* family;
    const char* names[6];
};
#define MFX_ALS_NAMES(p) {p "_half_rows(W over H)", p "_half_cols(H over W)", p "_base_gram(H)", p "_base_gram(W)", p "_inverse(H)", p "_inverse(W)"}
using PM = AlsPlan::Method;
using PO = AlsPlan::Objective;
static const AlsPair kAlsPairs[] = {
    {PM::Direct, PO::Als, "ALS", MFX_ALS_NAMES("als")},
    {PM::DirectExact, PO::Als, "ALS", MFX_ALS_NAMES("als")},
    {PM::Direct, PO::Implicit, "implicit ALS", MFX_ALS_NAMES("ials")},
    {PM::Direct, PO::ImplicitReg, "implicit ALS", MFX_ALS_NAMES("ials")},
    {PM::Blocks, PO::Als, "explicit ALS by block sweeps", MFX_ALS_NAMES("alsb")},
    {PM::Blocks, PO::Ccd, "explicit ALS by block sweeps", MFX_ALS_NAMES("alsb")},
    {PM::Blocks, PO::Implicit, "implicit ALS by block sweeps", MFX_ALS_NAMES("ialsb")},
    {PM::Blocks, PO::ImplicitReg, "implicit ALS by block sweeps", MFX_ALS_NAMES("ialsb")},
    {PM::Cg, PO::Implicit, "implicit ALS by conjugate gradients", MFX_ALS_NAMES("ialscg")},
};
#undef MFX_ALS_NAMES
static const AlsPair* als_pair(PM m, PO o) {
    for (const AlsPair& pr : kAlsPairs)
        if (pr.method == m && pr.objective == o) return &pr;
    return nullptr;
}
static uint32_t als_max_rank(PM m) { return m == PM::Blocks || m == PM::Cg ? kIalsBlockMaxRank : 128u; }

// The checks of the fourteen entry points, each in the order and with the text it always had.  What differs between them
// beyond the pair: a create checks alpha first and a half after the pair's own parameters; reg and lambda of the explicit
// block sweeps are named by the family in the create and by the function in the half; the sizes of a half are checked late
// (mfx_als_half: first).  mfx_als_create checks its rank with the matrix (AlsSolver::init).
int als_spec_check(const AlsSpec& s, int64_t k, float lambda, int64_t rows, int64_t cols, int64_t nnz) {
    const AlsPair* pr = als_pair(s.method, s.objective);
    MFX_REQUIRE(pr, "%s: there is no ALS trainer of method %d on objective %d", s.fn, (int) s.method, (int) s.objective);
    const char* fam = pr->family;
    const bool implicit = s.objective == PO::Implicit || s.objective == PO::ImplicitReg, reg = s.objective == PO::ImplicitReg;
    auto sizes = [&]() -> int {
        MFX_REQUIRE(!s.half || (rows < (int64_t) 0xFFFFFFFFll && cols < (int64_t) 0xFFFFFFFFll && nnz < (int64_t) 0xFFFF0000ll),
                    "%s: sizes exceed the 32-bit index range", s.fn);
        return MFX_OK;
    };
    auto alpha = [&]() -> int {
        MFX_REQUIRE(!implicit || (std::isfinite(s.alpha) && s.alpha >= 0.f), "%s: alpha = %g (finite and >= 0 required)", s.fn, (double) s.alpha);
        return MFX_OK;
    };
    if (!implicit && s.method != PM::Blocks) {  // Direct or DirectExact on Als
        MFX_TRY(sizes());
        MFX_REQUIRE(!s.half || k <= 128, "ALS: rank k = %lld not supported (1 <= k <= 128)", (long long) k);
        return MFX_OK;
    }
    if (!s.half) {
        MFX_REQUIRE(!(s.method == PM::Cg || reg) || s.space == MFX_HOST || s.space == MFX_DEVICE, "%s: bad memory space", s.fn);
        MFX_TRY(alpha());
    }
    MFX_REQUIRE(k >= 1 && k <= (int64_t) als_max_rank(s.method), "%s: rank k = %lld not supported (1 <= k <= %u)", fam, (long long) k,
                als_max_rank(s.method));
    if (s.method == PM::Blocks) {
        MFX_REQUIRE(s.block >= 0 && s.block <= (int32_t) kIalsBlockMaxBlock, "%s: block = %d (0 = chosen from k, else 1 <= block <= %u)", fam,
                    s.block, kIalsBlockMaxBlock);
        if (!implicit) {
            MFX_REQUIRE(s.reg == 0 || s.reg == 1, "%s: reg = %d (0 = lambda, 1 = lambda * entries of the segment)", s.half ? s.fn : fam, s.reg);
            MFX_REQUIRE(std::isfinite(lambda) && lambda > 0.f, "%s: lambda = %g (finite and > 0 required)", s.half ? s.fn : fam, (double) lambda);
        }
    }
    if (s.method == PM::Cg) {
        MFX_REQUIRE(s.cap >= 1, "%s: steps = %d (>= 1 required)", fam, s.cap);
        MFX_REQUIRE(std::isfinite(s.tol) && s.tol >= 0.f, "%s: tol = %g (finite and >= 0 required)", fam, (double) s.tol);
    }
    if (s.half) MFX_TRY(alpha());
    else MFX_REQUIRE(s.schedule == 1, "%s: schedule must be 1 (there is no as-written mode)", reg ? s.fn : fam);
    MFX_TRY(sizes());
    if (reg) MFX_TRY(ialsr_check_params(s.fn, lambda, s.alpha0, s.nu, rows, cols));
    return MFX_OK;
}

int AlsPlan::set(const AlsSpec& s, uint32_t k_, float lambda_) {
    pair = als_pair(s.method, s.objective);
    MFX_REQUIRE(pair, "%s: there is no ALS trainer of method %d on objective %d", s.fn, (int) s.method, (int) s.objective);
    method = s.method; objective = s.objective;
    k = k_; lambda = lambda_;
    alpha = implicit() ? s.alpha : 0.f;
    alpha0 = s.alpha0; nu = s.nu;
    if (method == Method::Blocks) block = std::min<uint32_t>(s.block ? (uint32_t) s.block : ialsb_default_block(k), k);
    cap = s.cap; tol = s.tol;
    return MFX_OK;
}

size_t AlsPlan::loss_ws_doubles() const { return objective == Objective::ImplicitReg ? ialsr_loss_ws_doubles(k) : ials_loss_ws_doubles(k); }

int AlsPlan::alloc(uint32_t max_rows_x, uint32_t max_seg, uint64_t nnz, uint32_t nslots, hipStream_t st) {
    switch (method) {
        case Method::Blocks:
            return implicit() ? bs.alloc(k, block, max_rows_x, max_seg, nnz, nslots, st)
                              : bs.alloc_explicit(k, block, max_rows_x, max_seg, nnz, nslots, st);
        case Method::Cg:
            MFX_TRY(cgs.alloc(k, max_rows_x, max_seg, nslots, cap));
            MFX_TRY(cg_fail.alloc_zero(4, st));
            return cg_cnt.alloc_zero(6, st);
        default:
            MFX_TRY(ws.alloc(std::max<size_t>(1, als_ws_floats(nslots, k))));
            if (!implicit()) return MFX_OK;
            MFX_TRY(G.alloc((size_t) k * k));
            return gpart.alloc(ials_base_ws_floats(max_rows_x, k));
    }
}

int AlsPlan::check_values(const AlsHalf& h, const char* what, hipStream_t st) const {
    if (implicit()) return ials_check_values(h.val.get(), h.nnz, alpha, what, st);
    if (method == Method::Blocks) return als_check_finite(h.val.get(), h.nnz, what, st);
    return MFX_OK;
}

int als_plan_half(AlsPlan& pl, const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, bool warm, const float* rho, hipEvent_t ev_gram,
                  hipEvent_t ev_inv, uint32_t* fails, unsigned long long* stats, hipStream_t st, unsigned long long* phases) {
    const uint32_t k = pl.k;
    constexpr auto pair_of = [](PM m, PO o) { return (int) m * 4 + (int) o; };
    auto gram_done = [&]() -> int {
        if (ev_gram) MFX_HIP(hipEventRecord(ev_gram, st));
        return MFX_OK;
    };
    switch (pair_of(pl.method, pl.objective)) {
        case pair_of(PM::Direct, PO::Als):
            return als_half_launch(h, X, x_rows, Y, k, pl.lambda, pl.ws.get(), fails, st, phases);
        case pair_of(PM::DirectExact, PO::Als):  // as written: the reference's arithmetic, bit for bit (als_exact.hip)
            return als_half_exact_launch(h, X, Y, k, pl.lambda, fails, st);
        case pair_of(PM::Direct, PO::Implicit):
            MFX_TRY(ials_base_gramian(X, x_rows, k, pl.lambda, pl.gpart.get(), pl.G.get(), st));
            MFX_TRY(gram_done());
            return ials_half_launch(h, X, x_rows, Y, k, pl.G.get(), pl.alpha, pl.ws.get(), fails, st);
        case pair_of(PM::Direct, PO::ImplicitReg):
            MFX_TRY(ialsr_base_gramian(X, x_rows, k, pl.alpha0, pl.gpart.get(), pl.G.get(), st));
            MFX_TRY(gram_done());
            return ialsr_half_launch(h, X, x_rows, Y, k, pl.G.get(), pl.alpha, pl.alpha0, rho, pl.ws.get(), fails, st);
        case pair_of(PM::Blocks, PO::Als):
        case pair_of(PM::Blocks, PO::Ccd):
            return alsb_half_launch(pl.bs, h, X, x_rows, Y, pl.lambda, pl.objective == PO::Ccd, fails, st);
        case pair_of(PM::Blocks, PO::Implicit):
            MFX_TRY(ialsb_gramian(pl.bs, X, x_rows, pl.lambda, st));
            MFX_TRY(gram_done());
            return ialsb_half_launch(pl.bs, h, X, x_rows, Y, pl.alpha, fails, st);
        case pair_of(PM::Blocks, PO::ImplicitReg):
            MFX_TRY(ialsrb_gramian(pl.bs, X, x_rows, pl.alpha0, st));
            MFX_TRY(gram_done());
            return ialsb_half_launch(pl.bs, h, X, x_rows, Y, pl.alpha, fails, st, pl.alpha0, rho);
        case pair_of(PM::Cg, PO::Implicit):
            return ialscg_half_launch(pl.cgs, h, X, x_rows, Y, warm, pl.lambda, pl.alpha, pl.cap, pl.tol, fails, stats, ev_gram, ev_inv, st);
    }
    return fail(MFX_ERR_INVALID, "ALS: no half-sweep of method %d on objective %d", (int) pl.method, (int) pl.objective);
}

// ------------------------------------------------------------------------------------------------
int AlsSolver::create(AlsSolver** out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space, const mfx_als_shard* shard,
                      const AlsSpec& spec) {
    MFX_REQUIRE(out && R && p, "%s: null argument", spec.fn);
    AlsSpec s = spec;
    s.schedule = p->schedule;
    s.space = space;
    if (s.method == PM::Direct && s.objective == PO::Als && p->schedule == 0) s.method = PM::DirectExact;
    MFX_TRY(als_spec_check(s, p->k, p->lambda, R->rows, R->cols, R->nnz));
    std::unique_ptr<AlsSolver> a(new AlsSolver());
    MFX_TRY(a->init(R, T, p, space, shard, s));
    *out = a.release();
    return MFX_OK;
}

AlsSolver::~AlsSolver() {
    (void) hipSetDevice(device_);
    for (hipEvent_t& e : ev_)
        if (e) (void) hipEventDestroy(e);
    if (st_) {
        (void) hipStreamSynchronize(st_);
        (void) hipStreamDestroy(st_);
    }
}

// Block boundaries of every rank, gathered through the communicator itself: each rank contributes
// its own (lo, hi) into a zeroed vector and a sum all-reduce fills in the rest.
static int gather_bounds(mfx_comm_s* c, int64_t lo, int64_t hi, std::vector<int64_t>* bounds, hipStream_t st) {
    DevBuf<double> d;
    std::vector<double> h((size_t) c->nranks * 2, 0.0);
    h[(size_t) c->rank * 2] = (double) lo;
    h[(size_t) c->rank * 2 + 1] = (double) hi;
    MFX_TRY(d.alloc(h.size()));
    MFX_TRY(d.upload(h.data(), h.size(), MFX_HOST, st));
    MFX_TRY(comm_allreduce_f64(c, d.get(), h.size(), st));
    MFX_HIP(hipMemcpyAsync(h.data(), d.get(), sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
    MFX_HIP(hipStreamSynchronize(st));
    bounds->assign((size_t) c->nranks + 1, 0);
    for (int r = 0; r < c->nranks; ++r) {
        MFX_REQUIRE((int64_t) h[(size_t) r * 2] == (*bounds)[r], "ALS shards are not contiguous in rank order");
        (*bounds)[(size_t) r + 1] = (int64_t) h[(size_t) r * 2 + 1];
    }
    return MFX_OK;
}

int AlsSolver::init(const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space, const mfx_als_shard* shard, const AlsSpec& spec) {
    MFX_REQUIRE(R->rows > 0 && R->cols > 0 && R->nnz >= 0, "bad matrix shape");
    MFX_REQUIRE(R->rows < (int64_t) 0xFFFFFFFFll && R->cols < (int64_t) 0xFFFFFFFFll &&
                    R->nnz < (int64_t) 0xFFFF0000ll, "matrix exceeds 32-bit index range");
    MFX_REQUIRE(p->k >= 1 && p->k <= als_max_rank(spec.method), "ALS: rank k = %u not supported (1 <= k <= 128)", p->k);
    MFX_REQUIRE(R->csc_col_ptr && R->csr_row_ptr, "null CSR/CSC pointer array");
    p_ = *p;
    device_ = p->device;
    MFX_TRY(use_device(device_));
    MFX_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    for (hipEvent_t& e : ev_) MFX_HIP(hipEventCreate(&e));
    m_ = (uint32_t) R->rows; n_ = (uint32_t) R->cols; k_ = p->k;
    uint32_t lrows = m_, lcols = n_;
    uint64_t nnz_rows = (uint64_t) R->nnz, nnz_cols = (uint64_t) R->nnz;
    if (shard && shard->comm) {
        MFX_REQUIRE(space == MFX_HOST, "sharded ALS takes host pointers");
        MFX_REQUIRE(0 <= shard->row_lo && shard->row_lo <= shard->row_hi && shard->row_hi <= R->rows &&
                        0 <= shard->col_lo && shard->col_lo <= shard->col_hi && shard->col_hi <= R->cols,
                    "bad ALS shard ranges");
        comm_ = shard->comm;
        row_lo_ = (uint32_t) shard->row_lo; col_lo_ = (uint32_t) shard->col_lo;
        lrows = (uint32_t) (shard->row_hi - shard->row_lo); lcols = (uint32_t) (shard->col_hi - shard->col_lo);
        nnz_rows = R->csr_row_ptr[lrows]; nnz_cols = R->csc_col_ptr[lcols];
        global_test_nnz_ = shard->global_test_nnz;
        row_hi_ = (uint32_t) shard->row_hi; col_hi_ = (uint32_t) shard->col_hi;
        // No collective in here (mfx.h, mfx_comm_agree): a rank that fails any check of its own setup must not leave
        // the others inside one.  The block boundaries of the other ranks are gathered by the first iterate() call,
        // which every rank reaches only after mfx_comm_agree reported that everybody's setup succeeded.
    }
    // W-half walks CSR rows with csr_val (src/ALS.cpp:132), H-half walks CSC columns
    MFX_TRY(rows_.build(lrows, nnz_rows, n_, R->csr_row_ptr, R->csr_col_idx, R->csr_val, space, kAlsChunk, st_));
    MFX_TRY(cols_.build(lcols, nnz_cols, m_, R->csc_col_ptr, R->csc_row_idx, R->csc_val, space, kAlsChunk, st_));
    // one extra, all-zero row each: the Gramian kernel gathers it for positions past a segment's end
    MFX_TRY(W_.alloc_zero(((size_t) m_ + 1) * k_, st_));
    MFX_TRY(H_.alloc_zero(((size_t) n_ + 1) * k_, st_));
    MFX_TRY(spd_fail_.alloc_zero(1, st_));
    if (std::getenv("MFX_ALS_PHASES")) { MFX_TRY(phases_.alloc_zero((size_t) kPhaseCopies * 8, st_)); }
    nnz_test_ = T ? T->nnz : 0;
    if (!comm_) global_test_nnz_ = nnz_test_;
    if (nnz_test_ > 0) {
        MFX_REQUIRE(T->row && T->col && T->val, "null test array");
        MFX_TRY(t_row_.alloc(nnz_test_)); MFX_TRY(t_row_.upload(T->row, nnz_test_, space, st_));
        MFX_TRY(t_col_.alloc(nnz_test_)); MFX_TRY(t_col_.upload(T->col, nnz_test_, space, st_));
        MFX_TRY(t_val_.alloc(nnz_test_)); MFX_TRY(t_val_.upload(T->val, nnz_test_, space, st_));
        MFX_TRY(check_index_range(t_row_.get(), (uint64_t) nnz_test_, m_, "test-set row", st_));
        MFX_TRY(check_index_range(t_col_.get(), (uint64_t) nnz_test_, n_, "test-set column", st_));
    }
    MFX_TRY(rmse_partials_.alloc_zero(kRmseBlocks, st_));
    MFX_TRY(rmse_sum_.alloc_zero(1, st_));
    // the pair: the value checks on the CSR copy, then on the CSC copy, then its buffers for the larger of the two halves
    MFX_TRY(plan_.set(spec, k_, p_.lambda));
    const char* fam = plan_.implicit() ? "implicit ALS" : plan_.pair->family;
    MFX_TRY(plan_.check_values(rows_, (std::string(fam) + ": R (CSR) value").c_str(), st_));
    MFX_TRY(plan_.check_values(cols_, (std::string(fam) + ": R (CSC) value").c_str(), st_));
    MFX_REQUIRE(plan_.method != PM::Blocks || rows_.nnz == cols_.nnz, "%s: the two orientations hold %llu and %llu entries", plan_.pair->family,
                (unsigned long long) rows_.nnz, (unsigned long long) cols_.nnz);
    MFX_TRY(plan_.alloc(std::max(m_, n_), std::max(m_, n_), rows_.nnz, std::max(rows_.nslots, cols_.nslots), st_));
    if (plan_.implicit()) {
        // (block sweeps and conjugate gradients: on the first loss(), up to 1 GB at k = 1024)
        if (plan_.direct()) MFX_TRY(plan_.loss_ws.alloc(plan_.loss_ws_doubles()));
        MFX_TRY(loss_.alloc_zero(1, st_));
    }
    if (plan_.objective == PO::ImplicitReg) {  // rho of every row over the n_ items and of every column over the m_ users
        MFX_TRY(plan_.rho_rows.alloc(m_)); MFX_TRY(plan_.rho_cols.alloc(n_));
        MFX_TRY(ialsr_rho_launch(rows_, n_, p_.lambda, plan_.alpha0, plan_.nu, plan_.rho_rows.get(), st_));
        MFX_TRY(ialsr_rho_launch(cols_, m_, p_.lambda, plan_.alpha0, plan_.nu, plan_.rho_cols.get(), st_));
    }
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}


// After a half-sweep every rank holds only its own block of the factor it just solved: ONE grouped exchange
// (every owner broadcasts its block inside a single ncclGroupStart / End) makes the replica whole again.
int AlsSolver::exchange(float* X, const std::vector<int64_t>& bounds) {
    MFX_REQUIRE(shards_met_ && bounds.size() == (size_t) comm_->nranks + 1, "ALS exchange without validated shard boundaries");
    std::vector<int64_t> elems(bounds.size());
    for (size_t r = 0; r < bounds.size(); ++r) elems[r] = bounds[r] * (int64_t) k_;
    return comm_allgather_blocks_f32(comm_, X, elems.data(), st_);
}

// First iterate() of a sharded solve: everyone's block boundaries.  Every rank sees the same gathered vector, so a
// partition that is not contiguous in rank order or does not cover the matrix fails on ALL ranks alike.
// The boundaries are gathered into LOCAL vectors and become the solver's only after every check has passed: a failed
// first iterate() (not contiguous / does not cover) must leave the solver in the state "not met" -- round 3 keyed on
// row_bounds_.empty(), which gather_bounds had already filled, so a second iterate() went on to exchange() with
// unvalidated (or, for the columns, missing) boundaries.
int AlsSolver::meet_shards() {
    shards_met_ = false;
    std::vector<int64_t> rb, cb;
    MFX_TRY(gather_bounds(comm_, row_lo_, row_hi_, &rb, st_));
    MFX_TRY(gather_bounds(comm_, col_lo_, col_hi_, &cb, st_));
    const size_t want = (size_t) comm_->nranks + 1;
    MFX_REQUIRE(rb.size() == want && cb.size() == want, "ALS shards: gathered %zu / %zu boundaries for %d ranks", rb.size(), cb.size(), comm_->nranks);
    MFX_REQUIRE(rb.back() == (int64_t) m_ && cb.back() == (int64_t) n_, "ALS shards do not cover the matrix");
    row_bounds_.swap(rb);
    col_bounds_.swap(cb);
    shards_met_ = true;
    return MFX_OK;
}

int AlsSolver::print_phases(const char* what) {
    unsigned long long h[8] = {};
    std::vector<unsigned long long> all((size_t) kPhaseCopies * 8);
    MFX_HIP(hipStreamSynchronize(st_));
    MFX_HIP(hipMemcpy(all.data(), phases_.get(), sizeof(unsigned long long) * all.size(), hipMemcpyDeviceToHost));
    MFX_HIP(hipMemset(phases_.get(), 0, sizeof(unsigned long long) * all.size()));
    for (size_t c = 0; c < kPhaseCopies; ++c)
        for (int q = 0; q < 8; ++q) h[q] += all[c * 8 + q];
    const double n = h[4] ? (double) h[4] : 1.0;
    fprintf(stderr, "[mfx als phases] %-22s systems %llu; s_memtime clocks per system: gramian %.0f, staging %.0f, factorisation %.0f (k > 64: MFMA updates %.0f, "
            "diagonal passes %.0f, passes below %.0f), solves %.0f\n", what, h[4], h[0] / n, h[1] / n, h[2] / n, h[5] / n, h[6] / n, h[7] / n, h[3] / n);
    return MFX_OK;
}

int AlsSolver::set_factors(const float* W, const float* H, mfx_memspace space) {
    // W's initial content is irrelevant (overwritten before its first read, src/ALS.cpp:98-158)
    MFX_REQUIRE(H, "mfx_als_set_factors: H is required");
    MFX_TRY(use_device(device_));
    if (W) MFX_TRY(W_.upload(W, (size_t) m_ * k_, space, st_));
    else if (plan_.warm_start()) MFX_HIP(hipMemsetAsync(W_.get(), 0, sizeof(float) * (size_t) m_ * k_, st_));  // W is the warm start of the first W-half
    w_cold_ = !W;
    MFX_TRY(H_.upload(H, (size_t) n_ * k_, space, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    factors_set_ = true;
    return MFX_OK;
}

int AlsSolver::half_sweep(int half) {
    const bool cg = plan_.method == PM::Cg;
    const AlsHalf& h = half ? cols_ : rows_;
    const float* X = half ? W_.get() : H_.get();
    float* Y = half ? H_.get() + (size_t) col_lo_ * k_ : W_.get() + (size_t) row_lo_ * k_;
    const float* rho = half ? plan_.rho_cols.get() : plan_.rho_rows.get();
    // the W-half is the only one that may be cold (W is then zero); ev_[4 + half]: the base Gramian of the fixed side is done,
    // ev_[6 + half]: its inverse
    MFX_TRY(als_plan_half(plan_, h, X, half ? m_ : n_, Y, half == 1 || !w_cold_, rho, ev_[4 + half], ev_[6 + half],
                          cg ? plan_.cg_fail.get() + 2 * half : spd_fail_.get(), cg ? plan_.cg_cnt.get() + 3 * half : nullptr, st_, phases_.get()));
    if (half == 0) w_cold_ = false;
    return MFX_OK;
}

int AlsSolver::iterate(int n_iter, int with_rmse, mfx_iter_report* reports) {
    MFX_REQUIRE(n_iter >= 0, "n_iter must be >= 0");
    MFX_REQUIRE(factors_set_, "mfx_als_iterate: call mfx_als_set_factors first");
    MFX_TRY(use_device(device_));
    if (comm_ && !shards_met_ && n_iter > 0) MFX_TRY(meet_shards());
    const bool cg = plan_.method == PM::Cg;
    for (int it = 0; it < n_iter; ++it) {
        MFX_HIP(hipMemsetAsync(spd_fail_.get(), 0, sizeof(uint32_t), st_));
        if (cg) MFX_HIP(hipMemsetAsync(plan_.cg_fail.get(), 0, sizeof(uint32_t) * 4, st_));
        MFX_HIP(hipEventRecord(ev_[0], st_));
        MFX_TRY(half_sweep(0));
        if (comm_) MFX_TRY(exchange(W_.get(), row_bounds_));
        MFX_HIP(hipEventRecord(ev_[1], st_));
        if (phases_.size()) MFX_TRY(print_phases("user half (W over H)"));
        MFX_TRY(half_sweep(1));
        if (comm_) MFX_TRY(exchange(H_.get(), col_bounds_));
        MFX_HIP(hipEventRecord(ev_[2], st_));
        if (phases_.size()) MFX_TRY(print_phases("item half (H over W)"));
        double rmse = 0.0, sum = 0.0;
        if (with_rmse && global_test_nnz_ > 0) {
            if (nnz_test_ > 0)
                MFX_TRY(launch_test_sqerr(nnz_test_, t_row_.get(), t_col_.get(), t_val_.get(), W_.get(), H_.get(), m_, n_,
                                          k_, 1, rmse_partials_.get(), kRmseBlocks, rmse_sum_.get(), st_));
            else
                MFX_HIP(hipMemsetAsync(rmse_sum_.get(), 0, sizeof(double), st_));
            if (comm_) MFX_TRY(comm_allreduce_f64(comm_, rmse_sum_.get(), 1, st_));
            MFX_HIP(hipMemcpyAsync(&sum, rmse_sum_.get(), sizeof(double), hipMemcpyDeviceToHost, st_));
        }
        MFX_HIP(hipEventRecord(ev_[3], st_));
        uint32_t bad = 0;
        MFX_HIP(hipMemcpyAsync(&bad, spd_fail_.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
        uint32_t cg_bad[4] = {0, 0, 0, 0};
        unsigned long long cg_cnt[6] = {0, 0, 0, 0, 0, 0};
        if (cg) {
            MFX_HIP(hipMemcpyAsync(cg_bad, plan_.cg_fail.get(), sizeof(cg_bad), hipMemcpyDeviceToHost, st_));
            MFX_HIP(hipMemcpyAsync(cg_cnt, plan_.cg_cnt.get(), sizeof(cg_cnt), hipMemcpyDeviceToHost, st_));
        }
        MFX_HIP(hipStreamSynchronize(st_));
        if (cg) {  // a failed inverse or failed rows: reported as the failed systems of the other solvers are
            for (int hf = 0; hf < 2; ++hf) {
                for (int q = 0; q < 3; ++q) cg_stats_[4 * hf + q] = (int64_t) cg_cnt[3 * hf + q];
                cg_stats_[4 * hf + 3] = (int64_t) cg_bad[2 * hf + 1];
            }
            cg_stats_set_ = true;
            bad = cg_bad[0] + cg_bad[1] + cg_bad[2] + cg_bad[3];
        }
        if (with_rmse && global_test_nnz_ > 0) rmse = std::sqrt(sum / (double) global_test_nnz_);
        float ms_w = 0.f, ms_h = 0.f, ms_r = 0.f, ms_gh = 0.f, ms_gw = 0.f, ms_ih = 0.f, ms_iw = 0.f;
        // either half: the base Gramian of the fixed side and its inverse, where the plan has them, then the solve
        hipEvent_t from_w = ev_[0], from_h = ev_[1];
        if (plan_.has_base_gramian()) {
            MFX_HIP(hipEventElapsedTime(&ms_gh, from_w, ev_[4]));
            MFX_HIP(hipEventElapsedTime(&ms_gw, from_h, ev_[5]));
            from_w = ev_[4]; from_h = ev_[5];
            t_half_[2] += ms_gh * 1e-3; t_half_[3] += ms_gw * 1e-3; n_half_[2]++; n_half_[3]++;
        }
        if (plan_.has_inverse()) {
            MFX_HIP(hipEventElapsedTime(&ms_ih, from_w, ev_[6]));
            MFX_HIP(hipEventElapsedTime(&ms_iw, from_h, ev_[7]));
            from_w = ev_[6]; from_h = ev_[7];
            t_half_[4] += ms_ih * 1e-3; t_half_[5] += ms_iw * 1e-3; n_half_[4]++; n_half_[5]++;
        }
        MFX_HIP(hipEventElapsedTime(&ms_w, from_w, ev_[1]));
        MFX_HIP(hipEventElapsedTime(&ms_h, from_h, ev_[2]));
        MFX_HIP(hipEventElapsedTime(&ms_r, ev_[2], ev_[3]));
        t_half_[0] += ms_w * 1e-3; t_half_[1] += ms_h * 1e-3; n_half_[0]++; n_half_[1]++;
        mfx_iter_report rep;
        rep.rank_time = 0.0;
        rep.update_time = (ms_gh + ms_ih + ms_w + ms_gw + ms_iw + ms_h) * 1e-3;
        rep.rmse = rmse;
        rep.rmse_time = ms_r * 1e-3;
        update_acc_ += rep.update_time;
        ++iter_;
        if (reports) reports[it] = rep;
        // the reference prints this from inside the kernel for every failing pivot (ALS_CUDA.cu:11-13)
        if (bad && p_.verbose && (!comm_ || comm_->rank == 0)) printf(" a is not positive definite! (%u systems or pivots)\n", bad);
        if (p_.verbose && (!comm_ || comm_->rank == 0)) {
            // log line format of cuda_src/ALS_CUDA.cu:360-361
            printf("[-INFO-] iteration num %d \tupdate_time %.4lf|%.4lfs \tRMSE=%lf time:%fs\n", (int) iter_,
                   rep.update_time, update_acc_, rep.rmse, rep.rmse_time);
            fflush(stdout);
        }
    }
    return MFX_OK;
}

int AlsSolver::get_factors(float* W, float* H, mfx_memspace space) {
    MFX_TRY(use_device(device_));
    const hipMemcpyKind kind = space == MFX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (W) MFX_HIP(hipMemcpyAsync(W, W_.get(), sizeof(float) * (size_t) m_ * k_, kind, st_));
    if (H) MFX_HIP(hipMemcpyAsync(H, H_.get(), sizeof(float) * (size_t) n_ * k_, kind, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

int AlsSolver::kernel_times(int cap, const char** names, double* seconds, int64_t* launches) {
    int n = 0;
    for (int i = 0; i < 6 && n < cap; ++i) {
        if (!n_half_[i]) continue;
        if (names) names[n] = plan_.pair->names[i];
        if (seconds) seconds[n] = t_half_[i];
        if (launches) launches[n] = n_half_[i];
        ++n;
    }
    for (int i = 0; i < 6; ++i) { t_half_[i] = 0; n_half_[i] = 0; }
    return n;
}

int AlsSolver::cg_stats(int64_t out[8]) {
    MFX_REQUIRE(plan_.method == PM::Cg, "mfx_ials_cg_stats: not a handle of mfx_ials_cg_create");
    MFX_REQUIRE(out, "mfx_ials_cg_stats: out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = cg_stats_set_ ? cg_stats_[i] : 0;
    return MFX_OK;
}

int AlsSolver::loss(double* out) {
    MFX_REQUIRE(plan_.implicit(), "mfx_ials_loss: not an implicit-feedback ALS handle (mfx_ials_create)");
    MFX_REQUIRE(factors_set_, "mfx_ials_loss: call mfx_als_set_factors first");
    MFX_TRY(use_device(device_));
    AlsPlan& pl = plan_;
    if (!pl.loss_ws.size()) MFX_TRY(pl.loss_ws.alloc(pl.loss_ws_doubles()));
    if (pl.objective == PO::ImplicitReg)
        MFX_TRY(ialsr_loss_launch(rows_, W_.get(), m_, H_.get(), n_, k_, pl.lambda, pl.alpha, pl.alpha0, pl.nu, pl.rho_rows.get(), pl.rho_cols.get(),
                                  pl.loss_ws.get(), loss_.get(), st_));
    else
        MFX_TRY(ials_loss_launch(rows_, W_.get(), m_, H_.get(), n_, k_, pl.lambda, pl.alpha, pl.loss_ws.get(), loss_.get(), st_));
    MFX_HIP(hipMemcpyAsync(out, loss_.get(), sizeof(double), hipMemcpyDeviceToHost, st_));
    MFX_HIP(hipStreamSynchronize(st_));
    return MFX_OK;
}

// ------------------------------------------------------------------------------------------------
int HalfOp::open(int device, int64_t nseg, int64_t nnz, int64_t nrows_x, const uint32_t* ptr, const uint32_t* idx, const float* val) {
    MFX_TRY(use_device(device));
    MFX_HIP(hipStreamCreateWithFlags(&os.st, hipStreamNonBlocking));
    return h.build((uint32_t) nseg, (uint64_t) nnz, (uint32_t) nrows_x, ptr, idx, val, MFX_HOST, kAlsChunk, os.st);
}

int HalfOp::upload(const float* X_in, int64_t nrows_x, int64_t k, bool zero_row, const float* Y_in) {
    if (zero_row) MFX_TRY(X.alloc_zero(((size_t) nrows_x + 1) * k, os.st));
    else MFX_TRY(X.alloc((size_t) nrows_x * k));
    MFX_TRY(X.upload(X_in, (size_t) nrows_x * k, MFX_HOST, os.st));
    MFX_TRY(Y.alloc_zero((size_t) h.nseg * k, os.st));
    if (Y_in) MFX_TRY(Y.upload(Y_in, (size_t) h.nseg * k, MFX_HOST, os.st));
    return fail_cnt.alloc_zero(1, os.st);
}

int HalfOp::download(float* Y_out) {
    MFX_HIP(hipMemcpyAsync(Y_out, Y.get(), sizeof(float) * Y.size(), hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipStreamSynchronize(os.st));
    return MFX_OK;
}

int als_gramian_op(int64_t cnt, const uint32_t* idx, int64_t nrows_x, const float* X, int64_t k, float* A, int device) {
    MFX_REQUIRE(k <= 128, "ALS: rank k = %lld not supported (1 <= k <= 128)", (long long) k);
    MFX_TRY(use_device(device));
    if (cnt == 0) { memset(A, 0, sizeof(float) * k * k); return MFX_OK; }
    MFX_REQUIRE(cnt <= kAlsChunk, "mfx_als_gramian: at most %u gathered rows per call", kAlsChunk);
    OpStream os;
    MFX_HIP(hipStreamCreateWithFlags(&os.st, hipStreamNonBlocking));
    DevBuf<uint32_t> didx, fail_cnt; DevBuf<float> dval, dX, dY, dA; DevBuf<AlsItem> ditem;
    const uint32_t zrow = (uint32_t) nrows_x;
    MFX_TRY(didx.alloc_zero(cnt + kAlsEntryPad, os.st)); MFX_TRY(didx.upload(idx, cnt, MFX_HOST, os.st));
    MFX_HIP(hipMemcpyAsync(didx.get() + cnt, &zrow, sizeof(uint32_t), hipMemcpyHostToDevice, os.st));
    MFX_TRY(check_index_range(didx.get(), (uint64_t) cnt, (uint32_t) nrows_x, "ALS gather index", os.st));
    MFX_TRY(dval.alloc_zero(cnt + kAlsEntryPad, os.st));
    MFX_TRY(dX.alloc_zero(((size_t) nrows_x + 1) * k, os.st)); MFX_TRY(dX.upload(X, (size_t) nrows_x * k, MFX_HOST, os.st));
    MFX_TRY(dY.alloc_zero(k, os.st)); MFX_TRY(dA.alloc_zero((size_t) k * k, os.st));
    MFX_TRY(fail_cnt.alloc_zero(1, os.st));
    AlsItem it{0, 0, (uint32_t) cnt, -1};
    MFX_TRY(ditem.alloc(1)); MFX_TRY(ditem.upload(&it, 1, MFX_HOST, os.st));
    MFX_TRY(als_gramian_launch(ditem.get(), didx.get(), dval.get(), (uint32_t) cnt, dX.get(), (uint32_t) nrows_x, dY.get(), (uint32_t) k,
                               fail_cnt.get(), dA.get(), os.st));
    MFX_HIP(hipMemcpyAsync(A, dA.get(), sizeof(float) * k * k, hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipStreamSynchronize(os.st));
    return MFX_OK;
}

int als_plan_half_op(const AlsSpec& spec, const HalfSegs& g, const float* X, const float* Y_in, float* Y_out, int64_t k, float lambda,
                     int32_t* counts, int device) {
    HalfOp op;
    AlsPlan pl;
    MFX_TRY(pl.set(spec, (uint32_t) k, lambda));
    MFX_TRY(op.open(device, g.nseg, g.nnz, g.nrows_x, g.ptr, g.idx, g.val));
    MFX_TRY(pl.check_values(op.h, (std::string(spec.fn) + ": value").c_str(), op.os.st));
    MFX_TRY(pl.alloc((uint32_t) g.nrows_x, op.h.nseg, op.h.nnz, op.h.nslots, op.os.st));
    MFX_TRY(op.upload(X, g.nrows_x, k, pl.method != PM::Blocks, Y_in));  // (the block sweeps gather the zero row from their packed copy)
    if (pl.objective == PO::ImplicitReg) {
        MFX_TRY(pl.rho_rows.alloc(op.h.nseg));
        MFX_TRY(ialsr_rho_launch(op.h, (uint32_t) g.nrows_x, lambda, pl.alpha0, pl.nu, pl.rho_rows.get(), op.os.st));
    }
    const bool cg = pl.method == PM::Cg;
    MFX_TRY(als_plan_half(pl, op.h, op.X.get(), (uint32_t) g.nrows_x, op.Y.get(), Y_in != nullptr, pl.rho_rows.get(), nullptr, nullptr,
                          cg ? pl.cg_fail.get() : op.fail_cnt.get(), pl.cg_cnt.get(), op.os.st));
    uint32_t bad_pivots = 0;
    if (cg) {
        MFX_HIP(hipMemcpyAsync(&bad_pivots, pl.cg_fail.get(), sizeof(bad_pivots), hipMemcpyDeviceToHost, op.os.st));
        if (counts) MFX_HIP(hipMemcpyAsync(counts, pl.cgs.counts.get(), sizeof(int32_t) * (size_t) g.nseg, hipMemcpyDeviceToHost, op.os.st));
    }
    MFX_TRY(op.download(Y_out));
    MFX_REQUIRE(bad_pivots == 0, "%s: X^T X + lambda I is not positive definite (%u pivots <= 0 or not finite): X must be finite and "
                "lambda > 0 unless X has full rank", spec.fn, bad_pivots);
    return MFX_OK;
}

}  // namespace mfx
