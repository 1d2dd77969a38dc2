// recommend.hpp -- resident top-N recommender (mfx_rec_*) and the host-side ranking metrics (mfx_topn_metrics).
//
// The query is one fused pass per (user block, item slice): scores come out of v_mfma_f32_32x32x2_f32 tiles (H staged
// in LDS and shared by the 128 users of a workgroup, W in registers), a running per-user threshold keeps the
// per-score work to one compare, and only the scores that pass reach a per-user candidate list in the workspace;
// nothing of the users x items score matrix is ever stored.  See recommend.hip; the pass over the tiles of H, which the
// rank count of rec_rank.hip runs too, is in rec_tiles.hpp.
#pragma once

#include "als_solver.hpp"  // IalsBlock (fold-in by block sweeps), FoldCg
#include "common.hpp"

namespace mfx {

// What a fold-in setup leaves in the handle: how the query rows are solved, on which objective, with which parameters, and
// the device state built for that.  The two axes are independent; fold_setup builds the combinations that exist.  A setup
// builds a fresh plan, so a field it does not set holds its default, never what an earlier setup left.
struct FoldPlan {
    // Direct: one closed-form solve per row at k <= 128 by the MFMA half-sweep families; DirectExact: MFX_FOLD_ALS_EXACT, the
    // same system in the reference's order of operations; Blocks: block subspace sweeps; Cg: conjugate gradients
    enum class Method { None, Direct, DirectExact, Blocks, Cg };
    // what goes on the diagonal: Als lambda, Ccd fp32(lambda * entries of the row), Implicit the base Gramian's lambda,
    // ImplicitReg fp32(lambda (n + alpha0 cols)^nu) per query row, with alpha0 the weight of the unobserved pairs
    enum class Objective { Als, Ccd, Implicit, ImplicitReg };
    Method method = Method::None;
    Objective objective = Objective::Als;
    float lambda = 0.f, alpha = 0.f, alpha0 = 1.f, nu = 0.f;  // alpha: 0 on an explicit objective
    int32_t cap = 0;  // the most sweeps (Blocks) or steps (Cg) a row gets
    float tol = 0.f;
    // Direct: the base Gramian [k][k] (Implicit: H^T H + lambda I; ImplicitReg: fp32(alpha0 H^T H)); Cg / Implicit:
    // G = H^T H + lambda I and minv ~ G^-1
    DevBuf<float> g, minv;
    // Blocks: H block-major, and on the implicit objectives G (as above) with its diagonal blocks; P, Z, the scores and the
    // split-segment slots live for one query
    IalsBlock b;

    bool implicit() const { return objective == Objective::Implicit || objective == Objective::ImplicitReg; }
    // takes W_init and reports sweeps_done (mfx_rec_fold_in_warm); needs no als_ws_floats workspace
    bool iterative() const { return method == Method::Blocks || method == Method::Cg; }
    // closed-form, and the factor is the MFMA system's: what mfx_rec_explain splits
    bool explains() const { return method == Method::Direct; }
    FoldCg cg() const {  // Cg only
        FoldCg m;
        m.reg = implicit() ? 0 : objective == Objective::Als ? 1 : 2;
        m.lambda = lambda; m.alpha = alpha;
        m.G = g.get(); m.Minv = minv.get();
        m.steps = cap; m.tol = tol;
        return m;
    }
};

// What a setup entry point asks for.  arg is its model (Direct, DirectExact, Cg) or reg (Blocks on an explicit objective)
// argument as the caller gave it, which fold_setup checks in the entry point's own place; method and objective are what a
// valid one selects.
struct FoldSpec {
    FoldPlan::Method method;
    FoldPlan::Objective objective;
    int arg = 0;
    float lambda = 0.f, alpha = 0.f, alpha0 = 1.f, nu = 0.f;
    int32_t block = 0, cap = 0;  // block: the requested width (Blocks), 0 = chosen from k; cap: sweeps or steps
    float tol = 0.f;
    // for an entry point that takes a model: Direct or Cg as asked (DirectExact for MFX_FOLD_ALS_EXACT) and the model's
    // objective; fold_setup refuses by arg a model that is unknown or not for the method, so what those map to is never used
    static FoldSpec of_model(FoldPlan::Method method, int model, float lambda, float alpha) {
        using O = FoldPlan::Objective;
        FoldSpec s{method == FoldPlan::Method::Direct && model == MFX_FOLD_ALS_EXACT ? FoldPlan::Method::DirectExact : method,
                   model == MFX_FOLD_IMPLICIT ? O::Implicit : model == MFX_FOLD_CCD ? O::Ccd : O::Als, model};
        s.lambda = lambda; s.alpha = alpha;
        return s;
    }
};

// What mfx_rec_ivf_setup leaves in the handle (rec_ivf.hip): the items in list order.  Every list starts on a tile and is
// padded to whole tiles, so no tile of hp holds items of two lists.
struct IvfIndex {
    int32_t nlist = 0;       // 0: not set up
    int nblk = 0;            // tiles of hp: sum over the lists of ceil(size / 32)
    int nblkc = 0;           // tiles of cp: ceil(nlist / 32)
    DevBuf<float> hp;        // [nblk][nch][2*KC][32]: H in list order, the bits of the handle's own tiles
    DevBuf<float> cp;        // [nblkc][nch][2*KC][32]: the centroids packed like H
    DevBuf<float> fac;       // [nblk * 32]: the item filter's 1 / NaN in list order (empty without a filter)
    DevBuf<uint32_t> ids;    // [nblk * 32]: position -> item id, 0xFFFFFFFF at the padding
    DevBuf<uint32_t> blk_ptr;   // [nlist + 1]: first tile of every list
    DevBuf<uint32_t> list_ptr;  // [nlist + 1], list_idx [cols]: the lists as mfx_rec_ivf_lists returns them
    DevBuf<uint32_t> list_idx;
};

// The candidate lists of a batch on the device, as the checks of rec_candidates.hip leave them (mfx_rec_query_candidates,
// mfx_rec_diversify).
struct CandLists {
    DevBuf<uint32_t> d_ptr, d_idx;  // the copies, when the caller's arrays live on the host
    DevBuf<uint32_t> long_list;     // [nu], the first nlong filled: the slots whose list is longer than 2048, in any order
    const uint32_t* ptr = nullptr;  // [nu + 1], on the device
    const uint32_t* idx = nullptr;  // NULL when the caller passed none
    int idx_grid = 0;               // workgroups of the check of the ids
    uint32_t total = 0, nlong = 0;  // after cand_check: ptr[nu] and the number of long lists
};

class Recommender {
public:
    static int create(Recommender** out, const float* W, const float* H, int64_t rows, int64_t cols, int64_t k,
                      int layout, const mfx_csx* exclude, mfx_memspace space, int device);
    int query(int64_t nusers, const uint32_t* users, int32_t n_top, uint32_t* items, float* scores,
              mfx_memspace space, int item_slices);
    // fold-in: the one setup behind the seven mfx_rec_fold_in_*setup* entry points (fn: the entry point, for its refusals),
    // then mfx_rec_fold_in: solve query rows against H and score them
    int fold_setup(const char* fn, const FoldSpec& s);
    int fold_in(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, float* W_out,
                int32_t n_top, uint32_t* items, float* scores, mfx_memspace space);
    // mfx_rec_fold_in_warm: after a block or cg setup only; W_init [nusers][k] / sweeps_done [nusers] in `space`, or NULL
    int fold_in_warm(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, const float* W_init,
                     float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space);
    // mfx_rec_set_item_filter / mfx_rec_similar_setup / mfx_rec_item_norms / mfx_rec_similar
    int set_item_filter(const uint8_t* keep, mfx_memspace space);
    int similar_setup();
    int item_norms(float* n2, float* c, mfx_memspace space);
    int similar(int64_t nq, const uint32_t* query_items, int metric, int exclude_self, int32_t n_top, uint32_t* items, float* scores,
                mfx_memspace space, int item_slices);
    void fold_in_times(double out[3]) const { for (int i = 0; i < 3; ++i) out[i] = fold_s_[i]; }
    // mfx_rec_rank / mfx_rec_evaluate / mfx_rec_rank_times (rec_rank.hip)
    int rank(int64_t npairs, const uint32_t* users, const uint32_t* items, uint32_t* ranks, float* scores, uint32_t* n_eligible,
             mfx_memspace space, int item_slices);
    int evaluate(const mfx_coo* T, float min_rating, int32_t n_cut, const int32_t* cutoffs, double* out, double* mrr, double* auc,
                 int64_t* users_evaluated, int64_t* auc_users, mfx_memspace space);
    void rank_times(double out[3]) const { for (int i = 0; i < 3; ++i) out[i] = rank_s_[i]; }
    // mfx_rec_query_candidates / mfx_rec_score / mfx_rec_candidates_times (rec_candidates.hip)
    int query_candidates(int64_t nusers, const uint32_t* users, const uint32_t* cand_ptr, const uint32_t* cand_idx, int32_t flags,
                         int32_t n_top, uint32_t* items, float* scores, uint32_t* n_eligible, mfx_memspace space);
    int score(int64_t npairs, const uint32_t* users, const uint32_t* items, float* scores, mfx_memspace space);
    void candidates_times(double out[3]) const { for (int i = 0; i < 3; ++i) out[i] = cand_s_[i]; }
    // mfx_rec_diversify / mfx_rec_diversify_times (rec_diversify.hip)
    int diversify(int64_t nusers, const uint32_t* users, const float* Wq, const uint32_t* cand_ptr, const uint32_t* cand_idx, int32_t flags,
                  int metric, float tradeoff, int32_t n_top, uint32_t* items, float* scores, float* values, uint32_t* n_eligible,
                  mfx_memspace space, int form);
    void diversify_times(double out[3]) const { for (int i = 0; i < 3; ++i) out[i] = div_s_[i]; }
    // mfx_rec_ivf_setup / mfx_rec_ivf_lists / mfx_rec_ivf_probe / mfx_rec_query_ivf / mfx_rec_ivf_times (rec_ivf.hip)
    int ivf_setup(int32_t nlist, const uint32_t* assign, const float* centroids, mfx_memspace space);
    int ivf_lists(uint32_t* list_ptr, uint32_t* list_idx, mfx_memspace space);
    int ivf_probe(int64_t nusers, const uint32_t* users, int32_t nprobe, uint32_t* lists, float* scores, mfx_memspace space);
    int query_ivf(int64_t nusers, const uint32_t* users, int32_t nprobe, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space);
    void ivf_times(double out[4]) const { for (int i = 0; i < 4; ++i) out[i] = ivf_s_[i]; }
    // mfx_rec_explain / mfx_rec_explain_times (recommend.hip; the lists: rec_candidates.hip)
    static constexpr int kMaxExplain = 64;
    int explain(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out, float* Z_out,
                mfx_memspace space);
    // mfx_rec_explain_cg: after mfx_rec_fold_in_cg_setup only; Z by conjugate gradients over the pairs (rec_explain_cg.hip)
    int explain_cg(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                   const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out, float* Z_out,
                   int32_t* row_steps, int32_t* target_steps, mfx_memspace space);
    void explain_times(double out[3]) const { for (int i = 0; i < 3; ++i) out[i] = expl_s_[i]; }
    ~Recommender();

private:
    // The top-N pass over nu batch slots: slot q scores packed row users[q] (q when users is NULL) of wp [.][kt_] and
    // excludes the items of row users[q] (q) of ex_ptr / ex_idx (ex_ptr NULL: none).  Device pointers except items /
    // scores, which live in `space`.  fac (NULL: none) [nblk_ * 32]: the ranking key of an item is fp32(score * fac[item]);
    // qfac (NULL: none, needs fac) [query id]: a slot's returned scores are fp32(key * qfac[users[q]]), the order the keys'.
    // tiles (NULL: the handle's own H): another packed item side of the same k, e.g. the centroids of the ivf index; then
    // item_slices is taken as given (pick_slices knows the handle's tiles only).
    struct TileSet {
        const float* hp;
        uint32_t cols;
        int nblk;
    };
    int topn(const float* wp, uint32_t nu, const uint32_t* users, const uint32_t* ex_ptr, const uint32_t* ex_idx,
             int32_t n_top, uint32_t* items, float* scores, mfx_memspace space, int item_slices, const float* fac,
             const float* qfac, const TileSet* tiles = nullptr);
    // mfx_rec_merge of recommend.hip over the partial lists ls / li [slices][nq][L] of batch slots q0 .. q0 + nq
    int merge_launch(const float* ls, const uint32_t* li, uint32_t q0, uint32_t nq, int slices, int L, int n_top, uint32_t* out_items,
                     float* out_scores);
    // mfx_rec_pack_h of recommend.hip: H [cols][k] (layout 1) or [k][cols] (layout 0) on the device into tiles hp
    int pack_h_launch(const float* H, int layout, uint32_t cols, int nblk, float* hp);
    // the ivf index's copy of the item filter's factor, after the filter or the index changed (rec_ivf.hip)
    int ivf_refresh_fac();
    int ivf_probe_dev(uint32_t nu, const uint32_t* du, int32_t nprobe, uint32_t* lists, float* scores, mfx_memspace space);
    // The ids of a batch [n] from `space` onto the device (buf holds the copy) with every id < bound checked; *dev is where
    // they are, NULL for ids = NULL.  `what` opens the refusal ("mfx_rec_query: user id").
    int stage_ids(const uint32_t* ids, uint32_t n, mfx_memspace space, uint32_t bound, const char* what, DevBuf<uint32_t>& buf,
                  const uint32_t** dev);
    // The candidate lists of nu slots (rec_candidates.hip).  cand_stage: onto the device when they live on the host (l.ptr /
    // l.idx are where they are then).  cand_check: the device-side checks of mfx_rec_query_candidates and their one host round
    // trip (it synchronises the stream): MFX_ERR_INVALID naming the first offending slot, else l.total, l.nlong and
    // l.long_list.  `fn` opens the refusals.
    int cand_stage(const char* fn, uint32_t nu, const uint32_t* cand_ptr, const uint32_t* cand_idx, mfx_memspace space, CandLists& l);
    int cand_check(const char* fn, uint32_t nu, CandLists& l);
    // Item slices (grid.y) of a tile pass over `blocks` workgroups of slots: `forced`, or for 0 enough for about two workgroups
    // per CU; at most cap, and none empty.  rank() passes its item_slices; topn() calls this for item_slices = 0 only and
    // takes a forced count as given (empty slices included: they merge as padding), as it always did.
    int pick_slices(int forced, int64_t blocks, int cap) const;
    // fac_keep_ (when keep is set) and fac_cos_ (after similar_setup) from the device filter bytes keep (NULL: no filter)
    int build_facs(const uint8_t* keep);
    // hq_ from the tiles unless it is there already (similar_setup builds it too): the rows of H that rank() gathers
    int ensure_hq();
    // the regulariser of every query row of h from its own entries into rho [h.nseg], under ImplicitReg (else rho stays empty)
    int fold_rho(const AlsHalf& h, DevBuf<float>& rho);
    int fold_rows(const char* fn, uint32_t nu, uint64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, mfx_memspace space,
                  AlsHalf& h);
    int explain_run(const char* fn, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                    const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out,
                    float* Z_out, int32_t* row_steps, int32_t* target_steps, mfx_memspace space);
    int explain_check_targets(const char* fn, const uint32_t* d_targets, size_t n, int32_t n_targets);
    int explain_lists(const AlsHalf& h, const uint32_t* d_targets, int32_t nt, const float* Z, const float* Y, int32_t n_expl,
                      uint32_t* d_items, float* d_contrib, float* d_totals);
    int fold_solve(int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, const float* W_init,
                   float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space);
    int device_ = 0;
    hipStream_t st_ = nullptr;
    int64_t rows_ = 0, cols_ = 0, k_ = 0;
    int kc_ = 0;       // MFMA steps (of two t values) per LDS stage: 1, 2, 4, ..., 64
    int nch_ = 0;      // t chunks of 2 * kc_ (k > 128 takes several)
    int kt_ = 0;       // padded k = nch_ * 2 * kc_
    int nblk_ = 0;     // 32-item tiles
    int cus_ = 256;    // compute units of the device (automatic slicing)
    DevBuf<float> wp_, hp_;
    DevBuf<uint32_t> ex_ptr_, ex_idx_;
    bool has_ex_ = false;
    // item filter (set_item_filter): the bytes, and 1 / NaN per item [nblk_ * 32] (null without a filter)
    DevBuf<uint8_t> keep_;
    DevBuf<float> fac_keep_;
    // item-to-item (similar_setup): H as a query operand [cols_][kt_], squared norms and inverse norms [cols_], 0 .. cols_
    // (row pointers and indices of the identity exclusion), inverse norms with NaN at the filtered items [nblk_ * 32]
    DevBuf<float> hq_, sim_n2_, sim_c_, fac_cos_;
    DevBuf<uint32_t> sim_id_;
    // fold-in: H row-major [cols_ + 1][k_] with a zero last row (built by the first setup, the same for every plan), and what
    // the last setup that went through left (method None: not set up)
    DevBuf<float> hx_;
    FoldPlan plan_;
    double fold_s_[3] = {0, 0, 0};  // host build / solve / score seconds of the last fold-in
    double rank_s_[3] = {0, 0, 0};  // device seconds of the last rank: target keys / counting pass / exclusion correction
    double expl_s_[3] = {0, 0, 0};  // seconds of the last explain of either kind: host build + checks / solve / totals + contributions
    IvfIndex ivf_;
    double ivf_s_[4] = {0, 0, 0, 0};  // stream seconds of the last query_ivf: probe / work-item build / list pass / merge
    double cand_s_[3] = {0, 0, 0};  // stream seconds of the last query_candidates / score: check + stage / score / merge of long lists
    double div_s_[3] = {0, 0, 0};   // stream seconds of the last diversify: check + stage / relevance / selection
};

// The sums behind {HR, precision, recall, NDCG} at one cutoff, shared by mfx_topn_metrics (positions read off a list) and
// mfx_rec_evaluate (positions are ranks).  add(): one kept user, the 0-based positions below n_top of its distinct hits in
// ascending order, and |R_u|.
struct TopnAcc {
    double hr = 0, prec = 0, rec = 0, ndcg = 0;
    int64_t kept = 0;
    void add(const uint32_t* pos, size_t nhits, size_t nrel, int64_t n_top);
    void mean(double out[4]) const;
};

int topn_metrics(int64_t nusers, const uint32_t* users, int32_t n_top, const uint32_t* items, const mfx_coo* T,
                 float min_rating, double out[4], int64_t* users_evaluated);

}  // namespace mfx

struct mfx_rec_s {
    mfx::Recommender* impl;
};
