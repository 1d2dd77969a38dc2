// api.hip -- the extern "C" surface declared in include/mfx.h.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <stdexcept>

#include "als_solver.hpp"
#include "bpr.hpp"
#include "ccd_solver.hpp"
#include "knn.hpp"
#include "hybrid.hpp"
#include "lgcn.hpp"
#include "recommend.hpp"
#include "slim.hpp"
#include "ease.hpp"

namespace mfx {

std::string& last_error() {
    static thread_local std::string e;
    return e;
}

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(MFX_ERR_NO_DEVICE, "no usable HIP device (%s); libmfx has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= n) return fail(MFX_ERR_NO_DEVICE, "device %d out of range (have %d)", device, n);
    MFX_HIP(hipSetDevice(device));
    // hipGetLastError() is a sticky per-thread slot shared with every other HIP user of the process
    // (RCCL under torch.distributed leaves "invalid device ordinal" there while probing peers).  Every
    // libmfx launch reads the slot right after itself, so whatever sits in it on ENTRY to a libmfx call
    // is somebody else's: drop it here, once per call -- never between our own launches.
    (void) hipGetLastError();
    return MFX_OK;
}

}  // namespace mfx

using namespace mfx;

// No C++ exception may cross the C ABI (std::bad_alloc from a multi-GB host vector, std::system_error
// from a thread that could not be started, ...): every entry point that does work runs inside this.
template <typename F>
static int guarded(const char* what, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(MFX_ERR_ALLOC, "%s: out of host memory", what);
    } catch (const std::exception& ex) {
        return fail(MFX_ERR_INVALID, "%s: %s", what, ex.what());
    } catch (...) {
        return fail(MFX_ERR_INVALID, "%s: unknown C++ exception", what);
    }
}

// A create entry point: `out` checked under the entry point's own name and cleared, the object made by `make`, the handle
// S around it; and the end of a handle.
template <class S, class Make>
static int make_handle(const char* fn, S** out, Make&& make) {
    MFX_REQUIRE(out, "%s: out is NULL", fn);
    *out = nullptr;
    decltype(S::impl) impl = nullptr;
    MFX_TRY(make(&impl));
    *out = new S{impl};
    return MFX_OK;
}
template <class S>
static int destroy_handle(S* h) {
    if (!h) return MFX_OK;
    delete h->impl;
    delete h;
    return MFX_OK;
}

extern "C" {

const char* mfx_last_error(void) { return last_error().c_str(); }
int mfx_version(void) { return MFX_VERSION; }

int mfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mfx_params_default(mfx_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->k = 10;            /* src/pmf.h:28 */
    p->lambda = 0.1f;     /* src/pmf.h:32 */
    p->maxiter = 5;       /* src/pmf.h:30 */
    p->maxinneriter = 1;  /* src/pmf.h:31 */
    p->nBlocks = 32;      /* src/pmf.h:39 */
    p->nThreadsPerBlock = 256;
    p->schedule = 1;
    p->kernel_variant = 1;
}

/* ------------------------------------------------------------------ resident CCD++ */
int mfx_ccd_create(mfx_ccd_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p,
                   mfx_memspace space, const mfx_shard* shard) {
    return guarded("mfx_ccd_create", [&]() -> int {
        return make_handle("mfx_ccd_create", out, [&](CcdSolver** s) { return CcdSolver::create(s, R, T, p, space, shard); });
    });
}
int mfx_ccd_set_factors(mfx_ccd_t s, const float* W, const float* H, mfx_memspace space) {
    return guarded("mfx_ccd_set_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_factors(W, H, space);
    });
}
int mfx_ccd_iterate(mfx_ccd_t s, int n_outer, int with_rmse, mfx_iter_report* reports) {
    return guarded("mfx_ccd_iterate", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->iterate(n_outer, with_rmse, reports);
    });
}
int mfx_ccd_get_factors(mfx_ccd_t s, float* W, float* H, mfx_memspace space) {
    return guarded("mfx_ccd_get_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_factors(W, H, space);
    });
}
int mfx_ccd_get_residual(mfx_ccd_t s, float* csc_val, float* csr_val) {
    return guarded("mfx_ccd_get_residual", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_residual(csc_val, csr_val);
    });
}
int mfx_ccd_kernel_times(mfx_ccd_t s, int cap, const char** names, double* seconds, int64_t* launches) {
    return guarded("mfx_ccd_kernel_times", [&]() -> int {
        if (!s || !s->impl) return 0;
        KernelProfiler& pr = s->impl->profiler();
        int n = 0;
        for (int i = 0; i < KernelProfiler::K_COUNT && n < cap; ++i) {
            if (pr.launches[i] == 0) continue;
            if (names) names[n] = KernelProfiler::name(i);
            if (seconds) seconds[n] = pr.seconds[i];
            if (launches) launches[n] = pr.launches[i];
            ++n;
        }
        pr.reset_totals();
        return n;
    });
}
int mfx_ccd_set_profile(mfx_ccd_t s, int on) {
    return guarded("mfx_ccd_set_profile", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_profile(on != 0);
    });
}
int mfx_ccd_rank_trace(mfx_ccd_t s, int cap, double* rmse, double* seconds, int iters_cap, int32_t* ranks_done) {
    int n = 0;
    const int rc = guarded("mfx_ccd_rank_trace", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null argument");
        MFX_REQUIRE(cap >= 0 && iters_cap >= 0, "negative capacity");
        n = s->impl->rank_trace(cap, rmse, seconds, iters_cap, ranks_done);
        return MFX_OK;
    });
    return rc == MFX_OK ? n : rc;
}
int mfx_ccd_layout_info(mfx_ccd_t s, int side, int32_t out[4]) {
    return guarded("mfx_ccd_layout_info", [&]() -> int {
        MFX_REQUIRE(s && s->impl && out, "null argument");
        MFX_REQUIRE(side == 0 || side == 1, "side must be 0 (CSC) or 1 (CSR)");
        s->impl->layout_info(side, out);
        return MFX_OK;
    });
}
int mfx_ccd_destroy(mfx_ccd_t s) {
    return guarded("mfx_ccd_destroy", [&]() -> int {
        return destroy_handle(s);
    });
}

/* ------------------------------------------------------------------ one-shot CCD++ */
int mfx_ccdpp_run(const mfx_csx* R, const mfx_coo* T, float* W, float* H, const mfx_params* p,
                  mfx_iter_report* reports) {
    return guarded("mfx_ccdpp_run", [&]() -> int {
        MFX_REQUIRE(R && W && H && p, "mfx_ccdpp_run: null argument");
        mfx_ccd_t s = nullptr;
        int rc = mfx_ccd_create(&s, R, T, p, MFX_HOST, nullptr);
        if (rc == MFX_OK) rc = mfx_ccd_set_factors(s, W, nullptr, MFX_HOST);
        if (rc == MFX_OK) rc = mfx_ccd_iterate(s, p->maxiter, 1, reports);
        if (rc == MFX_OK) rc = mfx_ccd_get_factors(s, W, H, MFX_HOST);
        mfx_ccd_destroy(s);
        if (rc != MFX_OK) fprintf(stderr, "CCD FAILED: %s\n", mfx_last_error()); /* CCD_CUDA.cu:174-176 */
        return rc;
    });
}

/* ------------------------------------------------------------------ ALS */
// The seven creates and the seven single halves of the ALS trainers: each fills an AlsSpec, which als_spec_check checks in the
// entry point's own order (AlsSolver::create, als_half).
using AlsM = AlsPlan::Method;
using AlsO = AlsPlan::Objective;

static int als_create(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space, const mfx_als_shard* shard,
                      const AlsSpec& spec) {
    // (argument checks before the device is touched)
    return make_handle(spec.fn, out, [&](AlsSolver** s) { return AlsSolver::create(s, R, T, p, space, shard, spec); });
}
// The checks of a half's arrays, then of its spec, then the half itself.  k_positive: mfx_als_half counts k <= 0 as a bad argument
static int als_half(AlsSpec spec, const HalfSegs& g, const float* X, const float* Y_in, float* Y_out, int64_t k, float lambda, int32_t* counts,
                    int device, bool k_positive = false) {
    spec.half = true;
    MFX_REQUIRE(g.nseg > 0 && g.nnz >= 0 && g.ptr && X && Y_out && (!k_positive || k > 0) && g.nrows_x > 0, "%s: bad argument", spec.fn);
    MFX_REQUIRE(g.nnz == 0 || (g.idx && g.val), "%s: null idx / val with nnz > 0", spec.fn);
    MFX_TRY(als_spec_check(spec, k, lambda, g.nseg, g.nrows_x, g.nnz));  // (with the sizes: their place differs by entry point)
    return als_plan_half_op(spec, g, X, Y_in, Y_out, k, lambda, counts, device);
}

int mfx_als_create(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, mfx_memspace space) {
    return guarded("mfx_als_create", [&]() -> int {
        return als_create(out, R, T, p, space, nullptr, AlsSpec{AlsM::Direct, AlsO::Als, "mfx_als_create"});
    });
}
int mfx_als_create_sharded(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p,
                           const mfx_als_shard* shard) {
    return guarded("mfx_als_create_sharded", [&]() -> int {
        MFX_REQUIRE(out && shard && shard->comm, "mfx_als_create_sharded: null argument");
        return als_create(out, R, T, p, MFX_HOST, shard, AlsSpec{AlsM::Direct, AlsO::Als, "mfx_als_create"});
    });
}
int mfx_als_set_factors(mfx_als_t s, const float* W, const float* H, mfx_memspace space) {
    return guarded("mfx_als_set_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_factors(W, H, space);
    });
}
int mfx_als_iterate(mfx_als_t s, int n_iter, int with_rmse, mfx_iter_report* reports) {
    return guarded("mfx_als_iterate", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->iterate(n_iter, with_rmse, reports);
    });
}
int mfx_als_get_factors(mfx_als_t s, float* W, float* H, mfx_memspace space) {
    return guarded("mfx_als_get_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_factors(W, H, space);
    });
}
int mfx_als_kernel_times(mfx_als_t s, int cap, const char** names, double* seconds, int64_t* launches) {
    return guarded("mfx_als_kernel_times", [&]() -> int {
        if (!s || !s->impl) return 0;
        return s->impl->kernel_times(cap, names, seconds, launches);
    });
}
int mfx_als_destroy(mfx_als_t s) {
    return guarded("mfx_als_destroy", [&]() -> int {
        return destroy_handle(s);
    });
}
/* ------------------------------------------------------------------ implicit-feedback ALS */
int mfx_ials_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, mfx_memspace space) {
    return guarded("mfx_ials_create", [&]() -> int {
        AlsSpec s{AlsM::Direct, AlsO::Implicit, "mfx_ials_create"};
        s.alpha = alpha;
        return als_create(out, R, nullptr, p, space, nullptr, s);
    });
}
int mfx_ials_block_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, int32_t block, mfx_memspace space) {
    return guarded("mfx_ials_block_create", [&]() -> int {
        AlsSpec s{AlsM::Blocks, AlsO::Implicit, "mfx_ials_block_create"};
        s.alpha = alpha; s.block = block;
        return als_create(out, R, nullptr, p, space, nullptr, s);
    });
}
int mfx_ials_block_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                        int64_t nrows_x, const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block,
                        float lambda, float alpha, int device) {
    return guarded("mfx_ials_block_half", [&]() -> int {
        AlsSpec s{AlsM::Blocks, AlsO::Implicit, "mfx_ials_block_half"};
        s.alpha = alpha; s.block = block;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, Y_in, Y_out, k, lambda, nullptr, device);
    });
}
/* ------------------------------------------------------------------ implicit ALS by conjugate gradients */
int mfx_ials_cg_create(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, int32_t steps, float tol, mfx_memspace space) {
    return guarded("mfx_ials_cg_create", [&]() -> int {
        AlsSpec s{AlsM::Cg, AlsO::Implicit, "mfx_ials_cg_create"};
        s.alpha = alpha; s.cap = steps; s.tol = tol;
        return als_create(out, R, nullptr, p, space, nullptr, s);
    });
}
int mfx_ials_cg_stats(mfx_als_t s, int64_t out[8]) {
    return guarded("mfx_ials_cg_stats", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "mfx_ials_cg_stats: null handle");
        return s->impl->cg_stats(out);
    });
}
int mfx_ials_cg_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x, const float* X,
                     const float* Y_in, float* Y_out, int64_t k, float lambda, float alpha, int32_t steps, float tol, int32_t* counts,
                     int device) {
    return guarded("mfx_ials_cg_half", [&]() -> int {
        AlsSpec s{AlsM::Cg, AlsO::Implicit, "mfx_ials_cg_half"};
        s.alpha = alpha; s.cap = steps; s.tol = tol;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, Y_in, Y_out, k, lambda, counts, device);
    });
}
int mfx_spd_inverse(int64_t k, const float* A, float* Ainv, int device) {
    return guarded("mfx_spd_inverse", [&]() -> int {
        MFX_REQUIRE(A && Ainv, "mfx_spd_inverse: null argument");
        return spd_inverse_op(k, A, Ainv, device);
    });
}
/* ------------------------------------------------------------------ explicit ALS by block subspace sweeps */
int mfx_als_block_create(mfx_als_t* out, const mfx_csx* R, const mfx_coo* T, const mfx_params* p, int32_t block, int32_t reg,
                         mfx_memspace space) {
    return guarded("mfx_als_block_create", [&]() -> int {
        AlsSpec s{AlsM::Blocks, reg == 1 ? AlsO::Ccd : AlsO::Als, "mfx_als_block_create"};
        s.block = block; s.reg = reg;
        return als_create(out, R, T, p, space, nullptr, s);
    });
}
int mfx_als_block_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x,
                       const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block, float lambda, int32_t reg, int device) {
    return guarded("mfx_als_block_half", [&]() -> int {
        AlsSpec s{AlsM::Blocks, reg == 1 ? AlsO::Ccd : AlsO::Als, "mfx_als_block_half"};
        s.block = block; s.reg = reg;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, Y_in, Y_out, k, lambda, nullptr, device);
    });
}
int mfx_ials_loss(mfx_als_t s, double* loss) {
    return guarded("mfx_ials_loss", [&]() -> int {
        MFX_REQUIRE(s && s->impl && loss, "mfx_ials_loss: null argument");
        return s->impl->loss(loss);
    });
}
int mfx_ials_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                  int64_t nrows_x, const float* X, float* Y, int64_t k, float lambda, float alpha, int device) {
    return guarded("mfx_ials_half", [&]() -> int {
        AlsSpec s{AlsM::Direct, AlsO::Implicit, "mfx_ials_half"};
        s.alpha = alpha;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, nullptr, Y, k, lambda, nullptr, device);
    });
}

/* ------------------------------------------------------------------ implicit ALS: unobserved weight, scaled regulariser */
int mfx_ials_create_reg(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, float alpha0, float nu, mfx_memspace space) {
    return guarded("mfx_ials_create_reg", [&]() -> int {
        AlsSpec s{AlsM::Direct, AlsO::ImplicitReg, "mfx_ials_create_reg"};
        s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu;
        return als_create(out, R, nullptr, p, space, nullptr, s);
    });
}
int mfx_ials_block_create_reg(mfx_als_t* out, const mfx_csx* R, const mfx_params* p, float alpha, float alpha0, float nu, int32_t block,
                              mfx_memspace space) {
    return guarded("mfx_ials_block_create_reg", [&]() -> int {
        MFX_REQUIRE(out, "mfx_ials_block_create_reg: out is NULL");  // (als_create repeats these two: they come before the
        *out = nullptr;                                              // block check here, and there for every other create)
        // (this entry point alone refuses a negative block before it looks at anything else)
        MFX_REQUIRE(block >= 0, "implicit ALS by block sweeps: block = %d (0 = chosen from k, else 1 <= block <= %u)", block, kIalsBlockMaxBlock);
        AlsSpec s{AlsM::Blocks, AlsO::ImplicitReg, "mfx_ials_block_create_reg"};
        s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu; s.block = block;
        return als_create(out, R, nullptr, p, space, nullptr, s);
    });
}
int mfx_ials_half_reg(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x, const float* X,
                      float* Y, int64_t k, float lambda, float alpha, float alpha0, float nu, int device) {
    return guarded("mfx_ials_half_reg", [&]() -> int {
        AlsSpec s{AlsM::Direct, AlsO::ImplicitReg, "mfx_ials_half_reg"};
        s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, nullptr, Y, k, lambda, nullptr, device);
    });
}
int mfx_ials_block_half_reg(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int64_t nrows_x,
                            const float* X, const float* Y_in, float* Y_out, int64_t k, int32_t block, float lambda, float alpha,
                            float alpha0, float nu, int device) {
    return guarded("mfx_ials_block_half_reg", [&]() -> int {
        AlsSpec s{AlsM::Blocks, AlsO::ImplicitReg, "mfx_ials_block_half_reg"};
        s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu; s.block = block;
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, Y_in, Y_out, k, lambda, nullptr, device);
    });
}

/* ------------------------------------------------------------------ BPR: deterministic mini-batch pairwise ranking */
int mfx_bpr_create(mfx_bpr_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed, mfx_memspace space) {
    return guarded("mfx_bpr_create", [&]() -> int {
        return make_handle("mfx_bpr_create", out, [&](BprSolver** s) { return BprSolver::create(s, R, p, lr, batch, seed, space); });
    });
}
int mfx_bpr_set_factors(mfx_bpr_t s, const float* W, const float* H, mfx_memspace space) {
    return guarded("mfx_bpr_set_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_factors(W, H, space);
    });
}
int mfx_bpr_get_factors(mfx_bpr_t s, float* W, float* H, mfx_memspace space) {
    return guarded("mfx_bpr_get_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_factors(W, H, space);
    });
}
int mfx_bpr_steps(mfx_bpr_t s, int64_t n_steps, int64_t stats[4], double* seconds) {
    return guarded("mfx_bpr_steps", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->steps(n_steps, stats, seconds);
    });
}
int mfx_bpr_epochs(mfx_bpr_t s, int32_t n_epochs, int64_t* stats, double* seconds) {
    return guarded("mfx_bpr_epochs", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->epochs(n_epochs, stats, seconds);
    });
}
int mfx_bpr_position(mfx_bpr_t s, int64_t* next_slot) {
    return guarded("mfx_bpr_position", [&]() -> int {
        MFX_REQUIRE(s && s->impl && next_slot, "null solver or next_slot");
        *next_slot = s->impl->position();
        return MFX_OK;
    });
}
int mfx_bpr_kernel_times(mfx_bpr_t s, double seconds[4]) {
    return guarded("mfx_bpr_kernel_times", [&]() -> int {
        MFX_REQUIRE(s && s->impl && seconds, "null solver or seconds");
        s->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_bpr_destroy(mfx_bpr_t s) {
    return guarded("mfx_bpr_destroy", [&]() -> int {
        return destroy_handle(s);
    });
}
int mfx_bpr_triples(uint64_t seed, int64_t first_slot, int64_t count, const mfx_csx* R, uint32_t* u, uint32_t* i, uint32_t* j,
                    uint8_t* skipped) {
    return guarded("mfx_bpr_triples", [&]() -> int { return bpr_triples(seed, first_slot, count, R, u, i, j, skipped); });
}
int mfx_bpr_apply(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i,
                  const uint32_t* j, const uint8_t* skipped, float lr, float lambda, int64_t stats[4], int device) {
    return guarded("mfx_bpr_apply", [&]() -> int { return bpr_apply(rows, cols, k, W, H, n, u, i, j, skipped, lr, lambda, stats, device); });
}
int mfx_bpr_create_neg(mfx_bpr_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, uint64_t seed, int32_t mode,
                       int64_t negatives, const float* rank_weight, mfx_memspace space) {
    return guarded("mfx_bpr_create_neg", [&]() -> int {
        return make_handle("mfx_bpr_create_neg", out, [&](BprSolver** s) {
            return BprSolver::create(s, R, p, lr, batch, seed, space, "mfx_bpr_create_neg", mode, negatives, rank_weight);
        });
    });
}
int mfx_bpr_trials(uint64_t seed, int64_t first_slot, int64_t count, int64_t negatives, const mfx_csx* R, uint32_t* u, uint32_t* i,
                   uint32_t* items, uint8_t* member) {
    return guarded("mfx_bpr_trials", [&]() -> int { return bpr_trials(seed, first_slot, count, negatives, R, u, i, items, member); });
}
int mfx_bpr_rank_weights(int64_t cols, int64_t negatives, float* out) {
    return guarded("mfx_bpr_rank_weights", [&]() -> int { return bpr_rank_weights(cols, negatives, out); });
}
int mfx_bpr_apply_neg(int64_t rows, int64_t cols, int64_t k, float* W, float* H, int64_t n, const uint32_t* u, const uint32_t* i,
                      int64_t negatives, const uint32_t* items, const uint8_t* member, int32_t mode, const float* rank_weight, float lr,
                      float lambda, int64_t stats[4], uint32_t* j_out, uint32_t* t_out, int device) {
    return guarded("mfx_bpr_apply_neg", [&]() -> int {
        return bpr_apply_neg(rows, cols, k, W, H, n, u, i, negatives, items, member, mode, rank_weight, lr, lambda, stats, j_out, t_out, device);
    });
}
int mfx_bpr_trial_stats(mfx_bpr_t s, int64_t out[2]) {
    return guarded("mfx_bpr_trial_stats", [&]() -> int {
        MFX_REQUIRE(s && s->impl && out, "null solver or out");
        s->impl->trial_stats(out);
        return MFX_OK;
    });
}

/* ------------------------------------------------------------------ LightGCN: BPR on graph-propagated embeddings */
int mfx_lgcn_create(mfx_lgcn_t* out, const mfx_csx* R, const mfx_params* p, float lr, int64_t batch, int32_t layers, uint64_t seed,
                    mfx_memspace space) {
    return guarded("mfx_lgcn_create", [&]() -> int {
        return make_handle("mfx_lgcn_create", out, [&](LgcnSolver** s) { return LgcnSolver::create(s, R, p, lr, batch, layers, seed, space); });
    });
}
int mfx_lgcn_set_base(mfx_lgcn_t s, const float* W0, const float* H0, mfx_memspace space) {
    return guarded("mfx_lgcn_set_base", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_base(W0, H0, space);
    });
}
int mfx_lgcn_get_base(mfx_lgcn_t s, float* W0, float* H0, mfx_memspace space) {
    return guarded("mfx_lgcn_get_base", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_base(W0, H0, space);
    });
}
int mfx_lgcn_get_factors(mfx_lgcn_t s, float* W, float* H, mfx_memspace space) {
    return guarded("mfx_lgcn_get_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_factors(W, H, space);
    });
}
int mfx_lgcn_steps(mfx_lgcn_t s, int64_t n_steps, int64_t stats[4], double* seconds) {
    return guarded("mfx_lgcn_steps", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->steps(n_steps, stats, seconds);
    });
}
int mfx_lgcn_epochs(mfx_lgcn_t s, int32_t n_epochs, int64_t* stats, double* seconds) {
    return guarded("mfx_lgcn_epochs", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->epochs(n_epochs, stats, seconds);
    });
}
int mfx_lgcn_position(mfx_lgcn_t s, int64_t* next_slot) {
    return guarded("mfx_lgcn_position", [&]() -> int {
        MFX_REQUIRE(s && s->impl && next_slot, "null solver or next_slot");
        *next_slot = s->impl->position();
        return MFX_OK;
    });
}
int mfx_lgcn_kernel_times(mfx_lgcn_t s, double seconds[6]) {
    return guarded("mfx_lgcn_kernel_times", [&]() -> int {
        MFX_REQUIRE(s && s->impl && seconds, "null solver or seconds");
        s->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_lgcn_destroy(mfx_lgcn_t s) {
    return guarded("mfx_lgcn_destroy", [&]() -> int {
        return destroy_handle(s);
    });
}
int mfx_lgcn_propagate(const mfx_csx* R, const float* W0, const float* H0, int64_t k, int32_t layers, float* W, float* H, int device) {
    return guarded("mfx_lgcn_propagate", [&]() -> int { return lgcn_propagate(R, W0, H0, k, layers, W, H, device); });
}
int mfx_lgcn_apply(const mfx_csx* R, int64_t k, float* W0, float* H0, int64_t n, const uint32_t* u, const uint32_t* i, const uint32_t* j,
                   const uint8_t* skipped, int32_t layers, float lr, float lambda, int64_t stats[4], int device) {
    return guarded("mfx_lgcn_apply", [&]() -> int { return lgcn_apply(R, k, W0, H0, n, u, i, j, skipped, layers, lr, lambda, stats, device); });
}

/* ------------------------------------------------------------------ hybrid BPR: rows embedded through their features */
int mfx_hyb_create(mfx_hyb_t* out, const mfx_csx* R, const mfx_features* Fu, const mfx_features* Fi, const mfx_params* p, float lr,
                   int64_t batch, uint64_t seed, mfx_memspace space) {
    return guarded("mfx_hyb_create", [&]() -> int {
        return make_handle("mfx_hyb_create", out, [&](HybSolver** s) { return HybSolver::create(s, R, Fu, Fi, p, lr, batch, seed, space); });
    });
}
int mfx_hyb_set_embeddings(mfx_hyb_t s, const float* Eu, const float* Ei, mfx_memspace space) {
    return guarded("mfx_hyb_set_embeddings", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->set_embeddings(Eu, Ei, space);
    });
}
int mfx_hyb_get_embeddings(mfx_hyb_t s, float* Eu, float* Ei, mfx_memspace space) {
    return guarded("mfx_hyb_get_embeddings", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_embeddings(Eu, Ei, space);
    });
}
int mfx_hyb_get_factors(mfx_hyb_t s, float* W, float* H, mfx_memspace space) {
    return guarded("mfx_hyb_get_factors", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->get_factors(W, H, space);
    });
}
int mfx_hyb_steps(mfx_hyb_t s, int64_t n_steps, int64_t stats[4], double* seconds) {
    return guarded("mfx_hyb_steps", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->steps(n_steps, stats, seconds);
    });
}
int mfx_hyb_epochs(mfx_hyb_t s, int32_t n_epochs, int64_t* stats, double* seconds) {
    return guarded("mfx_hyb_epochs", [&]() -> int {
        MFX_REQUIRE(s && s->impl, "null solver");
        return s->impl->epochs(n_epochs, stats, seconds);
    });
}
int mfx_hyb_position(mfx_hyb_t s, int64_t* next_slot) {
    return guarded("mfx_hyb_position", [&]() -> int {
        MFX_REQUIRE(s && s->impl && next_slot, "null solver or next_slot");
        *next_slot = s->impl->position();
        return MFX_OK;
    });
}
int mfx_hyb_kernel_times(mfx_hyb_t s, double seconds[6]) {
    return guarded("mfx_hyb_kernel_times", [&]() -> int {
        MFX_REQUIRE(s && s->impl && seconds, "null solver or seconds");
        s->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_hyb_destroy(mfx_hyb_t s) {
    return guarded("mfx_hyb_destroy", [&]() -> int {
        return destroy_handle(s);
    });
}
int mfx_hyb_embed(const mfx_features* F, const float* E, int64_t k, float* out, int device) {
    return guarded("mfx_hyb_embed", [&]() -> int { return hyb_embed(F, E, k, out, device); });
}
int mfx_hyb_apply(int64_t rows, int64_t cols, int64_t k, const mfx_features* Fu, const mfx_features* Fi, float* Eu, float* Ei, int64_t n,
                  const uint32_t* u, const uint32_t* i, const uint32_t* j, const uint8_t* skipped, float lr, float lambda, int64_t stats[4],
                  int device) {
    return guarded("mfx_hyb_apply", [&]() -> int { return hyb_apply(rows, cols, k, Fu, Fi, Eu, Ei, n, u, i, j, skipped, lr, lambda, stats, device); });
}

/* ------------------------------------------------------------------ item-kNN: neighbour lists on the interaction matrix */
int mfx_knn_build(mfx_knn_t* out, const mfx_csx* X, int32_t K, int32_t tile_items, mfx_memspace space, int device) {
    return guarded("mfx_knn_build", [&]() -> int {
        return make_handle("mfx_knn_build", out, [&](Knn** h) { return Knn::build(h, X, K, tile_items, space, device); });
    });
}
int mfx_knn_create_from_lists(mfx_knn_t* out, int64_t cols, int32_t K, const uint32_t* nbr_idx, const float* nbr_sim, mfx_memspace space,
                              int device) {
    return guarded("mfx_knn_create_from_lists", [&]() -> int {
        return make_handle("mfx_knn_create_from_lists", out,
                           [&](Knn** h) { return Knn::from_lists(h, cols, K, nbr_idx, nbr_sim, space, device); });
    });
}
int mfx_knn_lists(mfx_knn_t h, uint32_t* nbr_idx, float* nbr_sim, mfx_memspace space) {
    return guarded("mfx_knn_lists", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_knn_lists: null handle");
        return h->impl->lists(nbr_idx, nbr_sim, space);
    });
}
int mfx_knn_neighbours(mfx_knn_t h, int64_t nq, const uint32_t* items, int32_t n_top, uint32_t* out_items, float* out_sims,
                       mfx_memspace space) {
    return guarded("mfx_knn_neighbours", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_knn_neighbours: null handle");
        return h->impl->neighbours(nq, items, n_top, out_items, out_sims, space);
    });
}
int mfx_knn_recommend(mfx_knn_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top,
                      int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return guarded("mfx_knn_recommend", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_knn_recommend: null handle");
        return h->impl->recommend(nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space);
    });
}
int mfx_knn_times(mfx_knn_t h, double seconds[4]) {
    return guarded("mfx_knn_times", [&]() -> int {
        MFX_REQUIRE(h && h->impl && seconds, "mfx_knn_times: null handle or seconds");
        h->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_knn_destroy(mfx_knn_t h) {
    return guarded("mfx_knn_destroy", [&]() -> int {
        return destroy_handle(h);
    });
}

/* ------------------------------------------------------------------ SLIM: sparse linear item models on given supports */
int mfx_slim_train(mfx_slim_t* out, const mfx_csx* X, int32_t K, const uint32_t* support, float l1, float l2, int32_t sweeps, float tol, int flags,
                   int32_t tile_items, int64_t* failed, mfx_memspace space, int device) {
    return guarded("mfx_slim_train", [&]() -> int {
        return make_handle("mfx_slim_train", out, [&](Slim** h) {
            return Slim::train(h, X, K, support, SlimParams{l1, l2, tol, sweeps, flags}, tile_items, failed, space, device);
        });
    });
}
int mfx_slim_gram(const mfx_csx* X, int32_t K, const uint32_t* support, int32_t tile_items, float* blocks, mfx_memspace space, int device) {
    return guarded("mfx_slim_gram", [&]() -> int { return Slim::gram(X, K, support, tile_items, blocks, space, device); });
}
int mfx_slim_solve(int64_t n, int32_t K, const float* blocks, const uint32_t* n_real, float l1, float l2, int32_t sweeps, float tol, int flags,
                   float* w, int32_t* sweeps_used, int64_t* failed, mfx_memspace space, int device) {
    return guarded("mfx_slim_solve", [&]() -> int {
        return Slim::solve(n, K, blocks, n_real, SlimParams{l1, l2, tol, sweeps, flags}, w, sweeps_used, failed, space, device);
    });
}
int mfx_slim_create_from_lists(mfx_slim_t* out, int64_t cols, int32_t K, const uint32_t* support, const float* w, mfx_memspace space,
                               int device) {
    return guarded("mfx_slim_create_from_lists", [&]() -> int {
        return make_handle("mfx_slim_create_from_lists", out, [&](Slim** h) { return Slim::from_lists(h, cols, K, support, w, space, device); });
    });
}
int mfx_slim_weights(mfx_slim_t h, uint32_t* support, float* w, int32_t* sweeps_used, mfx_memspace space) {
    return guarded("mfx_slim_weights", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_slim_weights: null handle");
        return h->impl->weights(support, w, sweeps_used, space);
    });
}
int mfx_slim_recommend(mfx_slim_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top,
                       int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return guarded("mfx_slim_recommend", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_slim_recommend: null handle");
        return h->impl->recommend(nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space);
    });
}
int mfx_slim_times(mfx_slim_t h, double seconds[5]) {
    return guarded("mfx_slim_times", [&]() -> int {
        MFX_REQUIRE(h && h->impl && seconds, "mfx_slim_times: null handle or seconds");
        h->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_slim_destroy(mfx_slim_t h) {
    return guarded("mfx_slim_destroy", [&]() -> int {
        return destroy_handle(h);
    });
}

/* ------------------------------------------------------------------ EASE: closed-form dense item-item models */
int mfx_ease_gram(const mfx_csx* X, float lambda, int32_t tile_items, float* G, mfx_memspace space, int device) {
    return guarded("mfx_ease_gram", [&]() -> int { return Ease::gram(X, lambda, tile_items, G, space, device); });
}
int mfx_ease_inverse(int64_t n, const float* A, float* Ainv, int flags, mfx_memspace space, int device) {
    return guarded("mfx_ease_inverse", [&]() -> int { return Ease::inverse(n, A, Ainv, flags, space, device); });
}
int mfx_ease_weights_from_inverse(int64_t n, const float* P, float* B, mfx_memspace space, int device) {
    return guarded("mfx_ease_weights_from_inverse", [&]() -> int { return Ease::weights_from_inverse(n, P, B, space, device); });
}
int mfx_ease_train(mfx_ease_t* out, const mfx_csx* X, float lambda, int flags, int32_t tile_items, mfx_memspace space, int device) {
    return guarded("mfx_ease_train", [&]() -> int {
        return make_handle("mfx_ease_train", out, [&](Ease** h) { return Ease::train(h, X, lambda, flags, tile_items, space, device); });
    });
}
int mfx_ease_create_from_weights(mfx_ease_t* out, int64_t cols, const float* B, mfx_memspace space, int device) {
    return guarded("mfx_ease_create_from_weights", [&]() -> int {
        return make_handle("mfx_ease_create_from_weights", out, [&](Ease** h) { return Ease::from_weights(h, cols, B, space, device); });
    });
}
int mfx_ease_weights(mfx_ease_t h, int64_t first, int64_t count, float* B_rows, mfx_memspace space) {
    return guarded("mfx_ease_weights", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_ease_weights: null handle");
        return h->impl->weights(first, count, B_rows, space);
    });
}
int mfx_ease_recommend(mfx_ease_t h, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_top,
                       int flags, int32_t tile_items, uint32_t* items, float* scores, int64_t* bad_rows, mfx_memspace space) {
    return guarded("mfx_ease_recommend", [&]() -> int {
        MFX_REQUIRE(h && h->impl, "mfx_ease_recommend: null handle");
        return h->impl->recommend(nusers, nnz, ptr, idx, val, n_top, flags, tile_items, items, scores, bad_rows, space);
    });
}
int mfx_ease_times(mfx_ease_t h, double seconds[6]) {
    return guarded("mfx_ease_times", [&]() -> int {
        MFX_REQUIRE(h && h->impl && seconds, "mfx_ease_times: null handle or seconds");
        h->impl->times(seconds);
        return MFX_OK;
    });
}
int mfx_ease_destroy(mfx_ease_t h) {
    return guarded("mfx_ease_destroy", [&]() -> int {
        return destroy_handle(h);
    });
}

int mfx_als_run(const mfx_csx* R, const mfx_coo* T, float* W, float* H, const mfx_params* p,
                mfx_iter_report* reports) {
    return guarded("mfx_als_run", [&]() -> int {
        MFX_REQUIRE(R && W && H && p, "mfx_als_run: null argument");
        mfx_als_t s = nullptr;
        int rc = mfx_als_create(&s, R, T, p, MFX_HOST);
        if (rc == MFX_OK) rc = mfx_als_set_factors(s, nullptr, H, MFX_HOST);
        if (rc == MFX_OK) rc = mfx_als_iterate(s, p->maxiter, 1, reports);
        if (rc == MFX_OK) rc = mfx_als_get_factors(s, W, H, MFX_HOST);
        mfx_als_destroy(s);
        if (rc != MFX_OK) fprintf(stderr, "ALS FAILED: %s\n", mfx_last_error()); /* ALS_CUDA.cu:193-195 */
        return rc;
    });
}

/* ------------------------------------------------------------------ single operators */
namespace {
struct OpCtx {
    hipStream_t st = nullptr;
    ~OpCtx() { if (st) { (void) hipStreamSynchronize(st); (void) hipStreamDestroy(st); } }
    int open(int device) {
        MFX_TRY(use_device(device));
        MFX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return MFX_OK;
    }
};
}  // namespace

// variant -> layout of the single-operator entry points (see mfx.h)
// variants of the single-operator entry points: -1 reference order / 0 wave per segment (plain layout), 1 flat (plain),
// 2 flat with the layout chosen for the shape, >= 16 explicit LDS panel, <= -16 explicit cache panel.  Anything else is an error.
static bool op_variant_ok(int variant) { return variant == -1 || variant == 0 || variant == 1 || variant == 2 || variant >= 16 || variant <= -16; }
static FlatLayoutOptions op_layout(const CcdKnobs& kn, int variant, int64_t nseg, int64_t nnz, int64_t vec_len) {
    mfx_params p;
    mfx_params_default(&p);
    p.panel_rows = (variant >= 16 || variant <= -16) ? variant : variant == 2 ? 0 : -1;
    return choose_layout(p, kn, (uint32_t) nseg, (uint64_t) nnz, (uint32_t) vec_len, sizeof(float), variant == 0 || variant == -1);
}

int mfx_rank_one_sweep(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                       int64_t vec_len, const float* vec, float lambda, float* out, int variant, int device) {
    return guarded("mfx_rank_one_sweep", [&]() -> int {
        const CcdKnobs kn = CcdKnobs::from_env();
        MFX_REQUIRE(nseg > 0 && nnz >= 0 && vec_len > 0 && ptr && vec && out, "mfx_rank_one_sweep: bad argument");
        MFX_REQUIRE(nnz == 0 || (idx && val), "mfx_rank_one_sweep: null idx / val with nnz > 0");
        MFX_REQUIRE(nseg < (int64_t) 0xFFFFFFFFll && vec_len < (int64_t) 0xFFFFFFFFll && nnz < (int64_t) 0xFFFF0000ll,
                    "mfx_rank_one_sweep: sizes exceed the 32-bit index range");
        MFX_REQUIRE(op_variant_ok(variant), "mfx_rank_one_sweep: variant must be -1, 0, 1, 2, >= 16 or <= -16 (got %d)", variant);
        OpCtx cx;
        MFX_TRY(cx.open(device));
        SegStreamStore s;
        MFX_TRY(s.build((uint32_t) nseg, (uint64_t) nnz, (uint32_t) vec_len, ptr, idx, val, MFX_HOST,
                        op_layout(kn, variant, nseg, nnz, vec_len), 0, cx.st));
        DevBuf<float> dvec, dout, gh;
        MFX_TRY(dvec.alloc(vec_len)); MFX_TRY(dvec.upload(vec, vec_len, MFX_HOST, cx.st));
        MFX_TRY(dout.alloc(nseg));
        FinalizeArgs f; f.lambda = lambda; f.out_vec = dout.get();
        if (variant == -1) {  // the reference's summation order: sums and division in one kernel (ccd_reforder.hip)
            std::vector<uint32_t> order;
            const bool old_form = !kn.ref_fused;  // (MFX_REF_FUSED=0, A/B: the r3 / early-r4 kernels)
            const uint32_t nlong = ref_sweep_order(ptr, (uint32_t) nseg, &order, !old_form, kn.ref_long);
            DevBuf<uint32_t> dorder;
            MFX_TRY(dorder.alloc(order.size())); MFX_TRY(dorder.upload(order.data(), order.size(), MFX_HOST, cx.st));
            if (old_form) {
                MFX_TRY(launch_sweep_ref(s.view, dorder.get(), nlong, dvec.get(), lambda, dout.get(), cx.st, kn.ref_sweep_dpp));
            } else {
                RefOwnerCtx rs;
                kn.apply(rs);
                rs.main = cx.st;  // (one stream: the long segments' kernel first, the others behind it)
                MFX_TRY(launch_ref_owner(FM_SWEEP, s.view, dorder.get(), nlong, dvec.get(), nullptr, f, rs));
            }
            MFX_HIP(hipMemcpyAsync(out, dout.get(), sizeof(float) * nseg, hipMemcpyDeviceToHost, cx.st));
            MFX_HIP(hipStreamSynchronize(cx.st));
            return MFX_OK;
        }
        if (variant == 0) {
            MFX_TRY(gh.alloc_zero((size_t) 2 * nseg, cx.st));
            MFX_TRY(launch_sweep_wave(s.view, dvec.get(), gh.get(), gh.get() + nseg, cx.st));
            f.gh_dense = gh.get();
        } else {
            MFX_TRY(launch_flat(FM_SWEEP, s.view, dvec.get(), nullptr, 0, cx.st));
        }
        MFX_TRY(launch_finalize(s.view, f, cx.st));
        MFX_HIP(hipMemcpyAsync(out, dout.get(), sizeof(float) * nseg, hipMemcpyDeviceToHost, cx.st));
        MFX_HIP(hipStreamSynchronize(cx.st));
        return MFX_OK;
    });
}

int mfx_update_rating(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, float* val,
                      int64_t vec_len, const float* gathered, const float* per_seg, int add, int variant,
                      int device) {
    return guarded("mfx_update_rating", [&]() -> int {
        const CcdKnobs kn = CcdKnobs::from_env();
        MFX_REQUIRE(nseg > 0 && nnz >= 0 && vec_len > 0 && ptr && gathered && per_seg, "mfx_update_rating: bad argument");
        MFX_REQUIRE(nnz == 0 || (idx && val), "mfx_update_rating: null idx / val with nnz > 0");
        MFX_REQUIRE(nseg < (int64_t) 0xFFFFFFFFll && vec_len < (int64_t) 0xFFFFFFFFll && nnz < (int64_t) 0xFFFF0000ll,
                    "mfx_update_rating: sizes exceed the 32-bit index range");
        MFX_REQUIRE(op_variant_ok(variant), "mfx_update_rating: variant must be -1, 0, 1, 2, >= 16 or <= -16 (got %d)", variant);
        OpCtx cx;
        MFX_TRY(cx.open(device));
        SegStreamStore s;
        MFX_TRY(s.build((uint32_t) nseg, (uint64_t) nnz, (uint32_t) vec_len, ptr, idx, val, MFX_HOST,
                        op_layout(kn, variant, nseg, nnz, vec_len), 0, cx.st));
        DevBuf<float> dg, dp;
        MFX_TRY(dg.alloc(vec_len)); MFX_TRY(dg.upload(gathered, vec_len, MFX_HOST, cx.st));
        MFX_TRY(dp.alloc(nseg)); MFX_TRY(dp.upload(per_seg, nseg, MFX_HOST, cx.st));
        // 0: one wavefront per segment; -1 takes the flat kernel over its plain layout, like CcdSolver::resid (the update is
        // elementwise -- bit-identical in every kernel)
        if (variant == 0) MFX_TRY(launch_resid_wave(s.view, dg.get(), dp.get(), add, cx.st));
        else MFX_TRY(launch_flat(FM_RESID, s.view, dg.get(), dp.get(), add, cx.st));
        if (nnz) {
            DevBuf<float> tmp;
            MFX_TRY(tmp.alloc(nnz));
            MFX_TRY(s.unpermute(tmp.get(), cx.st));
            MFX_HIP(hipMemcpyAsync(val, tmp.get(), sizeof(float) * nnz, hipMemcpyDeviceToHost, cx.st));
            MFX_HIP(hipStreamSynchronize(cx.st));
        }
        MFX_HIP(hipStreamSynchronize(cx.st));
        return MFX_OK;
    });
}

int mfx_test_rmse(const mfx_coo* T, const float* W, const float* H, int64_t rows, int64_t cols, int64_t k,
                  int ifALS, double* rmse_out, int device) {
    return guarded("mfx_test_rmse", [&]() -> int {
        MFX_REQUIRE(T && W && H && rmse_out && rows > 0 && cols > 0 && k > 0, "mfx_test_rmse: bad argument");
        MFX_REQUIRE(rows < (int64_t) 0xFFFFFFFFll && cols < (int64_t) 0xFFFFFFFFll, "mfx_test_rmse: sizes exceed the 32-bit index range");
        MFX_REQUIRE(T->nnz <= 0 || (T->row && T->col && T->val), "mfx_test_rmse: null test array");
        *rmse_out = 0.0;
        if (T->nnz <= 0) return MFX_OK;
        OpCtx cx;
        MFX_TRY(cx.open(device));
        DevBuf<uint32_t> r, c; DevBuf<float> v, dW, dH; DevBuf<double> part, sum;
        MFX_TRY(r.alloc(T->nnz)); MFX_TRY(r.upload(T->row, T->nnz, MFX_HOST, cx.st));
        MFX_TRY(c.alloc(T->nnz)); MFX_TRY(c.upload(T->col, T->nnz, MFX_HOST, cx.st));
        MFX_TRY(v.alloc(T->nnz)); MFX_TRY(v.upload(T->val, T->nnz, MFX_HOST, cx.st));
        MFX_TRY(check_index_range(r.get(), (uint64_t) T->nnz, (uint32_t) rows, "test-set row", cx.st));
        MFX_TRY(check_index_range(c.get(), (uint64_t) T->nnz, (uint32_t) cols, "test-set column", cx.st));
        MFX_TRY(dW.alloc((size_t) rows * k)); MFX_TRY(dW.upload(W, (size_t) rows * k, MFX_HOST, cx.st));
        MFX_TRY(dH.alloc((size_t) cols * k)); MFX_TRY(dH.upload(H, (size_t) cols * k, MFX_HOST, cx.st));
        MFX_TRY(part.alloc_zero(kRmseBlocks, cx.st)); MFX_TRY(sum.alloc_zero(1, cx.st));
        MFX_TRY(launch_test_sqerr(T->nnz, r.get(), c.get(), v.get(), dW.get(), dH.get(), rows, cols, k, ifALS,
                                  part.get(), kRmseBlocks, sum.get(), cx.st));
        double s = 0;
        MFX_HIP(hipMemcpyAsync(&s, sum.get(), sizeof(double), hipMemcpyDeviceToHost, cx.st));
        MFX_HIP(hipStreamSynchronize(cx.st));
        *rmse_out = std::sqrt(s / (double) T->nnz);
        return MFX_OK;
    });
}

int mfx_als_gramian(int64_t cnt, const uint32_t* idx, int64_t nrows_x, const float* X, int64_t k, float* A,
                    int device) {
    return guarded("mfx_als_gramian", [&]() -> int {
        MFX_REQUIRE(cnt >= 0 && nrows_x > 0 && k > 0 && X && A && (cnt == 0 || idx), "mfx_als_gramian: bad argument");
        return als_gramian_op(cnt, idx, nrows_x, X, k, A, device);
    });
}

int mfx_als_inverse(int64_t k, const float* A, float* Ainv, int device) {
    return guarded("mfx_als_inverse", [&]() -> int {
        MFX_REQUIRE(A && Ainv, "mfx_als_inverse: null argument");
        return als_inverse_op(k, A, Ainv, device);
    });
}

int mfx_als_half(int64_t nseg, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                 int64_t nrows_x, const float* X, float* Y, int64_t k, float lambda, int variant, int device) {
    return guarded("mfx_als_half", [&]() -> int {
        const AlsSpec s{variant == 0 ? AlsM::DirectExact : AlsM::Direct, AlsO::Als, "mfx_als_half"};
        return als_half(s, {nseg, nnz, ptr, idx, val, nrows_x}, X, nullptr, Y, k, lambda, nullptr, device, true);
    });
}

/* ------------------------------------------------------------------ top-N recommendation */
int mfx_rec_create(mfx_rec_t* out, const float* W, const float* H, int64_t rows, int64_t cols, int64_t k, int layout,
                   const mfx_csx* exclude, mfx_memspace space, int device) {
    return guarded("mfx_rec_create", [&]() -> int {
        return make_handle("mfx_rec_create", out, [&](Recommender** r) {
            return Recommender::create(r, W, H, rows, cols, k, layout, exclude, space, device);
        });
    });
}
int mfx_rec_query(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t n_top, uint32_t* items, float* scores,
                  mfx_memspace space, int item_slices) {
    return guarded("mfx_rec_query", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->query(nusers, users, n_top, items, scores, space, item_slices);
    });
}
// The seven fold-in setups: each fills a FoldSpec for Recommender::fold_setup, which checks it in the entry point's order.
using FoldM = FoldPlan::Method;
using FoldO = FoldPlan::Objective;

int mfx_rec_fold_in_setup(mfx_rec_t r, int model, float lambda, float alpha) {
    return guarded("mfx_rec_fold_in_setup", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->fold_setup("mfx_rec_fold_in_setup", FoldSpec::of_model(FoldM::Direct, model, lambda, alpha));
    });
}
int mfx_rec_fold_in(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                    float* W_out, int32_t n_top, uint32_t* items, float* scores, mfx_memspace space) {
    return guarded("mfx_rec_fold_in", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->fold_in(nusers, nnz, ptr, idx, val, W_out, n_top, items, scores, space);
    });
}
int mfx_rec_fold_in_block_setup(mfx_rec_t r, float lambda, float alpha, int32_t block, int32_t sweeps, float tol) {
    return guarded("mfx_rec_fold_in_block_setup", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        FoldSpec s{FoldM::Blocks, FoldO::Implicit};
        s.lambda = lambda; s.alpha = alpha; s.block = block; s.cap = sweeps; s.tol = tol;
        return r->impl->fold_setup("mfx_rec_fold_in_block_setup", s);
    });
}
int mfx_rec_fold_in_setup_reg(mfx_rec_t r, float lambda, float alpha, float alpha0, float nu) {
    return guarded("mfx_rec_fold_in_setup_reg", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "mfx_rec_fold_in_setup_reg: null handle");
        FoldSpec s{FoldM::Direct, FoldO::ImplicitReg, MFX_FOLD_IMPLICIT};
        s.lambda = lambda; s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu;
        return r->impl->fold_setup("mfx_rec_fold_in_setup_reg", s);
    });
}
int mfx_rec_fold_in_block_setup_reg(mfx_rec_t r, float lambda, float alpha, float alpha0, float nu, int32_t block, int32_t sweeps, float tol) {
    return guarded("mfx_rec_fold_in_block_setup_reg", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "mfx_rec_fold_in_block_setup_reg: null handle");
        FoldSpec s{FoldM::Blocks, FoldO::ImplicitReg};
        s.lambda = lambda; s.alpha = alpha; s.alpha0 = alpha0; s.nu = nu; s.block = block; s.cap = sweeps; s.tol = tol;
        return r->impl->fold_setup("mfx_rec_fold_in_block_setup_reg", s);
    });
}
int mfx_rec_fold_in_block_setup_als(mfx_rec_t r, float lambda, int32_t reg, int32_t block, int32_t sweeps, float tol) {
    return guarded("mfx_rec_fold_in_block_setup_als", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        FoldSpec s{FoldM::Blocks, reg == 1 ? FoldO::Ccd : FoldO::Als, reg};
        s.lambda = lambda; s.block = block; s.cap = sweeps; s.tol = tol;
        return r->impl->fold_setup("mfx_rec_fold_in_block_setup_als", s);
    });
}
int mfx_rec_fold_in_cg_setup(mfx_rec_t r, int model, float lambda, float alpha, int32_t steps, float tol) {
    return guarded("mfx_rec_fold_in_cg_setup", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        FoldSpec s = FoldSpec::of_model(FoldM::Cg, model, lambda, alpha);
        s.cap = steps; s.tol = tol;
        return r->impl->fold_setup("mfx_rec_fold_in_cg_setup", s);
    });
}
int mfx_rec_fold_in_warm(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val,
                         const float* W_init, float* W_out, int32_t* sweeps_done, int32_t n_top, uint32_t* items, float* scores,
                         mfx_memspace space) {
    return guarded("mfx_rec_fold_in_warm", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->fold_in_warm(nusers, nnz, ptr, idx, val, W_init, W_out, sweeps_done, n_top, items, scores, space);
    });
}
int mfx_rec_explain(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                    const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out,
                    float* Z_out, mfx_memspace space) {
    return guarded("mfx_rec_explain", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "mfx_rec_explain: null handle");
        return r->impl->explain(nusers, nnz, ptr, idx, val, n_targets, targets, n_expl, expl_items, expl_contrib, totals, W_out, Z_out, space);
    });
}
int mfx_rec_explain_cg(mfx_rec_t r, int64_t nusers, int64_t nnz, const uint32_t* ptr, const uint32_t* idx, const float* val, int32_t n_targets,
                       const uint32_t* targets, int32_t n_expl, uint32_t* expl_items, float* expl_contrib, float* totals, float* W_out,
                       float* Z_out, int32_t* row_steps, int32_t* target_steps, mfx_memspace space) {
    return guarded("mfx_rec_explain_cg", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "mfx_rec_explain_cg: null handle");
        return r->impl->explain_cg(nusers, nnz, ptr, idx, val, n_targets, targets, n_expl, expl_items, expl_contrib, totals, W_out, Z_out,
                                   row_steps, target_steps, space);
    });
}
int mfx_rec_explain_times(mfx_rec_t r, double seconds[3]) {
    return guarded("mfx_rec_explain_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "mfx_rec_explain_times: null argument");
        r->impl->explain_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_fold_in_times(mfx_rec_t r, double seconds[3]) {
    return guarded("mfx_rec_fold_in_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "null recommender or seconds");
        r->impl->fold_in_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_set_item_filter(mfx_rec_t r, const uint8_t* keep, mfx_memspace space) {
    return guarded("mfx_rec_set_item_filter", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->set_item_filter(keep, space);
    });
}
int mfx_rec_similar_setup(mfx_rec_t r) {
    return guarded("mfx_rec_similar_setup", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->similar_setup();
    });
}
int mfx_rec_item_norms(mfx_rec_t r, float* n2, float* c, mfx_memspace space) {
    return guarded("mfx_rec_item_norms", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->item_norms(n2, c, space);
    });
}
int mfx_rec_similar(mfx_rec_t r, int64_t nq, const uint32_t* query_items, int metric, int exclude_self, int32_t n_top,
                    uint32_t* items, float* scores, mfx_memspace space, int item_slices) {
    return guarded("mfx_rec_similar", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->similar(nq, query_items, metric, exclude_self, n_top, items, scores, space, item_slices);
    });
}
int mfx_rec_rank(mfx_rec_t r, int64_t npairs, const uint32_t* users, const uint32_t* items, uint32_t* ranks, float* scores,
                 uint32_t* n_eligible, mfx_memspace space, int item_slices) {
    return guarded("mfx_rec_rank", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->rank(npairs, users, items, ranks, scores, n_eligible, space, item_slices);
    });
}
int mfx_rec_rank_times(mfx_rec_t r, double seconds[3]) {
    return guarded("mfx_rec_rank_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "null recommender or seconds");
        r->impl->rank_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_evaluate(mfx_rec_t r, const mfx_coo* T, float min_rating, int32_t n_cut, const int32_t* cutoffs, double* out,
                     double* mrr, double* auc, int64_t* users_evaluated, int64_t* auc_users, mfx_memspace space) {
    return guarded("mfx_rec_evaluate", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->evaluate(T, min_rating, n_cut, cutoffs, out, mrr, auc, users_evaluated, auc_users, space);
    });
}
int mfx_rec_query_candidates(mfx_rec_t r, int64_t nusers, const uint32_t* users, const uint32_t* cand_ptr, const uint32_t* cand_idx,
                             int32_t flags, int32_t n_top, uint32_t* items, float* scores, uint32_t* n_eligible, mfx_memspace space) {
    return guarded("mfx_rec_query_candidates", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->query_candidates(nusers, users, cand_ptr, cand_idx, flags, n_top, items, scores, n_eligible, space);
    });
}
int mfx_rec_score(mfx_rec_t r, int64_t npairs, const uint32_t* users, const uint32_t* items, float* scores, mfx_memspace space) {
    return guarded("mfx_rec_score", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->score(npairs, users, items, scores, space);
    });
}
int mfx_rec_ivf_setup(mfx_rec_t r, int32_t nlist, const uint32_t* assign, const float* centroids, mfx_memspace space) {
    return guarded("mfx_rec_ivf_setup", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->ivf_setup(nlist, assign, centroids, space);
    });
}
int mfx_rec_ivf_lists(mfx_rec_t r, uint32_t* list_ptr, uint32_t* list_idx, mfx_memspace space) {
    return guarded("mfx_rec_ivf_lists", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->ivf_lists(list_ptr, list_idx, space);
    });
}
int mfx_rec_ivf_probe(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t nprobe, uint32_t* lists, float* scores, mfx_memspace space) {
    return guarded("mfx_rec_ivf_probe", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->ivf_probe(nusers, users, nprobe, lists, scores, space);
    });
}
int mfx_rec_query_ivf(mfx_rec_t r, int64_t nusers, const uint32_t* users, int32_t nprobe, int32_t n_top, uint32_t* items, float* scores,
                      mfx_memspace space) {
    return guarded("mfx_rec_query_ivf", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->query_ivf(nusers, users, nprobe, n_top, items, scores, space);
    });
}
int mfx_rec_ivf_times(mfx_rec_t r, double seconds[4]) {
    return guarded("mfx_rec_ivf_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "null recommender or seconds");
        r->impl->ivf_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_candidates_times(mfx_rec_t r, double seconds[3]) {
    return guarded("mfx_rec_candidates_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "null recommender or seconds");
        r->impl->candidates_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_diversify(mfx_rec_t r, int64_t nusers, const uint32_t* users, const float* Wq, const uint32_t* cand_ptr,
                      const uint32_t* cand_idx, int32_t flags, int metric, float tradeoff, int32_t n_top, uint32_t* items, float* scores,
                      float* values, uint32_t* n_eligible, mfx_memspace space, int form) {
    return guarded("mfx_rec_diversify", [&]() -> int {
        MFX_REQUIRE(r && r->impl, "null recommender");
        return r->impl->diversify(nusers, users, Wq, cand_ptr, cand_idx, flags, metric, tradeoff, n_top, items, scores, values, n_eligible,
                                  space, form);
    });
}
int mfx_rec_diversify_times(mfx_rec_t r, double seconds[3]) {
    return guarded("mfx_rec_diversify_times", [&]() -> int {
        MFX_REQUIRE(r && r->impl && seconds, "null recommender or seconds");
        r->impl->diversify_times(seconds);
        return MFX_OK;
    });
}
int mfx_rec_destroy(mfx_rec_t r) {
    return guarded("mfx_rec_destroy", [&]() -> int {
        return destroy_handle(r);
    });
}
int mfx_topn_metrics(int64_t nusers, const uint32_t* users, int32_t n_top, const uint32_t* items, const mfx_coo* T,
                     float min_rating, double out[4], int64_t* users_evaluated) {
    return guarded("mfx_topn_metrics", [&]() -> int {
        return topn_metrics(nusers, users, n_top, items, T, min_rating, out, users_evaluated);
    });
}

/* ------------------------------------------------------------------ communicator */
int mfx_comm_unique_id(void* id_out) {
    return guarded("mfx_comm_unique_id", [&]() -> int {
        MFX_REQUIRE(id_out, "null id buffer");
        return comm_unique_id(id_out);
    });
}
int mfx_comm_create(mfx_comm_t* out, const void* id, int rank, int nranks, int device) {
    return guarded("mfx_comm_create", [&]() -> int {
        return comm_create(out, id, rank, nranks, device);
    });
}
int mfx_comm_create_local(mfx_comm_t* out, int group, int rank, int nranks, int device) {
    return guarded("mfx_comm_create_local", [&]() -> int {
        return comm_create_local(out, group, rank, nranks, device);
    });
}
int mfx_comm_agree(mfx_comm_t c, int local_status, int* global_status) {
    return guarded("mfx_comm_agree", [&]() -> int { return comm_agree(c, local_status, global_status); });
}
int mfx_comm_abort(mfx_comm_t c) {
    return guarded("mfx_comm_abort", [&]() -> int { return comm_abort(c); });
}
int mfx_comm_rank(mfx_comm_t c) { return c ? c->rank : -1; }
int mfx_comm_size(mfx_comm_t c) { return c ? c->nranks : 0; }
int mfx_comm_destroy(mfx_comm_t c) { return comm_destroy(c); }

/* ------------------------------------------------------------------ host-side helpers */
void mfx_initial_col(float* X, int64_t k, int64_t n) {
    srand(0L);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < k; ++j) X[j * n + i] = 0.1f * (float(rand()) / (float) RAND_MAX) + 0.001f;
}

int mfx_partition_rows(int64_t rows, const uint32_t* csr_row_ptr, int nshards, int64_t* bounds) {
    return guarded("mfx_partition_rows", [&]() -> int {
        MFX_REQUIRE(rows > 0 && csr_row_ptr && nshards >= 1 && bounds, "mfx_partition_rows: bad argument");
        const uint64_t nnz = csr_row_ptr[rows];
        bounds[0] = 0;
        for (int g = 1; g < nshards; ++g) {
            // first row whose prefix reaches g/nshards of the non-zeros
            const uint64_t target = (nnz * (uint64_t) g + nshards - 1) / (uint64_t) nshards;
            const uint32_t* it = std::lower_bound(csr_row_ptr, csr_row_ptr + rows + 1, (uint32_t) target);
            int64_t r = it - csr_row_ptr;
            if (r < bounds[g - 1]) r = bounds[g - 1];
            if (r > rows) r = rows;
            bounds[g] = r;
        }
        bounds[nshards] = rows;
        return MFX_OK;
    });
}

int mfx_extract_shard(const mfx_csx* R, int64_t row_lo, int64_t row_hi, uint32_t* l_csr_row_ptr,
                      uint32_t* l_csr_col_idx, float* l_csr_val, uint32_t* l_csc_col_ptr,
                      uint32_t* l_csc_row_idx, float* l_csc_val) {
    return guarded("mfx_extract_shard", [&]() -> int {
        MFX_REQUIRE(R && row_lo >= 0 && row_lo <= row_hi && row_hi <= R->rows, "mfx_extract_shard: bad row range");
        MFX_REQUIRE(l_csr_row_ptr && l_csc_col_ptr, "mfx_extract_shard: null output");
        const uint32_t base = R->csr_row_ptr[row_lo];
        const uint32_t lnnz = R->csr_row_ptr[row_hi] - base;
        for (int64_t r = row_lo; r <= row_hi; ++r) l_csr_row_ptr[r - row_lo] = R->csr_row_ptr[r] - base;
        if (lnnz) {
            memcpy(l_csr_col_idx, R->csr_col_idx + base, sizeof(uint32_t) * lnnz);
            memcpy(l_csr_val, R->csr_val + base, sizeof(float) * lnnz);
        }
        // local CSC: keep every column's entries whose row falls in the block, in R's column order
        uint32_t w = 0;
        for (int64_t c = 0; c < R->cols; ++c) {
            l_csc_col_ptr[c] = w;
            for (uint32_t p = R->csc_col_ptr[c]; p < R->csc_col_ptr[c + 1]; ++p) {
                const uint32_t r = R->csc_row_idx[p];
                if (r >= (uint32_t) row_lo && r < (uint32_t) row_hi) {
                    l_csc_row_idx[w] = r - (uint32_t) row_lo;
                    l_csc_val[w] = R->csc_val[p];
                    ++w;
                }
            }
        }
        l_csc_col_ptr[R->cols] = w;
        MFX_REQUIRE(w == lnnz, "CSR and CSC disagree on the shard's nnz (%u vs %u)", lnnz, w);
        return MFX_OK;
    });
}

}  // extern "C"
