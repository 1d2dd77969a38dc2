// als_solver.hip -- ALS kernels (gfx950) and their launches; the host orchestration is als_host.hip.
//
// Kernel shape.  One wavefront per work item; a work item is a whole segment, or a chunk of a long
// one (AlsHalf::build).  The gathered factor rows go straight from global memory into an MFMA
// operand layout -- no LDS staging, no cross-lane traffic:
//   * 32 < k <= 64, k % 4 == 0: k_als_gram16 -- v_mfma_f32_16x16x4_f32 on "column sets", rows fetched
//     with 16-byte loads, four whole rows per wave instruction (see the comment at the kernel);
//   * any other k <= 128: k_als_gram<NT> -- v_mfma_f32_32x32x2_f32, lane l supplies A[i = l&31][kk = l>>5]
//     and B[kk][j = l&31], so lane l loads X[row(q0 + (l>>5))][32*I + (l&31)]; the same register is
//     the A operand of tile (I, J) and the B operand of tile (J', I).
// Only the upper (block) triangle is accumulated.  fp32 MFMA is an exact k-ordered fmaf chain, so
// results are reproducible run to run.
//
// Tail (per segment, still one wave): accumulators -> LDS (lower triangle only, rows packed and
// 16-B aligned), + lambda on the diagonal (plain lambda, src/ALS.cpp:120-122), left-looking Cholesky
// (the reference's row-by-row scheme, src/ALS.cpp:6-23; dot products fused, one scale by 1/sqrt(pivot) per column),
// then L z = b and L^T y = z instead of the reference's explicit inverse (same solution up to
// rounding; tolerance in the tests).
#include "als_solver.hpp"

#include <type_traits>

// ---- The variant of this translation unit ------------------------------------------------------------------------
// This file is compiled eleven times: as itself (k_als_*) and through ten small files that set the macros below and include
// it.  A translation unit per family, so that the kernels of one compile to exactly the code they had without the others.
//   file                     macros                            kernels     what they solve
//   als_solver.hip           --                                k_als_*     explicit ALS, k <= 128
//   als_nreg.hip             MFX_ALS_NREG                      k_alsn_*    the same with fp32(lambda * n) on the diagonal of a segment of
//                                                                          n entries: the row minimiser of the CCD++ objective
//   ials_half.hip            MFX_ALS_IMPLICIT                  k_ials_*    implicit feedback, see "Implicit feedback" below
//   ials_reg_half.hip        MFX_ALS_IMPLICIT, MFX_ALS_REG     k_ialsr_*   implicit with an unobserved weight alpha0 and a regulariser per segment
//   ials_block_step.hip      MFX_ALS_BLOCK = 1                 k_ialsb_*   one block step of implicit ALS by block subspace sweeps (ials_block.hip)
//   ials_reg_block_step.hip  MFX_ALS_BLOCK = 1, MFX_ALS_REG    k_ialsrb_*  the block step of the alpha0 / regulariser objective
//   als_block_step.hip       MFX_ALS_BLOCK = 2                 k_alsb_*    one block step of EXPLICIT ALS by block sweeps (ials_block.hip, alsb_*)
//   als_mrhs.hip             MFX_ALS_MRHS                      k_alsm_*    k_als_*, then n_targets more right-hand sides per segment against
//                                                                          the segment's factor (mfx_rec_explain, "More right-hand sides" below)
//   als_nreg_mrhs.hip        MFX_ALS_NREG, MFX_ALS_MRHS        k_alsnm_*   k_alsn_* likewise
//   ials_half_mrhs.hip       MFX_ALS_IMPLICIT, MFX_ALS_MRHS    k_ialsm_*   k_ials_* likewise
//   ials_reg_half_mrhs.hip   MFX_ALS_IMPLICIT, _REG, _MRHS     k_ialsrm_*  k_ialsr_* likewise
// The macros are read in this header and nowhere else: it names the family, maps the macros onto constexpr traits and
// declares AlsArgs, whose conditional tail needs them (a field that a family does not have must not be declared: the
// kernel-argument layout of every family is part of what it compiles to).  The kernels below ask the traits; the entry
// points at the bottom of the file, one per family (the four *m_* families share one), ask ALS_FAMILY.
#ifndef MFX_ALS_BLOCK
#define MFX_ALS_BLOCK 0
#endif
#ifndef MFX_ALS_IMPLICIT
#define MFX_ALS_IMPLICIT (MFX_ALS_BLOCK == 1)
#endif
#ifndef MFX_ALS_NREG
#define MFX_ALS_NREG 0
#endif
#ifndef MFX_ALS_REG
#define MFX_ALS_REG 0
#endif
#ifndef MFX_ALS_MRHS
#define MFX_ALS_MRHS 0
#endif
#if MFX_ALS_REG && !MFX_ALS_IMPLICIT
#error "MFX_ALS_REG needs MFX_ALS_IMPLICIT or MFX_ALS_BLOCK = 1"
#endif
#if MFX_ALS_MRHS && MFX_ALS_BLOCK
#error "MFX_ALS_MRHS: a block step is not a solve of the segment's system"
#endif
// the family of this translation unit, and the prefix of its kernels' names
#define ALS_FAMILY_ALS 0
#define ALS_FAMILY_ALSN 1
#define ALS_FAMILY_IALS 2
#define ALS_FAMILY_IALSR 3
#define ALS_FAMILY_IALSB 4
#define ALS_FAMILY_IALSRB 5
#define ALS_FAMILY_ALSB 6
#define ALS_FAMILY_ALSM 7
#define ALS_FAMILY_ALSNM 8
#define ALS_FAMILY_IALSM 9
#define ALS_FAMILY_IALSRM 10
#if MFX_ALS_MRHS && MFX_ALS_REG
#define ALS_FAMILY ALS_FAMILY_IALSRM
#define ALS_KERNEL(name) k_ialsrm_##name
#elif MFX_ALS_MRHS && MFX_ALS_IMPLICIT
#define ALS_FAMILY ALS_FAMILY_IALSM
#define ALS_KERNEL(name) k_ialsm_##name
#elif MFX_ALS_MRHS && MFX_ALS_NREG
#define ALS_FAMILY ALS_FAMILY_ALSNM
#define ALS_KERNEL(name) k_alsnm_##name
#elif MFX_ALS_MRHS
#define ALS_FAMILY ALS_FAMILY_ALSM
#define ALS_KERNEL(name) k_alsm_##name
#elif MFX_ALS_BLOCK == 2
#define ALS_FAMILY ALS_FAMILY_ALSB
#define ALS_KERNEL(name) k_alsb_##name
#elif MFX_ALS_BLOCK && MFX_ALS_REG
#define ALS_FAMILY ALS_FAMILY_IALSRB
#define ALS_KERNEL(name) k_ialsrb_##name
#elif MFX_ALS_REG
#define ALS_FAMILY ALS_FAMILY_IALSR
#define ALS_KERNEL(name) k_ialsr_##name
#elif MFX_ALS_BLOCK
#define ALS_FAMILY ALS_FAMILY_IALSB
#define ALS_KERNEL(name) k_ialsb_##name
#elif MFX_ALS_IMPLICIT
#define ALS_FAMILY ALS_FAMILY_IALS
#define ALS_KERNEL(name) k_ials_##name
#elif MFX_ALS_NREG
#define ALS_FAMILY ALS_FAMILY_ALSN
#define ALS_KERNEL(name) k_alsn_##name
#else
#define ALS_FAMILY ALS_FAMILY_ALS
#define ALS_KERNEL(name) k_als_##name
#endif
// the entry point of a multi-right-hand-side family (als_solver.hpp)
#if ALS_FAMILY == ALS_FAMILY_IALSRM
#define ALS_MRHS_LAUNCH ialsr_half_mrhs_launch
#elif ALS_FAMILY == ALS_FAMILY_IALSM
#define ALS_MRHS_LAUNCH ials_half_mrhs_launch
#elif ALS_FAMILY == ALS_FAMILY_ALSNM
#define ALS_MRHS_LAUNCH als_half_nreg_mrhs_launch
#elif ALS_FAMILY == ALS_FAMILY_ALSM
#define ALS_MRHS_LAUNCH als_half_mrhs_launch
#endif

namespace mfx {
namespace {

// What goes on the diagonal of a segment's system
enum class Diag {
    kLambda,        // a.lambda
    kLambdaN,       // fp32(a.lambda * n) for a segment of n entries (a.seg_ptr)
    kLambdaNIfPtr,  // the second where a.seg_ptr is non-null, else the first
    kBase,          // nothing: an unsplit system / a reducer starts its accumulators from the base Gramian a.G = X^T X + lambda I
    kBaseRho,       // a.G is G0 = fp32(alpha0 X^T X) without lambda, and the start adds rho[seg] to its diagonal: add_rn(G0[c][c], rho[seg])
};
// Implicit weighting: a gathered entry r carries the Gramian weight w = fp32(a.alpha * r) and the rhs weight 1 + w
constexpr bool kImplicit = MFX_ALS_IMPLICIT != 0;
// Block step: the system of one block of d <= 128 coordinates.  a.k is d, a.X the block's column slice of X; an entry's rhs
// weight is taken at its stored score s (a.score: explicit r - s, implicit (1 + w) - w s), the rhs starts from -P[seg]
// (a.P: G[block, :] y, explicit rho y_block), and the solution written to Y is the step z = -Delta
constexpr bool kBlockStep = MFX_ALS_BLOCK != 0;
constexpr Diag kDiag = MFX_ALS_REG ? Diag::kBaseRho : kImplicit ? Diag::kBase : MFX_ALS_BLOCK == 2 ? Diag::kLambdaNIfPtr
                       : MFX_ALS_NREG ? Diag::kLambdaN : Diag::kLambda;
constexpr bool kBaseGramian = kDiag == Diag::kBase || kDiag == Diag::kBaseRho;
// Unobserved weight: alpha0 in the place of the 1 of the rhs weight (alpha0 + w; block step (alpha0 + w) - w s).  At alpha0 = 1
// and rho = lambda every operation of k_ialsr_* / k_ialsrb_* has the operands and the order of k_ials_* / k_ialsb_*
constexpr bool kAlpha0 = MFX_ALS_REG != 0;
static_assert(kAlpha0 == (kDiag == Diag::kBaseRho), "the unobserved weight and the regulariser per segment come together");
static_assert(kBaseGramian == kImplicit, "the implicit families, and only they, start from a base Gramian");
// More right-hand sides: after the system's own solve, n_targets more right-hand sides are solved against the same factor
// L -- rows of a.X gathered at a.targets[seg * n_targets + t], solution into a.Z[seg * n_targets + t] ("More right-hand
// sides" at factor_solve)
constexpr bool kMultiRhs = MFX_ALS_MRHS != 0;

// unfused multiply / subtract (HIP's __fmul_rn is a plain `*` and would be contracted into v_fma)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }  // v_pk_fma_f32

// 1 / x: v_rcp_f32 (1 ulp) + one Newton step
__device__ __forceinline__ float rcp_nr(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(r, __builtin_fmaf(-x, r, 1.0f), r);
}

struct AlsArgs {
    const AlsItem* items;
    const AlsReduce* reduces;
    uint32_t count;  // items (gram kernel) or reduces (reduce kernel)
    const uint32_t* idx;
    const float* val;
    const float* X;    // [x_rows + 1][k]: row x_rows is all zeros (gather target of positions past a segment's end)
    uint32_t x_rows;
    uint32_t sentinel;  // idx[sentinel] = x_rows, val[sentinel] = 0: what a position past a segment's end loads
    float* Y;
    uint32_t k;
    float lambda;
    float* ws;
    uint32_t* spd_fail;
    float* gram_out;  // != nullptr: dump the k x k Gramian (no lambda) of item 0 and stop
    unsigned long long* phases;  // != nullptr (MFX_ALS_PHASES=1): s_memtime clocks per phase, summed over the waves:
                                 // [0] Gramian loop, [1] staging into LDS, [2] factorisation, [3] triangular solves, [4] systems
    // implicit-feedback kernels only; appended so that the fields above keep their kernel-argument offsets
    float alpha;       // confidence weight of a gathered entry: w = fp32(alpha * r)
    const float* G;    // [k][k] base Gramian (ials_base_gramian), the start of every unsplit / reduced system
#if MFX_ALS_NREG || MFX_ALS_BLOCK == 2
    const uint32_t* seg_ptr;  // (k_alsn_*, k_alsb_* only) segment pointers [nseg + 1]: segment s has seg_ptr[s + 1] - seg_ptr[s] entries
#endif
#if MFX_ALS_BLOCK
    const float* score;  // (block steps only) [nnz + pad]: the score <x_j, y> of every stored pair, parallel to val
    const float* P;      // (block steps only) [nseg][k]: G[block, :] y of every segment (k_alsb_*: rho y_block)
#endif
#if MFX_ALS_REG
    float alpha0;      // (k_ialsr_*, k_ialsrb_* only) weight of the all-pairs term; G is fp32(alpha0 X^T X)
    const float* rho;  // (k_ialsr_*, k_ialsrb_* only) [nseg]: the regulariser of every segment (ialsr_rho_launch)
#endif
#if MFX_ALS_MRHS
    const uint32_t* targets;  // (k_*m_* only) [nseg][n_targets]: rows of X; an id >= x_rows (the padding 0xFFFFFFFF) reads the zero row
    uint32_t n_targets;
    float* Z;                 // (k_*m_* only) [nseg][n_targets][k]: zeroed by the caller (an empty segment writes nothing)
#endif
};
// The fields of the conditional tail, readable in every family (null / 1 where the family has none)
__device__ __forceinline__ const uint32_t* arg_seg_ptr(const AlsArgs& a) {
#if MFX_ALS_NREG || MFX_ALS_BLOCK == 2
    return a.seg_ptr;
#else
    return nullptr;
#endif
}
__device__ __forceinline__ const float* arg_score(const AlsArgs& a) {
#if MFX_ALS_BLOCK
    return a.score;
#else
    return nullptr;
#endif
}
__device__ __forceinline__ const float* arg_P(const AlsArgs& a) {
#if MFX_ALS_BLOCK
    return a.P;
#else
    return nullptr;
#endif
}
__device__ __forceinline__ float arg_alpha0(const AlsArgs& a) {
#if MFX_ALS_REG
    return a.alpha0;
#else
    return 1.0f;
#endif
}
__device__ __forceinline__ const float* arg_rho(const AlsArgs& a) {
#if MFX_ALS_REG
    return a.rho;
#else
    return nullptr;
#endif
}
__device__ __forceinline__ const uint32_t* arg_targets(const AlsArgs& a) {
#if MFX_ALS_MRHS
    return a.targets;
#else
    return nullptr;
#endif
}
__device__ __forceinline__ uint32_t arg_n_targets(const AlsArgs& a) {
#if MFX_ALS_MRHS
    return a.n_targets;
#else
    return 0;
#endif
}
__device__ __forceinline__ float* arg_Z(const AlsArgs& a) {
#if MFX_ALS_MRHS
    return a.Z;
#else
    return nullptr;
#endif
}
// ---- end of the variant header: no MFX_ALS_* macro from here to the entry points ------------------------------------

// The stored score of a gathered entry out of the register that holds it in a block step; 0, and the register unread (it is
// never written either), in every other family
__device__ __forceinline__ float score_of(const float& s) {
    if constexpr (kBlockStep) return s;
    else return 0.f;
}
// rhs weight of a gathered entry in the explicit kernels: its value r, or r - s at its stored score s in a block step
__device__ __forceinline__ float als_rhs(float r, float s) {
    if constexpr (kBlockStep) return sub_rn(r, s);
    else return r;
}
// lambda of segment `seg` on the diagonal of its system (0 from the launches of the base-Gramian families), one rounding
__device__ __forceinline__ float diag_lambda(const AlsArgs& a, uint32_t seg) {
    const uint32_t* sp = arg_seg_ptr(a);
    if constexpr (kDiag == Diag::kLambdaN) return mul_rn(a.lambda, (float) (sp[seg + 1] - sp[seg]));
    if constexpr (kDiag == Diag::kLambdaNIfPtr)
        if (sp) return mul_rn(a.lambda, (float) (sp[seg + 1] - sp[seg]));  // (wave-uniform)
    return a.lambda;
}
// rho of a work item's segment (Diag::kBaseRho; else 0, unused): the segment is the same in every lane, so one scalar load
__device__ __forceinline__ float seg_rho(const AlsArgs& a, uint32_t seg) {
    if constexpr (kDiag == Diag::kBaseRho) return arg_rho(a)[__builtin_amdgcn_readfirstlane((int) seg)];
    else return 0.f;
}
__device__ __forceinline__ void phase_mark(const AlsArgs& a, int slot, unsigned long long& t) {
    if (a.phases && t) {  // (t == 0: a caller that does not take part, e.g. the reducers of split segments)
        const unsigned long long now = __builtin_readcyclecounter();
        if ((threadIdx.x & 63) == 0) atomicAdd(a.phases + (blockIdx.x % kPhaseCopies) * 8 + slot, now - t);  // (spread: 480 k waves on one line serialise)
        t = now;
    }
}

template <int NT> struct Tiles { static constexpr int kCount = NT * (NT + 1) / 2; };

template <int NT>
__device__ __forceinline__ size_t slot_floats() { return (size_t) Tiles<NT>::kCount * 1024 + (size_t) NT * 64; }

// LDS image of one system: the lower triangle only, rows packed back to back with every row start
// rounded up to 4 floats (16-B aligned for ds_read_b128): 8.7 KB for k = 64 instead of 17.4 KB for
// the square, which is what lets 16 instead of 9 single-wave workgroups share a CU.  The rhs follows.
constexpr int roff_host(int r) { return 4 * ((r >> 2) + 1) * (2 * (r >> 2) + (r & 3)); }
__device__ __forceinline__ int roff(int r) { const int g = r >> 2, m = r & 3; return 4 * (g + 1) * (2 * g + m); }

// 32x32x2 accumulators (upper block triangle) + rhs -> LDS image.
template <int NT>
__device__ __forceinline__ void stage_tiles32(f32x16 (&acc)[Tiles<NT>::kCount], float (&bacc)[NT], float* lds) {
    constexpr int KP = 32 * NT;
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    float* L = lds;
    float* bv = lds + roff(KP);
    int ti = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I) {
#pragma unroll
        for (int J = I; J < NT; ++J, ++ti) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = I * 32 + (r & 3) + 8 * (r >> 2) + 4 * (int) h;
                const int col = J * 32 + (int) c31;
                const float x = acc[ti][r];
                if (row >= col) L[roff(row) + col] = x;  // diagonal tiles hold both (r,c) and (c,r): same value
                else L[roff(col) + row] = x;
            }
        }
    }
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        const float t = bacc[I] + __shfl_xor(bacc[I], 32, 64);
        if (h == 0) bv[I * 32 + c31] = t;
    }
}


// ---- Blocked Cholesky on the matrix cores, for KP = 32 * NT with NT >= 2 -----------------------------------
// The packed lower-triangular LDS image is factored block column by block column (32 x 32 blocks):
//   update   T_IJ = A_IJ - sum_{K<J} L_IK L_JK^T   v_mfma_f32_32x32x2_f32: lane (r, h) feeds row r of both blocks,
//            four consecutive columns per ds_read_b128 (columns 8t+4h+e in MFMA step 4t+e: the two halves of the
//            wave cover the K dimension between them)
//   panel    columns of block column J, one at a time, for 64 rows per pass: every lane keeps its row of the
//            panel in registers (the k <= 64 scheme: pivot row by LDS broadcast, packed fp32 math) and computes
//            L[row][i] = (T[row][i] - sum_{q<i} L[i][q] L[row][q]) / p_i.  First pass: lanes 0..31 hold the
//            diagonal block (they produce the pivots), lanes 32..63 the block below it -- its triangular solve
//            is the very same update (chol_diag_pass_rl, right-looking); further passes take two more blocks each, with
//            the pivots read back (chol_panel_pass).
// Against the row-by-row form of round 1 (one row at a time, a barrier per row) this takes the O(k^3) part off the
// VALU / LDS path (which bounded k > 64: every product needed two LDS rows, 200 ms per iteration at k = 128).  Rows /
// columns k .. KP-1 of the image are an identity block (set by the caller).
__device__ __forceinline__ void chol_panel_pass(float* __restrict__ L, int J, int blk_lo, int blk_hi) {
    const int lane = (int) (threadIdx.x & 63), r31 = lane & 31, h = lane >> 5;
    const bool stores = h == 0 || blk_hi >= 0;                    // lanes 32..63 without a block of their own shadow blk_lo
    const int row = ((h && blk_hi >= 0) ? blk_hi : blk_lo) * 32 + r31;
    float* blk = L + roff(row) + J * 32;
    f32x2 r2[16];
#pragma unroll
    for (int q = 0; q < 32; q += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(blk + q);
        r2[q / 2] = x.lo;
        r2[q / 2 + 1] = x.hi;
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float* pivrow = L + roff(J * 32 + i) + J * 32;  // row i of L_JJ: the same address in every lane
        f32x2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q + 4 <= i; q += 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(pivrow + q);
            s01 = fma2(x.lo, r2[q / 2], s01);
            s23 = fma2(x.hi, r2[q / 2 + 1], s23);
        }
#pragma unroll
        for (int q = i & ~3; q < i; ++q) s01.x = __builtin_fmaf(pivrow[q], r2[q / 2][q & 1], s01.x);
        const f32x2 s4 = s01 + s23;  // one v_pk_add_f32, then the two halves
        const float sum = r2[i / 2][i & 1] - (s4.x + s4.y);
        const float lji = sum * __builtin_amdgcn_rcpf(pivrow[i]);  // (1 ulp, like the rsq of the diagonal pass)
        if (stores) blk[i] = lji;
        r2[i / 2][i & 1] = lji;
    }
}

// (r3) The diagonal pass RIGHT-LOOKING and entirely in registers.  In the left-looking form of the passes below it, step i
// would read row i of the diagonal block from LDS -- a row whose entries the previous steps have only just written there: an
// LDS write -> read round trip inside every one of the 32 dependent steps of a pass, with one wave per SIMD and nothing to
// hide it behind.  Here every lane keeps its row of the block column in registers, and once column i is scaled its rank-one
// update is applied to the columns still to come, a_c -= l_i * L[c][i], with L[c][i] taken from lane c by v_readlane:
// 496 readlane + fma pairs per pass instead of 120 ds_read_b128 and 260 v_pk_fma, but the dependent chain of a step is
// readlane(pivot) -> rsq -> scale -> readlane -> fma (~50 clocks) and the LDS only sees the 32 column stores.  Lanes
// 32..63 (the block below the diagonal one) run the very same updates on their rows.
__device__ __forceinline__ void chol_diag_pass_rl(float* __restrict__ L, int J, int blk_hi, bool& spd_ok) {
    const int lane = (int) (threadIdx.x & 63), r31 = lane & 31, h = lane >> 5;
    const bool stores = h == 0 || blk_hi >= 0;                    // lanes 32..63 without a block of their own shadow the diagonal block
    const int row = ((h && blk_hi >= 0) ? blk_hi : J) * 32 + r31;
    float* blk = L + roff(row) + J * 32;
    f32x2 a2[16];  // columns (2 q, 2 q + 1) of the lane's row: the rank-one updates run as v_pk_fma_f32 on aligned pairs
#pragma unroll
    for (int q = 0; q < 32; q += 4) {  // (diagonal block: reads past the diagonal stay inside the image, never used)
        const f32x4 x = *reinterpret_cast<const f32x4*>(blk + q);
        a2[q / 2] = x.lo;
        a2[q / 2 + 1] = x.hi;
    }
    auto rl = [](float x, int src_lane) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
    };
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const float piv = rl(a2[i / 2][i & 1], i);  // lane i < 32 owns the diagonal entry, all earlier rank-one updates applied
        spd_ok = spd_ok && piv > 0.f;
        const float l = a2[i / 2][i & 1] * __builtin_amdgcn_rsqf(piv);  // lane i: pivot / sqrt(pivot) = the diagonal entry
        if (stores && (h || lane >= i)) blk[i] = l;
        const f32x2 nl = {-l, -l};
        if ((i & 1) == 0) a2[i / 2][1] = __builtin_fmaf(-l, rl(l, i + 1), a2[i / 2][1]);  // the odd partner of an even column
#pragma unroll
        for (int c = (i | 1) + 1; c < 32; c += 2)  // (rows above the diagonal: slots they never store)
            a2[c / 2] = fma2(nl, f32x2{rl(l, c), rl(l, c + 1)}, a2[c / 2]);
    }
}

template <int NT>
__device__ void chol_blocked(float* __restrict__ L, bool& spd_ok, const AlsArgs& a) {
    const int lane = (int) (threadIdx.x & 63), r31 = lane & 31, h = lane >> 5;
    unsigned long long tsub = a.phases ? __builtin_readcyclecounter() : 0ull;  // [5] MFMA updates, [6] diagonal passes, [7] passes below
#pragma unroll 1
    for (int J = 0; J < NT; ++J) {
        if (J > 0) {
#pragma unroll 1
            for (int I = J; I < NT; ++I) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                const float* rowI = L + roff(I * 32 + r31) + 4 * h;
                const float* rowJ = L + roff(J * 32 + r31) + 4 * h;
#pragma unroll 1
                for (int K = 0; K < J; ++K) {
                    // all eight operand reads of the K-block go out before its first MFMA: one LDS latency per block
                    // instead of four (the wave is alone on its SIMD: nothing else hides them)
                    f32x4 av[4], bv[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        av[t] = *reinterpret_cast<const f32x4*>(rowI + K * 32 + 8 * t);
                        bv[t] = *reinterpret_cast<const f32x4*>(rowJ + K * 32 + 8 * t);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][e], bv[t][e], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // accumulator register r of lane l: row (r&3) + 8 (r>>2) + 4 h, column r31
                    const int row = I * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, col = J * 32 + r31;
                    if (row >= col) L[roff(row) + col] = sub_rn(L[roff(row) + col], acc[r]);
                }
            }
            __syncthreads();
            phase_mark(a, 5, tsub);
        }
        chol_diag_pass_rl(L, J, J + 1 < NT ? J + 1 : -1, spd_ok);
        __syncthreads();
        phase_mark(a, 6, tsub);
#pragma unroll 1
        for (int I0 = J + 2; I0 < NT; I0 += 2) chol_panel_pass(L, J, I0, I0 + 1 < NT ? I0 + 1 : -1);
        __syncthreads();
        phase_mark(a, 7, tsub);
    }
}

// (r3) Triangular solves for 64 < k <= 128 in 32-column blocks, every operand of the 2 x KP dependent steps in
// registers.  The row-by-row form of round 1 read L[lane][i] (forward) / L[i][lane] (backward) from LDS inside each step:
// with one or two waves per SIMD nothing hides that read, and MFX_ALS_PHASES measured 90 000 clocks per system for the
// solves at k = 128 -- more than the Gramian (85 000) or the factorisation (81 000).  Here a block's operands are
// loaded up front -- forward: 32 consecutive entries of the lane's own rows (b128 reads); backward: element `lane` of 32
// consecutive rows (lane-contiguous, conflict-free) -- and a step is scale, v_readlane, masked fma on the UNSCALED
// unknowns (lane i carries z_i * L[i][i] until the end, as in the k <= 64 path).  Lane l owns rows l and l + 64; rows
// k .. KP-1 are identity rows with a zero right-hand side, so no step needs a bound on k.
// (kMultiRhs) The two passes of solve_blocked below on one more right-hand side, operation for operation: lane l comes in with
// entries l and l + 64 of the rhs in z0 / z1 and leaves with those of the solution.  rp0 / rp1: 1 / L[l][l], 1 / L[r1][r1];
// lanef: the lane as an opaque float.  (Why the system's own solve is not routed through it: see solve_regs_rhs.  A change
// to either copy goes into the other.)
template <int NT>
__device__ __forceinline__ void solve_blocked_rhs(const float* __restrict__ L, float& z0, float& z1, float rp0, float rp1, float lanef,
                                                  int lane, int r1) {
    auto rl = [](float x, int src_lane) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
    };
    // ---- forward: L z = b
#pragma unroll
    for (int B = 0; B < NT; ++B) {
        float a0[32], a1[32];
#pragma unroll
        for (int q = 0; q < 32; q += 4) {  // entries past a row's diagonal: inside the image, masked below
            const f32x4 x = *reinterpret_cast<const f32x4*>(L + roff(lane) + 32 * B + q);
            const f32x4 y = *reinterpret_cast<const f32x4*>(L + roff(r1) + 32 * B + q);
            a0[q] = x[0]; a0[q + 1] = x[1]; a0[q + 2] = x[2]; a0[q + 3] = x[3];
            a1[q] = y[0]; a1[q + 1] = y[1]; a1[q + 2] = y[2]; a1[q + 3] = y[3];
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int i = 32 * B + t;
            if (i < 64) {
                const float zi = rl(z0 * rp0, i);
                z0 = lanef > (float) i ? __builtin_fmaf(-a0[t], zi, z0) : z0;
                z1 = __builtin_fmaf(-a1[t], zi, z1);                      // rows 64 .. are all below row i
            } else {
                const float zi = rl(z1 * rp1, i - 64);
                z1 = lanef > (float) (i - 64) ? __builtin_fmaf(-a1[t], zi, z1) : z1;
            }
        }
    }
    z0 *= rp0;
    z1 *= rp1;
    // ---- backward: L^T y = z
#pragma unroll
    for (int B = NT - 1; B >= 0; --B) {
        float a0[32], a1[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) {  // element `lane` (and lane + 64) of rows 32 B + t: contiguous over the lanes
            const float* row = L + roff(32 * B + t);
            a0[t] = row[lane];
            a1[t] = row[r1];
        }
#pragma unroll
        for (int t = 31; t >= 0; --t) {
            const int i = 32 * B + t;
            if (i >= 64) {
                const float yi = rl(z1 * rp1, i - 64);
                z1 = lanef < (float) (i - 64) ? __builtin_fmaf(-a1[t], yi, z1) : z1;
                z0 = __builtin_fmaf(-a0[t], yi, z0);                      // rows 0 .. 63 are all above row i
            } else {
                const float yi = rl(z0 * rp0, i);
                z0 = lanef < (float) i ? __builtin_fmaf(-a0[t], yi, z0) : z0;
            }
        }
    }
    z0 *= rp0;
    z1 *= rp1;
}

template <int NT>
__device__ __forceinline__ void solve_blocked(const float* __restrict__ L, const float* __restrict__ bv, const AlsArgs& a, uint32_t seg, int k) {
    constexpr int KP = 32 * NT;
    const int lane = (int) (threadIdx.x & 63);
    const bool has1 = lane + 64 < KP;                 // (KP = 96: lanes 32..63 own no second row)
    const int r1 = has1 ? lane + 64 : KP - 1;         // ... they shadow the last row and never store
    float z0 = lane < k ? bv[lane] : 0.f;
    float z1 = (has1 && lane + 64 < k) ? bv[lane + 64] : 0.f;
    const float rp0 = rcp_nr(L[roff(lane) + lane]);
    const float rp1 = rcp_nr(L[roff(r1) + r1]);
    float lanef = (float) lane;
    asm volatile("" : "+v"(lanef));  // (opaque: keeps the masks float compares, see factor_solve k <= 64)
    // (solve_blocked_rhs above restates the two passes below for the further right-hand sides of kMultiRhs: change both together)
    auto rl = [](float x, int src_lane) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
    };
    // ---- forward: L z = b
#pragma unroll
    for (int B = 0; B < NT; ++B) {
        float a0[32], a1[32];
#pragma unroll
        for (int q = 0; q < 32; q += 4) {  // entries past a row's diagonal: inside the image, masked below
            const f32x4 x = *reinterpret_cast<const f32x4*>(L + roff(lane) + 32 * B + q);
            const f32x4 y = *reinterpret_cast<const f32x4*>(L + roff(r1) + 32 * B + q);
            a0[q] = x[0]; a0[q + 1] = x[1]; a0[q + 2] = x[2]; a0[q + 3] = x[3];
            a1[q] = y[0]; a1[q + 1] = y[1]; a1[q + 2] = y[2]; a1[q + 3] = y[3];
        }
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            const int i = 32 * B + t;
            if (i < 64) {
                const float zi = rl(z0 * rp0, i);
                z0 = lanef > (float) i ? __builtin_fmaf(-a0[t], zi, z0) : z0;
                z1 = __builtin_fmaf(-a1[t], zi, z1);                      // rows 64 .. are all below row i
            } else {
                const float zi = rl(z1 * rp1, i - 64);
                z1 = lanef > (float) (i - 64) ? __builtin_fmaf(-a1[t], zi, z1) : z1;
            }
        }
    }
    z0 *= rp0;
    z1 *= rp1;
    // ---- backward: L^T y = z
#pragma unroll
    for (int B = NT - 1; B >= 0; --B) {
        float a0[32], a1[32];
#pragma unroll
        for (int t = 0; t < 32; ++t) {  // element `lane` (and lane + 64) of rows 32 B + t: contiguous over the lanes
            const float* row = L + roff(32 * B + t);
            a0[t] = row[lane];
            a1[t] = row[r1];
        }
#pragma unroll
        for (int t = 31; t >= 0; --t) {
            const int i = 32 * B + t;
            if (i >= 64) {
                const float yi = rl(z1 * rp1, i - 64);
                z1 = lanef < (float) (i - 64) ? __builtin_fmaf(-a1[t], yi, z1) : z1;
                z0 = __builtin_fmaf(-a0[t], yi, z0);                      // rows 0 .. 63 are all above row i
            } else {
                const float yi = rl(z0 * rp0, i);
                z0 = lanef < (float) i ? __builtin_fmaf(-a0[t], yi, z0) : z0;
            }
        }
    }
    z0 *= rp0;
    z1 *= rp1;
    float* y = a.Y + (size_t) seg * k;
    if (lane < k) y[lane] = z0;
    if (has1 && lane + 64 < k) y[lane + 64] = z1;
    if constexpr (kMultiRhs) {  // More right-hand sides (see factor_solve): the two passes again per target
        const uint32_t nt = arg_n_targets(a);
#pragma unroll 1
        for (uint32_t t = 0; t < nt; ++t) {
            const size_t zt = (size_t) seg * nt + t;
            const uint32_t tg = arg_targets(a)[zt];
            const float* x = a.X + (size_t) (tg < a.x_rows ? tg : a.x_rows) * k;
            z0 = lane < k ? x[lane] : 0.f;
            z1 = (has1 && lane + 64 < k) ? x[lane + 64] : 0.f;
            solve_blocked_rhs<NT>(L, z0, z1, rp0, rp1, lanef, lane, r1);
            float* z = arg_Z(a) + zt * k;
            if (lane < k) z[lane] = z0;
            if (has1 && lane + 64 < k) z[lane + 64] = z1;
        }
    }
}

// (kMultiRhs) The triangular solves of the k <= 64 path on one more right-hand side: the two loops of factor_solve, operation
// for operation (see the comment there; a change to either copy goes into the other).  Lane i comes in with entry i of the rhs in z and leaves with that of the solution;
// r2: the lane's row of L, in registers.  The system's own solve stays written out in factor_solve: routed through this
// function it is the same arithmetic, but the kernels of the families without more right-hand sides then come out with another
// register allocation (SGPR spills move), and they are to compile to the code they had.
template <int KP>
__device__ __forceinline__ void solve_regs_rhs(const f32x2 (&r2)[KP / 2], const float* __restrict__ L, int k, float rp, float lanef, int lane,
                                               float& z) {
    auto rl = [](float x, int src_lane) {
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
    };
#pragma unroll
    for (int i = 0; i < KP; ++i) {  // forward: L z = b
        if (i < k) {
            const float zi = rl(z * rp, i);
            z = lanef > (float) i ? __builtin_fmaf(-r2[i / 2][i & 1], zi, z) : z;
        }
    }
    z *= rp;  // = the solution of L z = b; the backward pass carries y_i * L[i][i] the same way
#pragma unroll
    for (int i = KP - 1; i >= 0; --i) {  // backward: L^T y = z
        if (i < k) {
            const float yi = rl(z * rp, i);
            const float lij = L[roff(i) + lane];  // lanes >= i read past the row's diagonal: masked below
            z = lanef < (float) i ? __builtin_fmaf(-lij, yi, z) : z;
        }
    }
    z *= rp;
}

// LDS image -> + lambda, Cholesky, two triangular solves, Y[seg] <- solution.
// FULL: k == KP known at compile time (k = 64: no per-column `i < k` branches, no `lane < k` masks; user half at the
// Netflix shape 8.24 -> 7.89 ms)
template <int NT, bool FULL = false>
__device__ void factor_solve(float* lds, const AlsArgs& a, uint32_t seg, unsigned long long tmark = 0) {
    constexpr int KP = 32 * NT;
    const uint32_t lane = threadIdx.x & 63;
    const int k = FULL ? KP : (int) a.k;
    float* L = lds;
    float* bv = lds + roff(KP);
    __syncthreads();
    if (a.gram_out) {
        for (int e = (int) lane; e < k * k; e += 64) {
            int r = e / k, c = e % k;
            if (FULL) { r = 16 * (r & 3) + (r >> 2); c = 16 * (c & 3) + (c >> 2); }  // the permuted image of stage_tiles16_perm
            a.gram_out[e] = r >= c ? L[roff(r) + c] : L[roff(c) + r];
        }
        return;
    }
    const float lam = diag_lambda(a, seg);
    for (int i = (int) lane; i < KP; i += 64) L[roff(i) + i] = i < k ? add_rn(L[roff(i) + i], lam) : 1.0f;  // rows k.. : identity
    if constexpr (kBlockStep) {
        // rhs = sum_j ((1 + w_j) - w_j s_j) x_j - P[seg]; FULL: position i of the permuted image is column 4 (i & 15) + (i >> 4)
        const float* P = arg_P(a);
        for (int i = (int) lane; i < k; i += 64) bv[i] = sub_rn(bv[i], P[(size_t) seg * k + (FULL ? 4 * (i & 15) + (i >> 4) : i)]);
    }
    __syncthreads();

    // Left-looking Cholesky on the lower triangle, row i at a time (the reference's choldc1 loop,
    // src/ALS.cpp:6-23):  sum = A[i][j] - sum_q L[i][q] * L[j][q];  j == i: p = sqrt(sum);  else
    // L[j][i] = sum / p.  The dot product over q runs in four independent partial sums (the
    // reference's single accumulator would be a 64-deep dependent chain per row).  Both forms use fused multiply-adds and
    // one 1/sqrt(pivot) scale per column.
    phase_mark(a, 1, tmark);  // staging (+ lambda, barriers)
    if constexpr (NT >= 3) {  // k > 64: blocked (measured at k = 64: 16.9 ms per iteration blocked vs 15.9 in registers)
        bool spd_ok = true;
        chol_blocked<NT>(L, spd_ok, a);
        if (lane == 0 && !spd_ok) atomicAdd(a.spd_fail, 1u);
        phase_mark(a, 2, tmark);
        __syncthreads();
        solve_blocked<NT>(L, bv, a, seg, k);
        phase_mark(a, 3, tmark);
    } else {
        // k <= 64: lane j keeps its own row j in registers (static indices after full unrolling), so
        // only row i -- the same for every lane -- is read from LDS, as broadcast ds_read_b128 of
        // whole 4-column groups; the up to three columns past the last whole group come from lane
        // i's registers by v_readlane.  Each finished column goes back to LDS with one ds_write_b32,
        // so later rows find it there and the image is complete for the triangular solves.  Against
        // reading both rows from LDS this halves the LDS traffic (which bounded the user half-sweep,
        // 480 k systems) and drops the per-lane address arithmetic.
        // Register pairs and explicit 2-wide fused products: v_pk_fma_f32 on naturally aligned pairs (left to
        // itself the SLP vectoriser pairs non-adjacent columns and pays for it in v_mov).
        f32x2 r2[KP / 2];
        const int row = (int) lane < KP ? (int) lane : KP - 1;  // KP = 32: the upper half-wave mirrors row 31, never stores
#pragma unroll
        for (int q = 0; q < KP; q += 4) {  // reads past the end of a short row stay inside L; those slots are never used
            const f32x4 x = *reinterpret_cast<const f32x4*>(&L[roff(row) + q]);
            r2[q / 2] = x.lo;
            r2[q / 2 + 1] = x.hi;
        }
        auto rl = [](float x, int src_lane) {
            return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src_lane));
        };
        // Per column i: dot products as v_pk_fma_f32 (two columns per instruction, fused: one rounding less than the
        // reference's multiply-then-add), then ONE scale for the whole column: L[j][i] = sum_j * rs with
        // rs = 1/sqrt(pivot) (v_rsq_f32 + a Newton step, computed redundantly by every lane from the broadcast pivot).
        // Lane i's own product pivot * rs is the diagonal entry sqrt(pivot) to within an ulp, so there is no select
        // between "diagonal" and "below", no correctly rounded sqrt and no IEEE division in the loop (they were 21 of
        // the ~45 VALU instructions of a step; the solves below take 1 / L[i][i] once, in parallel).
#pragma unroll
        for (int i = 0; i < KP; ++i) {
            if (i < k) {  // wave-uniform
                f32x2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q + 4 <= i; q += 4) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(&L[roff(i) + q]);
                    s01 = fma2(x.lo, r2[q / 2], s01);
                    s23 = fma2(x.hi, r2[q / 2 + 1], s23);
                }
#pragma unroll
                for (int q = i & ~3; q < i; ++q) s01.x = __builtin_fmaf(rl(r2[q / 2][q & 1], i), r2[q / 2][q & 1], s01.x);
                const f32x2 s4 = s01 + s23;  // one v_pk_add_f32, then the two halves
        const float sum = r2[i / 2][i & 1] - (s4.x + s4.y);
                const float piv = rl(sum, i);
                // v_rsq_f32 as it comes (1 ulp): a column of L scaled by (1 + 1e-7) perturbs L L^T like one more fp32
                // rounding of A's entries; a Newton step here costs four more VALU instructions per column
                const float lji = sum * __builtin_amdgcn_rsqf(piv);
                r2[i / 2][i & 1] = lji;  // lanes j < i: a register slot (column i > j) they never read
                if ((int) lane >= i && (int) lane < KP) L[roff((int) lane) + i] = lji;
            }
        }
        __syncthreads();
        phase_mark(a, 2, tmark);
        // Triangular solves on the UNSCALED unknowns: lane i carries z_i * L[i][i] until the very end, so a step is
        // scale (one multiply for all lanes), broadcast (v_readlane), update (one masked fma) -- no per-step select of
        // the finished component.  The forward pass takes L[lane][i] from the lane's registers, the backward pass reads
        // row i of L from LDS at a compile-time offset (lane-strided, conflict-free).  Rows k .. KP-1 are identity rows
        // with a zero rhs: their updates add exact zeros.
        // (the lane masks of the solves are FLOAT compares on purpose: as integer compares they are the store masks
        // of the factorisation loop above, get computed there, and 128 of them are kept alive across it in VGPR lanes)
        // (solve_regs_rhs restates the two loops below for the further right-hand sides of kMultiRhs: change both together)
        float z = lane < (uint32_t) k ? bv[lane] : 0.f;
        const float rp = lane < (uint32_t) k ? rcp_nr(L[roff((int) lane) + lane]) : 0.f;
        float lanef = (float) lane;
        asm volatile("" : "+v"(lanef));  // (opaque: otherwise the compare is folded back to the integer one)
#pragma unroll
        for (int i = 0; i < KP; ++i) {  // forward: L z = b
            if (i < k) {
                const float zi = rl(z * rp, i);
                z = lanef > (float) i ? __builtin_fmaf(-r2[i / 2][i & 1], zi, z) : z;
            }
        }
        z *= rp;  // = the solution of L z = b; the backward pass carries y_i * L[i][i] the same way
#pragma unroll
        for (int i = KP - 1; i >= 0; --i) {  // backward: L^T y = z
            if (i < k) {
                const float yi = rl(z * rp, i);
                const float lij = L[roff(i) + (int) lane];  // lanes >= i read past the row's diagonal: masked below
                z = lanef < (float) i ? __builtin_fmaf(-lij, yi, z) : z;
            }
        }
        z *= rp;
        // FULL: the system was factored under the column permutation of stage_tiles16_perm (unknown 16 e + c is column 4 c + e)
        if ((int) lane < k) a.Y[(size_t) seg * k + (FULL ? 4 * (lane & 15) + (lane >> 4) : lane)] = z;
        // "a is not positive definite" (src/ALS.cpp:12): a pivot <= 0 or NaN makes its rsq inf / NaN, which reaches every
        // later column and the solution -- one test of the result instead of one compare per pivot; one count per system
        // (the k > 64 form counts pivots)
        const bool broken = (int) lane < k && !(__builtin_fabsf(z) <= 3.0e38f);
        if (__ballot(broken) != 0 && lane == 0) atomicAdd(a.spd_fail, 1u);
        phase_mark(a, 3, tmark);
        // More right-hand sides: z_t = A^-1 x_target for every target of the segment, against the rows of L that the
        // factorisation left in r2[] -- one more pair of passes each (solve_regs_rhs: the two loops above, restated), no
        // reload.  A target past x_rows (the padding id) is the all-zero row: its passes run on zeros.  FULL: position `lane`
        // of the permuted system is column `col` of the row.
        if constexpr (kMultiRhs) {
            const uint32_t nt = arg_n_targets(a);
            const uint32_t col = FULL ? 4 * (lane & 15) + (lane >> 4) : lane;
#pragma unroll 1
            for (uint32_t t = 0; t < nt; ++t) {
                const size_t zt = (size_t) seg * nt + t;
                const uint32_t tg = arg_targets(a)[zt];
                float zz = (int) lane < k ? a.X[(size_t) (tg < a.x_rows ? tg : a.x_rows) * k + col] : 0.f;
                solve_regs_rhs<KP>(r2, L, k, rp, lanef, (int) lane, zz);
                if ((int) lane < k) arg_Z(a)[zt * k + col] = zz;
            }
        }
    }
}

// ---- Implicit feedback (Hu, Koren, Volinsky 2008) --------------------------------------------------------------
// The k_ials_* kernels (kImplicit, ials_half.hip) are the kernels below: every gathered entry r carries the Gramian weight
// w = fp32(alpha r) and the rhs weight 1 + w (0 when r = 0: an explicit zero is no entry), and an unsplit system / a
// reducer starts its accumulators from the base Gramian G = X^T X + lambda I instead of zero (the launches pass
// lambda = 0, so factor_solve adds nothing more to the diagonal).  A system is then
//   (X^T X + lambda I + sum_j w_j x_j x_j^T) y = sum_{j, r_j > 0} (1 + w_j) x_j.
// How the weight reaches the MFMA (the same register is the A and the B operand of the unweighted Gramian): a scaled copy
// w x is the A operand.  The other form, scaling the row IN PLACE by sqrt(w) after its rhs update (no register more, one
// rounding more), was measured at the Netflix shape (tools/ials_bench.py, one MI355X, same box and call,
// profiles/r06_ials_bench*.json): copy 13.22 / 66.4 ms per iteration at k = 64 / 128, sqrt 14.02 / 70.4 ms -- the copy costs
// no spills where it matters (k_ials_gram16: 128 VGPRs, 20-24 bytes of scratch in both forms) and saves the v_sqrt and the
// multiplies that wait on it.
// (a diagonal tile holds sum fl(w x_i) x_j and sum fl(w x_j) x_i, equal up to rounding; the staging keeps one.)

// r -> (rhs weight, Gramian operand scale) = (a0 + w or 0, w); a0 is 1 (arg_alpha0) but for kAlpha0; block step: at the
// entry's stored score s
__device__ __forceinline__ void ials_weights(float r, float alpha, float& rhs, float& scale, float s, float a0) {
    const float w = mul_rn(alpha, r);
    if constexpr (kBlockStep) rhs = r > 0.f ? sub_rn(add_rn(a0, w), mul_rn(w, s)) : 0.f;  // (1 + w) - w s: minus half the gradient's weight at score s
    else rhs = r > 0.f ? add_rn(a0, w) : 0.f;
    scale = w;
}

// G into the 32x32x2 accumulators of k_als_gram<NT>: tile (I, J), register r of lane (c31, h) is G[32 I + (r & 3) + 8 (r >> 2) + 4 h][32 J + c31]
// (Diag::kBaseRho: rho, the segment's regulariser (seg_rho), goes on the diagonal -- one fp32 add on top of G0)
template <int NT>
__device__ __forceinline__ void ials_base32(f32x16 (&acc)[Tiles<NT>::kCount], const float* __restrict__ G, uint32_t k, uint32_t c31, uint32_t h,
                                            float rho) {
    int ti = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = 32 * I + (r & 3) + 8 * (r >> 2) + 4 * h, col = 32 * J + c31;
                acc[ti][r] = row < k && col < k ? G[row * k + col] : 0.f;
                if constexpr (kDiag == Diag::kBaseRho)
                    if (I == J && row == col && row < k) acc[ti][r] = add_rn(acc[ti][r], rho);
            }
}
// One gathered row pair of k_als_gram<NT>, implicit form: rhs from the unscaled row, then the weighted MFMAs
template <int NT>
__device__ __forceinline__ void ials_rows(float (&av)[NT], float rv, float alpha, float (&bacc)[NT], f32x16 (&acc)[Tiles<NT>::kCount],
                                          float sv, float a0) {
    float rw, sw;
    ials_weights(rv, alpha, rw, sw, sv, a0);
    float xa[NT];
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        bacc[I] += rw * av[I];
        xa[I] = av[I] * sw;
    }
    int ti = 0;
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = I; J < NT; ++J, ++ti)
            acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[I], av[J], acc[ti], 0, 0, 0);
}

// Waves per SIMD the LDS image allows anyway (k = 128: 34 KB per system -> one wave per SIMD; k = 96: two), stated
// so that the register allocator does not trade the Gramian loop's pipelining for an occupancy it cannot get.
constexpr int als_waves(int NT) { return NT >= 4 ? 1 : NT == 3 ? 2 : NT == 2 ? 3 : 6; }

template <int NT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(als_waves(NT), als_waves(NT)))) void ALS_KERNEL(gram)(AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63, c31 = lane & 31, h = lane >> 5;
    const uint32_t item = blockIdx.x;
    if (item >= a.count) return;
    const AlsItem it = a.items[item];
    const uint32_t k = a.k;
    if (it.hi == it.lo) {  // empty segment: zero vector (src/ALS.cpp:151-157)
        for (uint32_t c = lane; c < k; c += 64) a.Y[(size_t) it.seg * k + c] = 0.f;
        return;
    }
    f32x16 acc[Tiles<NT>::kCount];
    float bacc[NT];
    unsigned long long tmark = a.phases ? __builtin_readcyclecounter() : 0ull;
#pragma unroll
    for (int t = 0; t < Tiles<NT>::kCount; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    if constexpr (kBaseGramian)
        if (it.slot < 0) ials_base32<NT>(acc, a.G, k, c31, h, seg_rho(a, it.seg));  // chunk partials start from zero: the reducer adds G
#pragma unroll
    for (int I = 0; I < NT; ++I) bacc[I] = 0.f;

    constexpr int U = NT >= 3 ? 4 : 8;  // gathered row pairs per step
    if constexpr (NT >= 3) {
        // The pipeline of k_als_gram16 in its generic form (64-bit addressing: this kernel also takes the gather tables
        // that one cannot): two register sets used alternately by consecutive steps of 2 U entries, no copies -- MFMAs of
        // step s on one set while the factor rows (and ratings) of step s + 1 load into the other and the indices of step
        // s + 2 load behind them.  Positions past the segment's end load the SENTINEL entry of the index / value arrays
        // (zero row, rating 0); columns past k gather the zero row.  (As a compiler-scheduled loop with "next" and
        // "current" arrays the copies between the two forced `s_waitcnt vmcnt(0)` on the loads just issued in front of
        // every MFMA block: at one wave per SIMD, k = 128, the whole gather latency of every step lay open.)
        const uint32_t zrow = (uint32_t) __builtin_amdgcn_readfirstlane((int) a.x_rows);
        uint32_t ix[2][U];
        float rv[2][U], sv[2][U];  // (sv: the stored scores, block steps only)
        float av[2][U][NT];
        auto load_idx = [&](auto S, uint32_t q0) {
            constexpr int s = decltype(S)::value;
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = q0 + 2 * u + h;
                ix[s][u] = a.idx[q < it.hi ? q : a.sentinel];
            }
        };
        auto load_rows = [&](auto S, uint32_t q0) {
            constexpr int s = decltype(S)::value;
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t row = ix[s][u];
                asm volatile("" : "+v"(row));  // opaque use: keeps the index load where it was issued (see g16_load_rows)
                const uint32_t q = q0 + 2 * u + h;
                rv[s][u] = a.val[q < it.hi ? q : a.sentinel];
                if constexpr (kBlockStep) sv[s][u] = arg_score(a)[q < it.hi ? q : a.sentinel];
    #pragma unroll
                for (int I = 0; I < NT; ++I) {
                    const uint32_t col = I * 32 + c31;
                    const bool in = col < k;
                    av[s][u][I] = a.X[(size_t) (in ? row : zrow) * k + (in ? col : 0u)];
                }
            }
        };
        auto mfmas = [&](auto S) {
            constexpr int s = decltype(S)::value;
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (kImplicit) {
                    ials_rows<NT>(av[s][u], rv[s][u], a.alpha, bacc, acc, score_of(sv[s][u]), arg_alpha0(a));
                    continue;
                }
                int ti = 0;
    #pragma unroll
                for (int I = 0; I < NT; ++I) {
                    bacc[I] += als_rhs(rv[s][u], score_of(sv[s][u])) * av[s][u][I];
    #pragma unroll
                    for (int J = I; J < NT; ++J, ++ti)
                        acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s][u][I], av[s][u][J], acc[ti], 0, 0, 0);
                }
            }
        };
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        load_idx(S0{}, it.lo);
        load_idx(S1{}, it.lo + 2 * U);
        load_rows(S0{}, it.lo);
        for (uint32_t q0 = it.lo;;) {
            load_rows(S1{}, q0 + 2 * U);
            load_idx(S0{}, q0 + 4 * U);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(S0{});
            __builtin_amdgcn_sched_barrier(0);
            q0 += 2 * U;
            if (q0 >= it.hi) break;
            load_rows(S0{}, q0 + 2 * U);
            load_idx(S1{}, q0 + 4 * U);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(S1{});
            __builtin_amdgcn_sched_barrier(0);
            q0 += 2 * U;
            if (q0 >= it.hi) break;
        }
    } else {
        // k <= 64 (3 to 6 waves per SIMD): the compiler-scheduled form of the same pipeline, which is the faster
        // one there (k = 32: 7.9 ms per iteration against 9.0 ms for the explicit two-set form)
        // Same pipeline as k_als_gram16: indices / ratings two batches ahead, factor rows one batch ahead,
        // every load unconditional -- positions past the segment's end and columns past k gather from the
        // all-zero row X[x_rows].
        // A position past the segment's end loads the SENTINEL entry of the index / value arrays (the zero row, rating 0):
        // a select between two positions of one array.  Written as `q < hi ? idx[q] : x_rows` the conditional is folded
        // into a select between two ADDRESSES (the index array, the slot holding x_rows) feeding one flat_load -- which
        // counts on lgkmcnt as well as vmcnt, so every batch began with `s_waitcnt vmcnt(0) lgkmcnt(0)`: all loads in
        // flight drained, the one issued two instructions earlier included (58 % of the MFMA rate).
        const uint32_t zrow = (uint32_t) __builtin_amdgcn_readfirstlane((int) a.x_rows);
        uint32_t row_n[U];
        float rv_n[U], rv_c[U];
        float sv_n[U], sv_c[U];  // (the stored scores, block steps only)
        float av_n[U][NT];
        auto load_idx = [&](uint32_t q0) {
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t q = q0 + 2 * u + h;
                const uint32_t qe = q < it.hi ? q : a.sentinel;
                row_n[u] = a.idx[qe];
                rv_n[u] = a.val[qe];
                if constexpr (kBlockStep) sv_n[u] = arg_score(a)[qe];
            }
        };
        auto load_rows = [&]() {
    #pragma unroll
            for (int u = 0; u < U; ++u) {
    #pragma unroll
                for (int I = 0; I < NT; ++I) {
                    const uint32_t col = I * 32 + c31;
                    const bool in = col < k;
                    av_n[u][I] = a.X[(size_t) (in ? row_n[u] : zrow) * k + (in ? col : 0u)];
                }
                rv_c[u] = rv_n[u];
                if constexpr (kBlockStep) sv_c[u] = sv_n[u];
            }
        };
        load_idx(it.lo);
        load_rows();
        load_idx(it.lo + 2 * U);
        for (uint32_t q0 = it.lo; q0 < it.hi; q0 += 2 * U) {
            float av[U][NT], rv[U], sv[U];
            if constexpr (kBlockStep) {
    #pragma unroll
                for (int u = 0; u < U; ++u) sv[u] = sv_c[u];
            }
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                rv[u] = rv_c[u];
    #pragma unroll
                for (int I = 0; I < NT; ++I) av[u][I] = av_n[u][I];
            }
            load_rows();
            load_idx(q0 + 4 * U);
    #pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (kImplicit) {
                    ials_rows<NT>(av[u], rv[u], a.alpha, bacc, acc, score_of(sv[u]), arg_alpha0(a));
                    continue;
                }
                int ti = 0;
    #pragma unroll
                for (int I = 0; I < NT; ++I) {
                    bacc[I] += als_rhs(rv[u], score_of(sv[u])) * av[u][I];
    #pragma unroll
                    for (int J = I; J < NT; ++J, ++ti)
                        acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][I], av[u][J], acc[ti], 0, 0, 0);
                }
            }
        }
    }
    if (it.slot >= 0) {  // chunk of a long segment: park the raw accumulators, the reducer finishes
        float* w = a.ws + (size_t) it.slot * slot_floats<NT>();
#pragma unroll
        for (int t = 0; t < Tiles<NT>::kCount; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) w[t * 1024 + r * 64 + lane] = acc[t][r];
#pragma unroll
        for (int I = 0; I < NT; ++I) w[Tiles<NT>::kCount * 1024 + I * 64 + lane] = bacc[I];
        return;
    }
    phase_mark(a, 0, tmark);
    if (a.phases && lane == 0) atomicAdd(a.phases + (blockIdx.x % kPhaseCopies) * 8 + 4, 1ull);
    stage_tiles32<NT>(acc, bacc, lds);
    factor_solve<NT>(lds, a, it.seg, tmark);
}

template <int NT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(als_waves(NT), als_waves(NT)))) void ALS_KERNEL(reduce)(AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63;
    if (blockIdx.x >= a.count) return;
    const AlsReduce rd = a.reduces[blockIdx.x];
    f32x16 acc[Tiles<NT>::kCount];
    float bacc[NT];
#pragma unroll
    for (int t = 0; t < Tiles<NT>::kCount; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    if constexpr (kBaseGramian) ials_base32<NT>(acc, a.G, a.k, lane & 31, lane >> 5, seg_rho(a, rd.seg));
#pragma unroll
    for (int I = 0; I < NT; ++I) bacc[I] = 0.f;
    for (uint32_t s = 0; s < rd.nslots; ++s) {  // chunk order: deterministic
        const float* w = a.ws + (size_t) (rd.slot0 + s) * slot_floats<NT>();
#pragma unroll
        for (int t = 0; t < Tiles<NT>::kCount; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] += w[t * 1024 + r * 64 + lane];
#pragma unroll
        for (int I = 0; I < NT; ++I) bacc[I] += w[Tiles<NT>::kCount * 1024 + I * 64 + lane];
    }
    stage_tiles32<NT>(acc, bacc, lds);
    factor_solve<NT>(lds, a, rd.seg);
}

// ---- 32 < k <= 64, k % 4 == 0: 16x16x4 tiles fed by 16-byte gathers ---------------------------------
// Lane l = (g = l >> 4, c = l & 15) loads X[row(q0 + g)][4c .. 4c+3] with ONE global_load_dwordx4: a
// wave instruction fetches four whole factor rows (1 KB) instead of two half rows (256 B), which is
// what the L2 / Infinity Cache gather rate wants.  Register e of that float4 is column 4c + e; taken
// as the A (and B) operand of v_mfma_f32_16x16x4_f32 (lane supplies A[i = c][kk = g]) it is "column
// set e", so tile (e, e') accumulates G[4c + e][4c' + e'] -- the Gramian under a fixed column
// permutation that stage_tiles16 undoes on the way to LDS.  10 of 16 tiles (upper triangle of the
// 4 x 4 set grid) = 320 MFMA cycles per 4 rows, against 384 for 3 of 4 32x32 tiles.
constexpr int kSets = 4, kTiles16 = kSets * (kSets + 1) / 2;

// G [k][k] into the 16x16x4 accumulators of k_als_gram16: tile (e, f), register q of lane (c, g) is G[4 (4 g + q) + e][4 c + f]
// (Diag::kBaseRho: rho on the diagonal, as in ials_base32)
__device__ __forceinline__ void ials_base16(f32x4 (&acc)[kTiles16], const float* __restrict__ G, uint32_t k, uint32_t c, uint32_t g,
                                            float rho) {
    int ti = 0;
#pragma unroll
    for (int e = 0; e < kSets; ++e)
#pragma unroll
        for (int f = e; f < kSets; ++f, ++ti)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t row = 4 * (4 * g + q) + e, col = 4 * c + f;
                acc[ti][q] = row < k && col < k ? G[row * k + col] : 0.f;
                if constexpr (kDiag == Diag::kBaseRho)
                    if (e == f && row == col && row < k) acc[ti][q] = add_rn(acc[ti][q], rho);
            }
}

__device__ __forceinline__ void stage_tiles16(f32x4 (&acc)[kTiles16], float (&bacc)[kSets], float* lds) {
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    float* L = lds;
    float* bv = lds + roff(64);
    int ti = 0;
#pragma unroll
    for (int e = 0; e < kSets; ++e) {
#pragma unroll
        for (int f = e; f < kSets; ++f, ++ti) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // accumulator register r of lane l is C[i = 4g + r][j = c]
                const int row = 4 * (4 * (int) g + r) + e;
                const int col = 4 * (int) c + f;
                const float x = acc[ti][r];
                if (row >= col) L[roff(row) + col] = x;
                else L[roff(col) + row] = x;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < kSets; ++e) {  // rhs: the four row groups hold partial sums of the same column
        float t = bacc[e] + __shfl_xor(bacc[e], 16, 64);
        t += __shfl_xor(t, 32, 64);
        if (g == 0) bv[4 * c + e] = t;
    }
}

// k = 64: the same image under the symmetric permutation "column 4 c + e -> 16 e + c", i.e. in the order the MFMA tiles
// hold it.  Tile (e, f), e <= f, of lane (c, g) holds G'[16 e + 4 g + r][16 f + c], r = 0..3: mirrored, four CONSECUTIVE
// entries of row 16 f + c of the packed lower triangle -- one ds_write_b128 per tile, ten in all, where the natural order
// needs forty ds_write_b32 with a row-or-column select each (a Cholesky factorisation is as good under one symmetric
// permutation as under another; the solution is written back through the inverse permutation).  Diagonal tiles: the
// lanes whose four entries lie (at least partly) on or below the diagonal of their row write, g <= c >> 2; what reaches
// past the diagonal lands in the row's alignment padding; the entries of the other lanes are the mirror images of those.
__device__ __forceinline__ void stage_tiles16_perm(f32x4 (&acc)[kTiles16], float (&bacc)[kSets], float* lds) {
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    float* L = lds;
    float* bv = lds + roff(64);
    int ti = 0;
#pragma unroll
    for (int e = 0; e < kSets; ++e) {
#pragma unroll
        for (int f = e; f < kSets; ++f, ++ti) {
            float* dst = L + roff(16 * f + (int) c) + 16 * e + 4 * (int) g;
            if (f > e || g <= (c >> 2)) *reinterpret_cast<f32x4*>(dst) = acc[ti];
        }
    }
#pragma unroll
    for (int e = 0; e < kSets; ++e) {  // rhs: the four row groups hold partial sums of the same column
        float t = bacc[e] + __shfl_xor(bacc[e], 16, 64);
        t += __shfl_xor(t, 32, 64);
        if (g == 0) bv[16 * e + c] = t;
    }
}

// Pipeline state of k_als_gram16: D register sets, used in turn by consecutive 16-row steps (no copies).
// (r4) two 4-row groups per step (8 gathered rows, 2 KB per set) instead of four: the loop's register sets halve, and a tail-dominated
// launch then fits FOUR waves per SIMD (128 VGPRs, 44 bytes of scratch per lane) -- user half of the Netflix shape 7.67 -> 7.26 ms, iteration
// 12.80 -> 12.30 ms; (waves, groups) = (3, 2) 12.80, (4, 4) 12.46, (5, 2) 21.3 (264 bytes of scratch), (4, 1) 13.3 (tools/exp_als_libs.sh)
constexpr int kU16 = 2;  // 4-row MFMA groups per step
constexpr uint32_t kRows16 = 4u * kU16;
template <int D>
struct Gram16Regs {
    uint32_t ix[D][kU16];  // gathered row indices           (stage 0: loaded D steps ahead of their MFMAs)
    f32x4 av[D][kU16];     // gathered factor-row quarters   (stage 1: D - 1 steps ahead)
    float rv[D][kU16];     // ratings                        (stage 1)
    float sv[D][kU16];     // scores of the stored pairs     (stage 1; block steps only.  Its place decides the allocation: DESIGN 5.7)
    f32x4 acc[kTiles16];
    f32x2 bacc[2];         // rhs partial sums of column sets (0, 1) and (2, 3)
};

// The three stages of one 16-row step s of a work item (entries lo + 16 s + 4 u + g, u = 0..3), each on register
// set S.  Every load is unconditional and has a wave-uniform base (SGPR pair: the item's first entry, advanced by
// the scalar unit) plus a lane-constant 32-bit offset plus an immediate -- no per-load address arithmetic on the
// vector unit.  Positions past the item's end read on into the next segment's entries (or the arrays' zero padding,
// AlsHalf::build); their ROW OFFSET is replaced by the all-zero row X[x_rows], so they add exact zeros (a rating
// read from past the end multiplies that zero row).
template <int D, int S>
__device__ __forceinline__ void g16_load_idx(Gram16Regs<D>& r, const uint32_t* __restrict__ ibase, uint32_t s, uint32_t g) {
#pragma unroll
    for (int u = 0; u < kU16; ++u) r.ix[S][u] = ibase[s * kRows16 + 4 * u + g];
}
template <int D, int S>
__device__ __forceinline__ void g16_load_rows(Gram16Regs<D>& r, const char* __restrict__ Xb, const float* __restrict__ vbase,
                                              uint32_t s, uint32_t g, uint32_t len, bool col_ok, uint32_t rowbytes,
                                              uint32_t lane_off, uint32_t zero_off, const float* __restrict__ sbase) {
#pragma unroll
    for (int u = 0; u < kU16; ++u) {
        const bool ok = col_ok && s * kRows16 + 4 * u + g < len;
        uint32_t ix = r.ix[S][u];
        // opaque use: otherwise the index load (only consumed when `ok`) is sunk out of the previous step into a
        // divergent branch right here, with a full wait behind it
        asm volatile("" : "+v"(ix));
        const uint32_t off = ok ? __umul24(ix, rowbytes) + lane_off : zero_off;  // x_rows < 2^24, table < 4 GB (launch_half)
        r.av[S][u] = *reinterpret_cast<const f32x4*>(Xb + off);
        r.rv[S][u] = vbase[s * kRows16 + 4 * u + g];
        if constexpr (kBlockStep) r.sv[S][u] = sbase[s * kRows16 + 4 * u + g];
    }
}
template <int D, int S>
__device__ __forceinline__ void g16_mfma(Gram16Regs<D>& r, float alpha, float a0) {
#pragma unroll
    for (int u = 0; u < kU16; ++u) {
        if constexpr (kImplicit) {  // the same with the weights of ials_weights: rhs from the unscaled row, then the MFMAs
            float rw, sw;
            ials_weights(r.rv[S][u], alpha, rw, sw, score_of(r.sv[S][u]), a0);
            const float hi = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, rw), 0xE4, 0xF, 0xF, false));
            const f32x2 rr = {rw, hi};
            r.bacc[0] = fma2(rr, r.av[S][u].lo, r.bacc[0]);
            r.bacc[1] = fma2(rr, r.av[S][u].hi, r.bacc[1]);
            const f32x4 xa = r.av[S][u] * sw;  // A operand
            int ti = 0;
#pragma unroll
            for (int e = 0; e < kSets; ++e)
#pragma unroll
                for (int f = e; f < kSets; ++f, ++ti)
                    r.acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[e], r.av[S][u][f], r.acc[ti], 0, 0, 0);
            continue;
        }
        // rhs: two v_pk_fma_f32 with the rating duplicated into a register pair BY HAND.  The compiler's own form reads
        // the rating through op_sel from (rating, whatever sits in the odd partner register) -- which the allocator
        // fills with a destination of the loads just issued, and the waitcnt pass then drains every load in flight
        // (s_waitcnt vmcnt(0)) in front of the MFMA block of every second step.
        const float rw = als_rhs(r.rv[S][u], score_of(r.sv[S][u]));
        const float hi = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(
            0, __builtin_bit_cast(int, rw), 0xE4 /* quad_perm [0,1,2,3]: a plain copy the optimiser cannot fold */, 0xF, 0xF, false));
        const f32x2 rr = {rw, hi};
        r.bacc[0] = fma2(rr, r.av[S][u].lo, r.bacc[0]);
        r.bacc[1] = fma2(rr, r.av[S][u].hi, r.bacc[1]);
        int ti = 0;
#pragma unroll
        for (int e = 0; e < kSets; ++e)
#pragma unroll
            for (int f = e; f < kSets; ++f, ++ti)
                r.acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(r.av[S][u][e], r.av[S][u][f], r.acc[ti], 0, 0, 0);
    }
}
struct Gram16Ctx {  // loop-invariant operands of the stages
    const uint32_t* ibase; const float* vbase; const char* Xb;
    uint32_t g, len, rowbytes, lane_off, zero_off;
    bool col_ok;
    float alpha, alpha0;  // (kImplicit only; alpha0 is 1 but for kAlpha0)
    const float* sbase;   // (kBlockStep only) the stored scores of the item's entries
};
// Steps s, s + 1, ... on sets U, U + 1, ... D - 1: MFMAs of step s on set U, the factor rows of step s + D - 1 into the
// set the previous step has just released, the indices of step s + D into this step's own (already consumed) slots.
// True when the item is finished.  (sched_barrier: left to itself the scheduler sinks the loads of a step down to
// their first use, D - 1 steps later.)
template <int D, int U>
__device__ __forceinline__ bool g16_steps(Gram16Regs<D>& r, const Gram16Ctx& c, uint32_t& s) {
    if constexpr (U < D) {
        g16_load_rows<D, (U + D - 1) % D>(r, c.Xb, c.vbase, s + D - 1, c.g, c.len, c.col_ok, c.rowbytes, c.lane_off, c.zero_off, c.sbase);
        g16_load_idx<D, U>(r, c.ibase, s + D, c.g);
        __builtin_amdgcn_sched_barrier(0);
        g16_mfma<D, U>(r, c.alpha, c.alpha0);
        __builtin_amdgcn_sched_barrier(0);
        if (++s * kRows16 >= c.len) return true;
        return g16_steps<D, U + 1>(r, c, s);
    } else {
        return false;
    }
}
template <int D, int U>
__device__ __forceinline__ void g16_prologue(Gram16Regs<D>& r, const Gram16Ctx& c) {
    if constexpr (U < D) {
        g16_load_idx<D, U>(r, c.ibase, U, c.g);
        g16_prologue<D, U + 1>(r, c);
        if constexpr (U + 1 < D)  // (after ALL index loads are in flight)
            g16_load_rows<D, U>(r, c.Xb, c.vbase, U, c.g, c.len, c.col_ok, c.rowbytes, c.lane_off, c.zero_off, c.sbase);
    }
}

// Why the loop looks the way it does: with ~100 vector instructions around the 40 MFMAs of a step (64-bit address
// arithmetic per gathered row, clamps and selects per index, register copies between "next" and "current" sets, a
// flat_load born from a select between two addresses) the loop was replaced by this explicit two-set pipeline:
// ~45 vector instructions per step.  tools/ubench_mfma32.hip replays it on L1-resident data: 130 TF of the 157 TF
// fp32 matrix peak at 2.4 GHz; inside the solver (2.2 GHz under load) the Gramian alone runs at 62 % of the matrix
// rate whether the gather is served from HBM, L2 or L1 -- the rest of a half-sweep is the per-system tail.
// WAVES per SIMD: a launch whose items are long (the item half: 2048-row chunks, hardly any tails) is fastest with
// TWO waves per SIMD (5.42 -> 4.91 ms at the Netflix shape), one dominated by per-system tails (the user half, 206
// entries per system) wants the latency hiding of three or four (7.9 ms; 9.2 ms at two; r4: four, see kU16).  Three = 168 VGPRs, no
// spills; four = 128 VGPRs + 18 spilled dwords, same time.
template <int WAVES, int D, bool FULL>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void ALS_KERNEL(gram16)(AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const uint32_t item = blockIdx.x;
    if (item >= a.count) return;
    const AlsItem it = a.items[item];
    const uint32_t k = a.k;
    if (it.hi == it.lo) {  // empty segment: zero vector (src/ALS.cpp:151-157)
        for (uint32_t cc = lane; cc < k; cc += 64) a.Y[(size_t) it.seg * k + cc] = 0.f;
        return;
    }
    Gram16Regs<D> r;
    unsigned long long tmark = a.phases ? __builtin_readcyclecounter() : 0ull;
#pragma unroll
    for (int t = 0; t < kTiles16; ++t) r.acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (kBaseGramian)
        if (it.slot < 0) ials_base16(r.acc, a.G, k, c, g, seg_rho(a, it.seg));  // chunk partials start from zero: the reducer adds G
    r.bacc[0] = r.bacc[1] = f32x2{0.f, 0.f};

    Gram16Ctx cx;
    cx.len = it.hi - it.lo;
    cx.ibase = a.idx + it.lo;
    cx.vbase = a.val + it.lo;
    cx.sbase = kBlockStep ? arg_score(a) + it.lo : nullptr;
    cx.Xb = reinterpret_cast<const char*>(a.X);
    cx.rowbytes = 4 * k;
    cx.col_ok = 4 * c < k;                 // lanes past column k gather the zero row
    cx.lane_off = 16 * c;
    cx.zero_off = a.x_rows * cx.rowbytes;
    cx.g = g;
    cx.alpha = kImplicit ? a.alpha : 0.f;
    cx.alpha0 = arg_alpha0(a);
    g16_prologue<D, 0>(r, cx);
    for (uint32_t s = 0;;)
        if (g16_steps<D, 0>(r, cx, s)) break;
    if (it.slot >= 0) {  // chunk of a long segment: park the raw accumulators, the reducer finishes
        float* w = a.ws + (size_t) it.slot * slot_floats<2>();
#pragma unroll
        for (int t = 0; t < kTiles16; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[t * 256 + q * 64 + lane] = r.acc[t][q];
#pragma unroll
        for (int e = 0; e < kSets; ++e) w[kTiles16 * 256 + e * 64 + lane] = r.bacc[e >> 1][e & 1];
        return;
    }
    phase_mark(a, 0, tmark);
    if (a.phases && lane == 0) atomicAdd(a.phases + (blockIdx.x % kPhaseCopies) * 8 + 4, 1ull);
    float bacc[kSets] = {r.bacc[0].x, r.bacc[0].y, r.bacc[1].x, r.bacc[1].y};
    if constexpr (FULL) stage_tiles16_perm(r.acc, bacc, lds);
    else stage_tiles16(r.acc, bacc, lds);
    factor_solve<2, FULL>(lds, a, it.seg, tmark);
}

__global__ __launch_bounds__(64) void ALS_KERNEL(reduce16)(AlsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const uint32_t lane = threadIdx.x & 63;
    if (blockIdx.x >= a.count) return;
    const AlsReduce rd = a.reduces[blockIdx.x];
    f32x4 acc[kTiles16];
    float bacc[kSets];
#pragma unroll
    for (int t = 0; t < kTiles16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (kBaseGramian) ials_base16(acc, a.G, a.k, lane & 15, lane >> 4, seg_rho(a, rd.seg));
#pragma unroll
    for (int e = 0; e < kSets; ++e) bacc[e] = 0.f;
    for (uint32_t s = 0; s < rd.nslots; ++s) {  // chunk order: deterministic
        const float* w = a.ws + (size_t) (rd.slot0 + s) * slot_floats<2>();
#pragma unroll
        for (int t = 0; t < kTiles16; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += w[t * 256 + r * 64 + lane];
#pragma unroll
        for (int e = 0; e < kSets; ++e) bacc[e] += w[kTiles16 * 256 + e * 64 + lane];
    }
    stage_tiles16(acc, bacc, lds);
    factor_solve<2>(lds, a, rd.seg);
}

// (waves per SIMD, pipeline depth) of k_als_gram16 for launches of long items / of tail-dominated items.  Depth:
// measured at the Netflix shape, item half: (2 waves, depth 2) 4.90 ms, (2, 4) 4.93, (2, 6) 4.94, (3, 4) 5.09 -- the
// gather of 25 GB of 256-byte rows from a 123 MB table runs at 5.2 TB/s either way.
// (kMultiRhs: the further solves of the implicit families leave the k < 64 form no room for four waves -- 152 VGPRs -- so they ask for three)
constexpr int kG16WavesLong = 2, kG16DepthLong = 2, kG16WavesShort = kMultiRhs && kImplicit ? 3 : 4, kG16DepthShort = 2;
int launch_half_16(const AlsArgs& base, uint32_t nitems, uint32_t nreduces, uint64_t nnz, hipStream_t st) {
    const size_t lds_bytes = ((size_t) roff_host(64) + 64) * sizeof(float);
    AlsArgs a = base;
    if (nitems) {
        a.count = nitems;
        // mean entries per work item: long items -> two waves per SIMD, tail-dominated launches -> three.  The items are
        // AlsHalf::build's (als_host.hip), with chunk = kAlsChunk: a segment [lo, hi) is one item `if (hi - lo <= chunk)`,
        // else `pieces = (hi - lo + chunk - 1) / chunk;` items of chunk entries and a shorter last one -- so a mean of 1024
        // and more is reached only where much of the work is chunks of split segments
        const bool longs = nnz / nitems >= 1024, full = a.k == 64;
        if (longs && full) hipLaunchKernelGGL((ALS_KERNEL(gram16)<kG16WavesLong, kG16DepthLong, true>), dim3(nitems), dim3(64), lds_bytes, st, a);
        else if (longs) hipLaunchKernelGGL((ALS_KERNEL(gram16)<kG16WavesLong, kG16DepthLong, false>), dim3(nitems), dim3(64), lds_bytes, st, a);
        else if (full) hipLaunchKernelGGL((ALS_KERNEL(gram16)<kG16WavesShort, kG16DepthShort, true>), dim3(nitems), dim3(64), lds_bytes, st, a);
        else hipLaunchKernelGGL((ALS_KERNEL(gram16)<kG16WavesShort, kG16DepthShort, false>), dim3(nitems), dim3(64), lds_bytes, st, a);
        MFX_HIP(hipGetLastError());
    }
    if (nreduces) {
        a.count = nreduces;
        hipLaunchKernelGGL(ALS_KERNEL(reduce16), dim3(nreduces), dim3(64), lds_bytes, st, a);
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

template <int NT>
int launch_half_nt(const AlsArgs& base, uint32_t nitems, uint32_t nreduces, hipStream_t st) {
    constexpr int KP = 32 * NT;
    // packed lower triangle (rows rounded up to 4 floats) + rhs: see solve_tail
    const size_t lds_bytes = ((size_t) 4 * (KP / 4 + 1) * (2 * (KP / 4)) + KP) * sizeof(float);
    if (lds_bytes > 48 * 1024) {  // a per-device attribute; setting it again is cheap next to a half-sweep
        MFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ALS_KERNEL(gram)<NT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes));
        MFX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ALS_KERNEL(reduce)<NT>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_bytes));
    }
    AlsArgs a = base;
    if (nitems) {
        a.count = nitems;
        hipLaunchKernelGGL(ALS_KERNEL(gram)<NT>, dim3(nitems), dim3(64), lds_bytes, st, a);
        MFX_HIP(hipGetLastError());
    }
    if (nreduces) {
        a.count = nreduces;
        hipLaunchKernelGGL(ALS_KERNEL(reduce)<NT>, dim3(nreduces), dim3(64), lds_bytes, st, a);
        MFX_HIP(hipGetLastError());
    }
    return MFX_OK;
}

int launch_half(const AlsArgs& a, uint32_t nitems, uint32_t nreduces, uint64_t nnz, hipStream_t st) {
    const uint32_t nt = (a.k + 31) / 32;
    // 16-byte aligned factor rows; k_als_gram16 forms 32-bit byte offsets into X with a 24-bit multiply
    if (a.k > 32 && a.k <= 64 && a.k % 4 == 0 && a.x_rows < (1u << 24) && ((uint64_t) a.x_rows + 1) * a.k * 4 < (1ull << 32))
        return launch_half_16(a, nitems, nreduces, nnz, st);
    switch (nt) {
        case 1: return launch_half_nt<1>(a, nitems, nreduces, st);
        case 2: return launch_half_nt<2>(a, nitems, nreduces, st);
        case 3: return launch_half_nt<3>(a, nitems, nreduces, st);
        case 4: return launch_half_nt<4>(a, nitems, nreduces, st);
        default: return fail(MFX_ERR_INVALID, "ALS: rank k = %u not supported (1 <= k <= 128)", a.k);
    }
}

// k_als_gram16 at pipeline depth D loads the indices of step s + D while it works on step s: at most 16 (D + 1) + 15
// entries past an item's end, inside the padding that AlsHalf::build puts behind the index / value arrays
static_assert(kAlsEntryPad >= 16 * ((kG16DepthLong > kG16DepthShort ? kG16DepthLong : kG16DepthShort) + 2),
              "index / value padding too short for the pipeline depth");

// The arguments that every family takes from an orientation, its factor tables and its workspace; everything else is zero
AlsArgs half_args(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, float* ws, uint32_t* spd_fail) {
    AlsArgs a{};
    a.items = h.items.get(); a.reduces = h.reduces.get(); a.idx = h.idx.get(); a.val = h.val.get();
    a.X = X; a.x_rows = x_rows; a.sentinel = (uint32_t) h.nnz; a.Y = Y; a.k = k; a.ws = ws; a.spd_fail = spd_fail;
    return a;
}

}  // namespace

// ---- Entry points: one per family (declared in als_solver.hpp) ---------------------------------------------------------
// The base-Gramian families leave a.lambda = 0: lambda is on G's diagonal already (Diag::kBase), or rho goes on the diagonal
// with the start of the accumulators (Diag::kBaseRho).
#if ALS_FAMILY >= ALS_FAMILY_ALSM
// The four multi-right-hand-side families (mfx_rec_explain): the half-sweep of the family without, plus the targets and Z;
// each takes from m what its diagonal needs
int ALS_MRHS_LAUNCH(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const AlsMrhs& m, float* ws, uint32_t* spd_fail,
                    hipStream_t st) {
    AlsArgs a = half_args(h, X, x_rows, Y, k, ws, spd_fail);
    a.targets = m.targets; a.n_targets = m.n_targets; a.Z = m.Z;
#if ALS_FAMILY == ALS_FAMILY_IALSRM
    a.alpha = m.alpha; a.G = m.G; a.alpha0 = m.alpha0; a.rho = m.rho;
#elif ALS_FAMILY == ALS_FAMILY_IALSM
    a.alpha = m.alpha; a.G = m.G;
#elif ALS_FAMILY == ALS_FAMILY_ALSNM
    a.lambda = m.lambda;
    a.seg_ptr = h.ptr.get();
#else
    a.lambda = m.lambda;
#endif
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_ALSB
int alsb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, float lambda, int32_t reg,
                     const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, Xb, x_rows, Z, d, ws, spd_fail);
    a.lambda = lambda;
    a.seg_ptr = reg ? h.ptr.get() : nullptr;
    a.score = score; a.P = P;
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_IALSRB
int ialsrb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, const float* Gbb, float alpha, float alpha0,
                       const float* rho, const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, Xb, x_rows, Z, d, ws, spd_fail);
    a.alpha = alpha; a.G = Gbb; a.score = score; a.P = P; a.alpha0 = alpha0; a.rho = rho;
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_IALSR
int ialsr_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const float* G0, float alpha, float alpha0,
                      const float* rho, float* ws, uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, X, x_rows, Y, k, ws, spd_fail);
    a.alpha = alpha; a.G = G0; a.alpha0 = alpha0; a.rho = rho;
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_IALSB
int ialsb_step_launch(const AlsHalf& h, const float* Xb, uint32_t x_rows, float* Z, uint32_t d, const float* Gbb, float alpha,
                      const float* score, const float* P, float* ws, uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, Xb, x_rows, Z, d, ws, spd_fail);
    a.alpha = alpha; a.G = Gbb; a.score = score; a.P = P;
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_IALS
int ials_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, const float* G, float alpha,
                     float* ws, uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, X, x_rows, Y, k, ws, spd_fail);
    a.alpha = alpha; a.G = G;
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#elif ALS_FAMILY == ALS_FAMILY_ALSN
int als_half_nreg_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, float lambda, float* ws,
                         uint32_t* spd_fail, hipStream_t st) {
    AlsArgs a = half_args(h, X, x_rows, Y, k, ws, spd_fail);
    a.lambda = lambda;
    a.seg_ptr = h.ptr.get();
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}
#else  // ALS_FAMILY_ALS
int als_half_launch(const AlsHalf& h, const float* X, uint32_t x_rows, float* Y, uint32_t k, float lambda, float* ws,
                    uint32_t* spd_fail, hipStream_t st, unsigned long long* phases) {
    AlsArgs a = half_args(h, X, x_rows, Y, k, ws, spd_fail);
    a.lambda = lambda;
    a.phases = phases;  // MFX_ALS_PHASES=1 (diagnostic): per-phase clocks of the half-sweep kernels, printed by AlsSolver::iterate
    return launch_half(a, h.nitems, h.nreduces, h.nnz, st);
}

// The Gramian dump of als_gramian_op: one unsplit item over `cnt` gathered rows, A [k][k] = its Gramian without lambda
int als_gramian_launch(const AlsItem* item, const uint32_t* idx, const float* val, uint32_t cnt, const float* X, uint32_t x_rows, float* Y,
                       uint32_t k, uint32_t* spd_fail, float* A, hipStream_t st) {
    AlsArgs a{};
    a.items = item; a.idx = idx; a.val = val; a.X = X; a.x_rows = x_rows; a.sentinel = cnt; a.Y = Y;
    a.k = k; a.lambda = 0.f; a.spd_fail = spd_fail; a.gram_out = A;
    return launch_half(a, 1, 0, (uint64_t) cnt, st);
}
#endif

}  // namespace mfx
