// spd_inverse.hip -- Minv ~ G^-1 of one symmetric positive definite matrix G [k][k] on the device, 1 <= k <= 1024, gfx950
// (mfx_spd_inverse; the preconditioner of mfx_ials_cg_create).  Blocked with blocks of kSpdB = 32 coordinates on
// a padded copy A [kp][kp], kp = k rounded up to 32, whose tail is the identity (nothing outside [k][k] of G or Minv is ever
// touched, and the tail contributes exact zeros):
//   G = L L^T      for j = 0 .. nb - 1:  k_spd_diag   L_jj and T_jj = L_jj^-1 of the diagonal block, one workgroup, fp64 in LDS
//                                        k_spd_panel  L_ij = A_ij T_jj^T for i > j, one wavefront per block
//                                        k_spd_trail  A_ip -= L_ij L_pj^T for j < p <= i, one wavefront per block
//   T = L^-1       k_spd_scale   M_it = T_ii L_it for t < i (every block at once); then for s = 1 .. nb - 1
//                  k_spd_tinv    T_ij = -sum_{t = j .. i - 1} M_it T_tj for i = j + s, one wavefront per block, t ascending
//   Minv = T^T T   k_spd_prod    block (a, b), a <= b: sum_{t = b .. nb - 1} T_ta^T T_tb, t ascending, written with its mirror
// kp = 32 (k <= 32) is the diagonal kernel alone, which then forms T^T T in fp64 too.  Every block product is a chain of
// v_mfma_f32_32x32x2_f32 over the summed index in ascending order, so every sum's order is fixed by k: the bits of Minv depend
// on (G, k) alone.  The stages depend on each other by stream order only: no kernel waits for another workgroup, no float
// atomics.  A pivot that is <= 0 or not finite counts into *fail (an integer atomic) and is replaced by 1: every later stage
// runs to its end, Minv is then unspecified.  4 nb launches for nb = kp / 32 > 1 blocks: 128 at k = 1024.
// The kernels themselves are in spd_device.hpp (ease_inverse.hip runs them without the cap).
#include "als_solver.hpp"

namespace mfx {
namespace {
constexpr uint32_t kSpdB = 32;
}  // namespace
}  // namespace mfx

#include "spd_device.hpp"

namespace mfx {

size_t spd_inverse_ws_floats(uint32_t k) { return (size_t) 3 * spd_kp(k) * spd_kp(k); }

int spd_inverse_launch(const float* G, uint32_t k, float* Minv, float* ws, uint32_t* fail, hipStream_t st) {
    MFX_REQUIRE(k >= 1 && k <= kIalsBlockMaxRank, "SPD inverse: k = %u not supported (1 <= k <= %u)", k, kIalsBlockMaxRank);
    const uint32_t kp = spd_kp(k), nb = kp / kSpdB;
    float *A = ws, *T = ws + (size_t) kp * kp, *M = ws + (size_t) 2 * kp * kp;
    hipLaunchKernelGGL(k_spd_copy, dim3((kp * kp + 255) / 256), dim3(256), 0, st, G, k, kp, A);
    MFX_HIP(hipGetLastError());
    for (uint32_t j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(k_spd_diag, dim3(1), dim3(64), 0, st, A, T, kp, j, fail, nb == 1 ? Minv : nullptr, k);
        MFX_HIP(hipGetLastError());
        const uint32_t left = nb - j - 1;
        if (!left) break;
        hipLaunchKernelGGL(k_spd_panel, dim3(left), dim3(64), 0, st, A, T, kp, j);
        MFX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_spd_trail, dim3(left * (left + 1) / 2), dim3(64), 0, st, A, kp, j);
        MFX_HIP(hipGetLastError());
    }
    if (nb == 1) return MFX_OK;
    hipLaunchKernelGGL(k_spd_scale, dim3(nb * (nb - 1) / 2), dim3(64), 0, st, A, T, kp, M);
    MFX_HIP(hipGetLastError());
    for (uint32_t s = 1; s < nb; ++s) {
        hipLaunchKernelGGL(k_spd_tinv, dim3(nb - s), dim3(64), 0, st, M, T, kp, s);
        MFX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_spd_prod, dim3(nb * (nb + 1) / 2), dim3(64), 0, st, T, kp, nb, k, Minv);
    MFX_HIP(hipGetLastError());
    return MFX_OK;
}

int spd_inverse_op(int64_t k, const float* A, float* Ainv, int device) {
    MFX_REQUIRE(k >= 1 && k <= (int64_t) kIalsBlockMaxRank, "mfx_spd_inverse: k = %lld not supported (1 <= k <= %u)", (long long) k, kIalsBlockMaxRank);
    MFX_TRY(use_device(device));
    OpStream os;
    MFX_HIP(hipStreamCreateWithFlags(&os.st, hipStreamNonBlocking));
    const size_t kk = (size_t) k * k;
    DevBuf<float> G, Minv, ws;
    DevBuf<uint32_t> fail;
    MFX_TRY(G.alloc(kk));
    MFX_TRY(G.upload(A, kk, MFX_HOST, os.st));
    MFX_TRY(Minv.alloc_zero(kk, os.st));
    MFX_TRY(ws.alloc(spd_inverse_ws_floats((uint32_t) k)));
    MFX_TRY(fail.alloc_zero(1, os.st));
    MFX_TRY(spd_inverse_launch(G.get(), (uint32_t) k, Minv.get(), ws.get(), fail.get(), os.st));
    uint32_t bad = 0;
    MFX_HIP(hipMemcpyAsync(&bad, fail.get(), sizeof(uint32_t), hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipMemcpyAsync(Ainv, Minv.get(), sizeof(float) * kk, hipMemcpyDeviceToHost, os.st));
    MFX_HIP(hipStreamSynchronize(os.st));
    MFX_REQUIRE(bad == 0, "mfx_spd_inverse: A is not positive definite (%u pivots <= 0 or not finite): it must be symmetric, positive definite and finite",
                bad);
    return MFX_OK;
}

}  // namespace mfx
