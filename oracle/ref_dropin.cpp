/*
 * ref_dropin.cpp -- drop-in proof for host/reference_api.hpp.
 * TEST INFRASTRUCTURE ONLY; builds into oracle/_ref/ref_dropin (git-ignored).
 *
 * Compiled by oracle/Makefile against the REFERENCE's own src/pmf.h types (included from where
 * they lie, nothing copied) and linked with libmfx.so: both kernel_wrapper_*_NV signatures are
 * called exactly like the reference's src/main.cpp:11-17 does.  tests/test_host.py runs the
 * binary, so the check needs no reference tree at test time.
 */
#include "pmf.h" /* reference: SparseMatrix / TestData / MatData / parameter */
#define MFX_SHIM_EXTERNAL_TYPES
#include "reference_api.hpp"

void runCUDA(SparseMatrix& R, TestData& T, MatData& W, MatData& H, parameter& parameters, bool ALS) {
    if (ALS) kernel_wrapper_als_NV(R, T, W, H, parameters);
    else kernel_wrapper_ccdpp_NV(R, T, W, H, parameters);
}

int main() { return 0; }
