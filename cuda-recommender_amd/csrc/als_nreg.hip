// als_nreg.hip -- the explicit half-sweep kernels with fp32(lambda * n) on the diagonal of a segment of n entries (k_alsn_*,
// see MFX_ALS_NREG in als_solver.hip) and als_half_nreg_launch: als_solver.hip's kernels compiled once more with the
// per-segment regularisation flag set.  mfx_rec_fold_in solves MFX_FOLD_CCD with them.
#define MFX_ALS_NREG 1
#include "als_solver.hip"
