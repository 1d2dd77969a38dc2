// als_nreg.hip -- the explicit half-sweep kernels with fp32(lambda * n) on the diagonal of a segment of n entries (k_alsn_*)
// and als_half_nreg_launch: als_solver.hip as the k_alsn_* family of its variant table.  mfx_rec_fold_in solves
// MFX_FOLD_CCD with them.
#define MFX_ALS_NREG 1
#include "als_solver.hip"
