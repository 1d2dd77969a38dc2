// ials_half_mrhs.hip -- the k_ialsm_* (k_ials_* with n_targets more right-hand sides per segment, for mfx_rec_explain):
// als_solver.hip as that family of its variant table.
#define MFX_ALS_IMPLICIT 1
#define MFX_ALS_MRHS 1
#include "als_solver.hip"
