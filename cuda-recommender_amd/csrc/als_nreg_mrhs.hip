// als_nreg_mrhs.hip -- the k_alsnm_* (k_alsn_* with n_targets more right-hand sides per segment, for mfx_rec_explain):
// als_solver.hip as that family of its variant table.
#define MFX_ALS_NREG 1
#define MFX_ALS_MRHS 1
#include "als_solver.hip"
