// als_mrhs.hip -- the k_alsm_* (k_als_* with n_targets more right-hand sides per segment, for mfx_rec_explain):
// als_solver.hip as that family of its variant table.
#define MFX_ALS_MRHS 1
#include "als_solver.hip"
