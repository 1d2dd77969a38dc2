// ials_reg_half.hip -- the implicit half-sweep kernels with an unobserved weight and a regulariser per segment (k_ialsr_*)
// and ialsr_half_launch: als_solver.hip as the k_ialsr_* family of its variant table.
#define MFX_ALS_IMPLICIT 1
#define MFX_ALS_REG 1
#include "als_solver.hip"
