// ials_reg_half.hip -- the implicit half-sweep kernels with an unobserved weight and a regulariser per segment (k_ialsr_*,
// see MFX_ALS_REG in als_solver.hip) and ialsr_half_launch: als_solver.hip's kernels compiled once more with both flags set.
#define MFX_ALS_IMPLICIT 1
#define MFX_ALS_REG 1
#include "als_solver.hip"
