// ials_reg_block_step.hip -- the block systems of the objective of ials_reg_half.hip (k_ialsrb_* and ialsrb_step_launch):
// als_solver.hip as the k_ialsrb_* family of its variant table; the sweep itself is ials_block.hip.
#define MFX_ALS_BLOCK 1
#define MFX_ALS_REG 1
#include "als_solver.hip"
