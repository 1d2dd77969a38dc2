// ials_reg_block_step.hip -- the block systems of the same objective (k_ialsrb_* and ialsrb_step_launch, see MFX_ALS_REG and
// MFX_ALS_BLOCK in als_solver.hip); the sweep itself is ials_block.hip.
#define MFX_ALS_BLOCK 1
#define MFX_ALS_REG 1
#include "als_solver.hip"
