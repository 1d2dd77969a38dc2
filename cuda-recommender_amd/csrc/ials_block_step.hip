// ials_block_step.hip -- the block systems of implicit ALS by block subspace sweeps (k_ialsb_gram / gram16 / reduce /
// reduce16 and ialsb_step_launch, see MFX_ALS_BLOCK in als_solver.hip): als_solver.hip's kernels compiled once more with
// the block-step flag set.  The sweep itself is ials_block.hip.
#define MFX_ALS_BLOCK 1
#include "als_solver.hip"
