// ials_block_step.hip -- the block systems of implicit ALS by block subspace sweeps (k_ialsb_gram / gram16 / reduce /
// reduce16 and ialsb_step_launch): als_solver.hip as the k_ialsb_* family of its variant table.  The sweep itself is
// ials_block.hip.
#define MFX_ALS_BLOCK 1
#include "als_solver.hip"
