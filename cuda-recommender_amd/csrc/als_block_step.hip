// als_block_step.hip -- the block systems of explicit ALS by block subspace sweeps (k_alsb_gram / gram16 / reduce /
// reduce16 and alsb_step_launch): als_solver.hip as the k_alsb_* family of its variant table, the explicit kernels with the
// block-step inputs (stored scores, rhs from -P, the step written out).  The sweep is the explicit part of ials_block.hip.
#define MFX_ALS_BLOCK 2
#include "als_solver.hip"
