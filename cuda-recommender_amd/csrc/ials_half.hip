// ials_half.hip -- the implicit-feedback half-sweep kernels (k_ials_*, see "Implicit feedback" in als_solver.hip) and
// ials_half_launch: als_solver.hip as the k_ials_* family of its variant table.
#define MFX_ALS_IMPLICIT 1
#include "als_solver.hip"
