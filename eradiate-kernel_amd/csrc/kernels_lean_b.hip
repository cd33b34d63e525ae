// kernels_lean_b.hip -- as kernels_lean_a.hip for scenes that keep all promises but two: an rpv BSDF and grids evaluated through
// volume_eval() (the weight volume of a blendphase) are allowed.  The layered atmosphere (C4 / C5) is one.
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_B     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
