// kernels_lean_p.hip -- `path` as the flat loop with regeneration (kernels.hip: path_pixel_flat; rgb / mono) for scenes with a walked primitive
// list, no spheres and no rpv BSDF -- the cornell box (C1, C1L) is one; area emitters stay.  Three of the four out-of-line functions of
// the general kernel are not compiled: 35 spilled VGPR dwords instead of 98 at the same four waves per SIMD.
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_P     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
