// kernels_lean_h.hip -- as kernels_lean_b.hip for scenes whose media are all HOMOGENEOUS (rgb / mono): no grid behind volume_eval(), a walked
// primitive list without spheres, no area emitters, no nested blendphase; rpv allowed.  A homogeneous atmosphere over a surface (C2) is one:
// the tracking step keeps neither the slab test nor a grid lookup.
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_H     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
