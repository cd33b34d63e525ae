// kernels_lean_c.hip -- as kernels_lean_b.hip for scenes WITH a BVH (more than 40 primitives: mesh canopies, many rectangles) under
// heterogeneous grey media on pair grids: no spheres, no area emitters, no nested blendphase; rpv, blend-weight grids and the BVH allowed.
// The traversal stays the one real function of the kernel (bvh_intersect: its loop keeps its registers out of the blocks that call it).
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_C     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
