// kernels_lean_s.hip -- as kernels_lean_b.hip for the spectral variant (gpu_spectral): the 256-path regrouping kernels of `volpath` and
// `volpathmis` for scenes whose media are all heterogeneous with two gridvolume_spectral grids on one geometry and spectral interval, with a
// walked primitive list without spheres, no area emitters and no nested blendphase (rpv and blend-weight grids allowed): the layered
// atmosphere as Eradiate renders it (C5S, C5SB under nbins, C5SM under volpathmis).
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_S     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
