// kernels_lean_a.hip -- the regrouping kernels of `volpath` and `volpathmis` (rgb / mono) compiled for scenes that keep EVERY promise of
// integrator_dev.h's scene traits: heterogeneous grey media on pair grids, a walked primitive list without spheres, no area emitters, no
// nested blendphase, no rpv, no grid evaluated through volume_eval().  The metric scene (C3) is one: a kernel without a single call
// (122 VGPRs, no spilled VGPR dword, 28 B of scratch against 384).  Same source as kernels.hip, same arithmetic: the promised-away branches
// are not compiled.  mts_render selects it from HostScene::traits (render_plan.cpp: choose_kernel); MTSAMD_LEAN=0 keeps every scene on the general kernels.
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_A     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
