// kernels_lean_ps.hip -- kernels_lean_p.hip for the spectral variant (gpu_spectral): `path` as the flat loop, four wavelengths per sample.
#if !defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT MTS_UNIT_ID_PS     // unit_config.h: this unit's row of the table
#include "kernels.hip"
#endif
