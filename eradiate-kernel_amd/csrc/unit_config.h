// unit_config.h -- what distinguishes the device units: ONE table, one row per unit ("What a unit is").
//
// kernels.hip is compiled nine times: as it is and through kernels_spectral.hip (the two general units), and through the seven
// kernels_lean_*.hip, each of which sets MTS_UNIT -- a KernelUnit of kernel_names.h by number (kernels.hip holds the numbers below
// against the enum) -- and includes kernels.hip.  Everything else that shapes a unit's kernels is its row here.  Preprocessor only:
// tests/test_unit_config.py reads the table with the host preprocessor and holds it against a table of its own.
#pragma once
#include "dscene.h"                 // MT_*

#define MTS_UNIT_ID_GENERAL 0
#define MTS_UNIT_ID_A 1
#define MTS_UNIT_ID_B 2
#define MTS_UNIT_ID_S 3
#define MTS_UNIT_ID_P 4
#define MTS_UNIT_ID_PS 5
#define MTS_UNIT_ID_H 6
#define MTS_UNIT_ID_C 7
#ifndef MTS_UNIT
#define MTS_UNIT MTS_UNIT_ID_GENERAL
#endif

// SPEC_N  3: rgb / mono, 4: the spectral variant (dmath.h).  namespace: the unit's inline namespace, part of every mangled kernel name.
// suffix  of the unit's launcher (launch.h).  TRAITS: what the unit's scenes promise (dscene.h; the host checks them per scene,
//         render_plan.cpp: KERNEL_UNITS) -- the promised-away branches are not compiled.
// PATH    the unit carries `path` as the flat loop and nothing else, so no kernel reads the columns to its right; 0: the ring
//         kernels of `volpath` and `volpathmis` (the general units: every kernel).
// STEP    MTS_STEP_FAST: the tracking step as straight-line code (volpath_flat.h: step_fast), written for media that are all
//         heterogeneous, grey and on a pair grid (a, b, c: C3 +3.6 %).  The spectral units' step evaluates two four-channel grids and
//         divides per channel, h has no lookup to make unconditional, the general units choose the medium's kind per step.
// CROSS   MTS_CROSS_CLASS: `volpath` sorts null-boundary crossings into a class of their own (volpath_flat.h: cross_class).  Measured on
//         the units of the benchmark scenes (a: C3 +2.5 %, b: C4 +4.1 %) and kept there; elsewhere the class stays empty.
// DRCP    MTS_HOT_DRCP: the hot state holds 1 / d (volpath_flat.h: HotFront).  0: a block forms it from d, and the ring driver's init loop
//         loads the kernel arguments inside its body (MTS_OPAQUE_INIT below) -- measured together, unit by unit.  a, b: the ninth ring
//         needs the 12 KiB, and with the loads ahead of the loop the flagship kernel spills 177 SGPRs (test_abi holds 160); h: C2 +0.2 %
//         with both, -1.3 % with neither; general rgb: 19 spilled VGPRs with 1 / d loaded (test_abi holds 16), 10 without; spectral
//         units and c: -0.7 % (C5S) with both changes, nothing with neither.
// GEOM    MTS_GEOM_LDS: small scenes keep their triangles' attribute rows in LDS (integrator_dev.h; the volpath rings).  a: C3 +2.4 %,
//         h: C2 +0.6 %; b: C4 -0.7 % with it, cause unknown; c's scenes have a BVH, which the table does not serve.
// MIS     MTS_MIS_THREADS of the unit's `volpathmis` ring kernel: one per path, but 768 on the 512 paths of a -- 164 VGPRs there
//         (general: 193), and three waves per SIMD want <= 168 (C3M 375 -> 393).
// BLOCKSTATS_RGB: the diagnostic build (-DMTSAMD_BLOCKSTATS) has no lean units; its general rgb unit stands in for a and b, its
// general spectral unit is the product's.
//      unit                     SPEC_N namespace          suffix     TRAITS     PATH STEP CROSS DRCP GEOM MIS
#define MTS_ROW_GENERAL_RGB      3,     v_rgb,             ,          0,         0,   0,   0,    0,   0,   512
#define MTS_ROW_GENERAL_SPECTRAL 4,     v_spectral,        _spectral, 0,         0,   0,   0,    1,   0,   256
#define MTS_ROW_A                3,     v_rgb_lean_a,      _lean_a,   MT_UNIT_A, 0,   1,   1,    0,   1,   768
#define MTS_ROW_B                3,     v_rgb_lean_b,      _lean_b,   MT_UNIT_B, 0,   1,   1,    0,   0,   512
#define MTS_ROW_C                3,     v_rgb_lean_c,      _lean_c,   MT_UNIT_C, 0,   1,   0,    1,   0,   512
#define MTS_ROW_H                3,     v_rgb_lean_h,      _lean_h,   MT_UNIT_H, 0,   0,   0,    0,   1,   512
#define MTS_ROW_S                4,     v_spectral_lean,   _lean_s,   MT_UNIT_B, 0,   0,   0,    1,   0,   256
#define MTS_ROW_P                3,     v_rgb_lean_p,      _lean_p,   MT_UNIT_P, 1,   0,   0,    1,   0,   512
#define MTS_ROW_PS               4,     v_spectral_lean_p, _lean_ps,  MT_UNIT_P, 1,   0,   0,    1,   0,   256
#define MTS_ROW_BLOCKSTATS_RGB   3,     v_rgb,             ,          0,         0,   0,   1,    0,   1,   512

#if MTS_UNIT == MTS_UNIT_ID_GENERAL && MTS_SPEC_N == 4          // kernels_spectral.hip says no more than this
#undef MTS_SPEC_N
#define MTS_UNIT_ROW MTS_ROW_GENERAL_SPECTRAL
#elif MTS_UNIT == MTS_UNIT_ID_GENERAL && defined(MTSAMD_BLOCKSTATS)
#define MTS_UNIT_ROW MTS_ROW_BLOCKSTATS_RGB
#elif MTS_UNIT == MTS_UNIT_ID_GENERAL
#define MTS_UNIT_ROW MTS_ROW_GENERAL_RGB
#elif defined(MTSAMD_BLOCKSTATS)
#error "the diagnostic build has no lean units (kernels_lean_*.hip compile to empty objects under -DMTSAMD_BLOCKSTATS)"
#elif MTS_UNIT == MTS_UNIT_ID_A
#define MTS_UNIT_ROW MTS_ROW_A
#elif MTS_UNIT == MTS_UNIT_ID_B
#define MTS_UNIT_ROW MTS_ROW_B
#elif MTS_UNIT == MTS_UNIT_ID_C
#define MTS_UNIT_ROW MTS_ROW_C
#elif MTS_UNIT == MTS_UNIT_ID_H
#define MTS_UNIT_ROW MTS_ROW_H
#elif MTS_UNIT == MTS_UNIT_ID_S
#define MTS_UNIT_ROW MTS_ROW_S
#elif MTS_UNIT == MTS_UNIT_ID_P
#define MTS_UNIT_ROW MTS_ROW_P
#elif MTS_UNIT == MTS_UNIT_ID_PS
#define MTS_UNIT_ROW MTS_ROW_PS
#else
#error "MTS_UNIT names no unit of this table"
#endif

// the columns of the unit's row, under the names the code reads
#define MTS_ROW_PICK(column, row) column(row)
#define MTS_ROW_0(a, ...) a
#define MTS_ROW_1(a, b, ...) b
#define MTS_ROW_2(a, b, c, ...) c
#define MTS_ROW_3(a, b, c, d, ...) d
#define MTS_ROW_4(a, b, c, d, e, ...) e
#define MTS_ROW_5(a, b, c, d, e, f, ...) f
#define MTS_ROW_6(a, b, c, d, e, f, g, ...) g
#define MTS_ROW_7(a, b, c, d, e, f, g, h, ...) h
#define MTS_ROW_8(a, b, c, d, e, f, g, h, i, j) i
#define MTS_ROW_9(a, b, c, d, e, f, g, h, i, j) j
#define MTS_CAT2(a, b) a##b
#define MTS_CAT(a, b) MTS_CAT2(a, b)
#define MTS_SPEC_N MTS_ROW_PICK(MTS_ROW_0, MTS_UNIT_ROW)
#define MTS_VARIANT_NS MTS_ROW_PICK(MTS_ROW_1, MTS_UNIT_ROW)
#define MTS_LAUNCHER(name) MTS_CAT(name, MTS_ROW_PICK(MTS_ROW_2, MTS_UNIT_ROW))
#define MTS_TRAITS MTS_ROW_PICK(MTS_ROW_3, MTS_UNIT_ROW)
#define MTS_PATH_ONLY MTS_ROW_PICK(MTS_ROW_4, MTS_UNIT_ROW)
#define MTS_STEP_FAST MTS_ROW_PICK(MTS_ROW_5, MTS_UNIT_ROW)
#define MTS_CROSS_CLASS MTS_ROW_PICK(MTS_ROW_6, MTS_UNIT_ROW)
#define MTS_HOT_DRCP MTS_ROW_PICK(MTS_ROW_7, MTS_UNIT_ROW)
#define MTS_OPAQUE_INIT (!MTS_HOT_DRCP)         // ring_driver.h: M::OPAQUE_INIT of both ring machines
#define MTS_GEOM_LDS MTS_ROW_PICK(MTS_ROW_8, MTS_UNIT_ROW)
#define MTS_MIS_THREADS MTS_ROW_PICK(MTS_ROW_9, MTS_UNIT_ROW)
#if MTS_UNIT != MTS_UNIT_ID_GENERAL
#define MTS_LEAN 1                              // a lean unit: no moment kernels, no per-lane fallbacks, its few functions inline (DEV_CALL_UNLESS_LEAN)
#endif
#if MTS_PATH_ONLY
#define MTS_LEAN_PATH 1
#endif
