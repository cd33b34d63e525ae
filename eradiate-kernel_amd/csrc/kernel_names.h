// kernel_names.h -- the names of a render kernel ("kernel table"), for the host planning code (render_plan.h) and the
// launchers of the device units (launch.h) alike.  Constants only: it includes nothing.
#pragma once

namespace mtsamd {

// A VARIANT is a kernel formulation: nested per-lane loops, the flat per-lane state machine, or the regrouping machine on LDS rings with
// P paths per workgroup.  A UNIT is the translation unit the kernel comes from: the general kernels (kernels.hip, kernels_spectral.hip)
// or a lean unit (kernels_lean_*.hip), the same kernels compiled without what a scene cannot contain.  mts_stats.kernel_variant carries
// both.  The values are ABI: they never change.
namespace kv {
constexpr int NESTED = 0, FLAT = 1, RING_BASE = 10000, UNIT_STRIDE = 100000;
constexpr int ring(int paths) { return RING_BASE + paths; }
constexpr bool is_ring(int variant) { return variant >= RING_BASE; }
constexpr int ring_paths(int variant) { return variant - RING_BASE; }
constexpr int stat(int variant, int unit) { return variant + UNIT_STRIDE * unit; }        // mts_stats.kernel_variant
constexpr int stat_variant(int kernel_variant) { return kernel_variant % UNIT_STRIDE; }
constexpr int stat_unit(int kernel_variant) { return kernel_variant / UNIT_STRIDE; }
// The `moment` integrator (mts_integrator.moment) renders on the general rgb / mono unit.  Its eleven-channel sample tail is built into
// three formulations -- `volpath` on 1024-path rings, `volpathmis` on 512-path rings, `path` as the flat loop -- with scalar streams and
// without counters; for every other row of the kernel table the nested moment kernel runs.  `variant`: what choose_kernel gave the
// scene; `integrator`: MTS_INTEGRATOR_* (0 path, 1 volpath, 2 volpathmis).  Returns the variant that renders it.
constexpr int moment_variant(int variant, int integrator, bool wavefront, bool counters) {
    return counters || wavefront ? NESTED
         : variant == ring(1024) && integrator == 1 ? variant
         : variant == ring(512) && integrator == 2 ? variant
         : variant == FLAT && integrator == 0 ? variant : NESTED;
}
// A textured scene (mts_scene_desc.textures), or one that holds a blendbsdf, a twosided, a dielectric or a conductor, renders on the general rgb / mono unit as well, in TEX instantiations: `volpath` on
// 1024-path rings in its ring TEX kernel (scalar streams, no counters), `path` on the flat row in the flat TEX loop, every other row
// -- `volpathmis`, wavefront streams, counters, 256-path rings -- in the nested TEX kernel (same functions, same streams: the same film).
// mts_stats.kernel_variant keeps naming the table's row; mts_stats.textured says that this mapping applied.
constexpr int textured_variant(int variant, int integrator, bool wavefront, bool counters) {
    return variant == ring(1024) && integrator == 1 && !wavefront && !counters ? variant
         : variant == FLAT && integrator == 0 ? FLAT : NESTED;
}
} // namespace kv
enum KernelUnit : int { UNIT_GENERAL = 0, UNIT_A = 1, UNIT_B = 2, UNIT_S = 3, UNIT_P = 4, UNIT_PS = 5, UNIT_H = 6, UNIT_C = 7, UNIT_COUNT = 8 };

} // namespace mtsamd
