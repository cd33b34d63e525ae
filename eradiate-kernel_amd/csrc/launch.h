// launch.h -- host-callable launchers of the kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include "dscene.h"
#include "kernel_names.h"

namespace mtsamd {

// One launch of a render kernel over `n_blocks` spiral blocks, as mts_render (capi.cpp) hands it to every render launcher below.
// variant: kernel_names.h's kv names; a ring variant needs a workspace of render_workspace_floats() floats for the cold path state.
struct RenderArgs {
    const DScene *sc;
    const DBlock *blocks; uint32_t n_blocks, block_size, sample_count;
    float *film; unsigned long long *counters; bool count; int variant; float *workspace;
    const uint32_t *stop_flag;                      // host-visible word polled by the kernels: non-zero = stop
    const uint32_t *tiles; uint32_t n_tiles;        // cost-sorted tiles of the regrouping kernels (volpath_flat.h, WgArgs::tiles) or NULL
    hipStream_t stream;
    bool moment;                                    // the `moment` integrator's eleven-channel film (general rgb / mono unit only; variant = kv::moment_variant())
    bool textured;                                  // the scene has textures, a blendbsdf or a twosided (general rgb / mono unit only; variant = kv::textured_variant())
    bool instanced;                                 // the scene has instances (DScene::instances) or a cone: the INST kernels of the general rgb / mono unit; `textured` is set as well
};
typedef hipError_t (*RenderLauncher)(const RenderArgs &);
size_t render_workspace_floats(uint64_t paths, int variant);
// the general kernels of the rgb / mono variants (kernels.hip) and of the spectral variant (kernels_spectral.hip)
hipError_t launch_render(const RenderArgs &a);
hipError_t launch_render_spectral(const RenderArgs &a);
// the lean translation units (kernels_lean_*.hip), for scenes that keep the promises of their traits (integrator_dev.h: MTS_TRAITS);
// anything else: hipErrorInvalidConfiguration.  Which kernels each carries and what it promises: render_plan.cpp, KERNEL_ROWS / KERNEL_UNITS
hipError_t launch_render_lean_a(const RenderArgs &a);
hipError_t launch_render_lean_b(const RenderArgs &a);
hipError_t launch_render_lean_c(const RenderArgs &a);
hipError_t launch_render_lean_h(const RenderArgs &a);
hipError_t launch_render_lean_s(const RenderArgs &a);
hipError_t launch_render_lean_p(const RenderArgs &a);
hipError_t launch_render_lean_ps(const RenderArgs &a);
// film = sum over k < count of the film-sized slot k of d_slots, added in slot order (the passes of a render: capi.cpp)
hipError_t launch_film_sum_slots(float *d_film, const float *d_slots, size_t film_floats, uint32_t count, hipStream_t stream);
// One pass over a grid a scene update has just written (mts_scene_update, capi.cpp): the statistics the volume's constructor
// derives from the data and, where a medium keeps the grid interleaved with its partner, that pair grid (DMedium::pair_grid).
struct GridUpdateJob {
    const float *grid;          // the dirty grid in the scene's device memory: `count` floats, z slices of `plane` floats, voxels of `channels`
    uint32_t count, plane, channels;
    uint32_t *stats;            // NULL, or two words: [0] atomicMax of the order-preserving key of every value (grid_key_to_float), [1] set to 0
                                // when some column differs bitwise from column (0, 0) of its slice; the caller presets { 0, 1 }
    float *pair;                // NULL, or the pair grid `grid` belongs to (single-channel grids only) ...
    const float *partner;       // ... the other grid of the pair, and which of the two slots of a voxel `grid` fills (0 sigma_t, 1 albedo)
    uint32_t slot, nx;          // nx == 1: the column is stored twice (scene_host.cpp: build_pair_grid)
};
hipError_t launch_grid_update(const GridUpdateJob &job, int compute_units, hipStream_t stream);
// the value behind a key of GridUpdateJob::stats[0]: keys order like the floats they stand for (-0 below +0; NaNs are outside the contract)
inline float grid_key_to_float(uint32_t key) { const uint32_t u = (key & 0x80000000u) ? key ^ 0x80000000u : ~key; float f; __builtin_memcpy(&f, &u, 4); return f; }
hipError_t launch_sample(const DScene &sc, int32_t n, uint64_t seed_offset, const float *d_rays, float *d_rgb, uint8_t *d_valid, hipStream_t stream);
// spectral variant (kernels_spectral.hip): per-ray wavelengths (4 n floats), four-wide result
hipError_t launch_sample_spectral(const DScene &sc, int32_t n, uint64_t seed_offset, const float *d_rays, const float *d_wavelengths, float *d_spec, uint8_t *d_valid,
                                  hipStream_t stream);
hipError_t launch_intersect(const DScene &sc, int32_t n, const float *o, const float *d, const float *mint, const float *maxt,
                            float *t, int32_t *shape, int32_t *prim, float *p, float *nn, hipStream_t stream);

hipError_t launch_tea(int32_t n, const uint32_t *v0, const uint32_t *v1, int rounds, uint32_t *out32, uint64_t *out64, float *outf, hipStream_t stream);
hipError_t launch_wavefront_sampler(int32_t lanes, uint64_t seed_value, int32_t count, float *out, hipStream_t stream);

} // namespace mtsamd
