// kernels.hip -- HIP kernels of the path / volpath render loop for gfx950 (MI355X) and their launchers.
//
// Execution model: one lane per pixel, one wave = an 8x8 Morton tile, one 256-thread workgroup = a
// 16x16 tile of a 32x32 spiral block.  A lane seeds the reference's per-pixel PCG32 stream
// (librender/integrator.cpp:198) and runs all samples of its pixel; path state never leaves
// registers, the scene is read with scalar loads, the only vector memory traffic is the volume
// gathers and one film update per pixel.  Citations are relative to /root/reference.
// Compiled twice into libmtsamd.so: as it is (MTS_SPEC_N = 3: the rgb / mono variants, all kernels) and through kernels_spectral.hip
// (MTS_SPEC_N = 4: the spectral variant: `volpath` on the regrouping machine with 256-path workgroups, `path` per lane; launchers carry
// the suffix _spectral), and once per lean unit through kernels_lean_*.hip (MTS_UNIT).  What a unit is -- its namespace, its launchers'
// suffix, its traits and the switches of its ring kernels -- is one row of unit_config.h (through integrator_dev.h).
#include <hip/hip_runtime.h>
#define PM_TABLES_IN_LDS 1            // pmath.h: LDS copies of the two hot lookup tables; every kernel below fills them first
#include "integrator_dev.h"
#include "volpath_flat.h"
#include "volpathmis_flat.h"
#include "ring_driver.h"
#include "launch.h"
static_assert(MTS_UNIT_ID_GENERAL == mtsamd::UNIT_GENERAL && MTS_UNIT_ID_A == mtsamd::UNIT_A && MTS_UNIT_ID_B == mtsamd::UNIT_B && MTS_UNIT_ID_S == mtsamd::UNIT_S &&
              MTS_UNIT_ID_P == mtsamd::UNIT_P && MTS_UNIT_ID_PS == mtsamd::UNIT_PS && MTS_UNIT_ID_H == mtsamd::UNIT_H && MTS_UNIT_ID_C == mtsamd::UNIT_C &&
              mtsamd::UNIT_COUNT == 8, "unit_config.h numbers the units as kernel_names.h does");

namespace mtsamd {
inline namespace MTS_VARIANT_NS {

// a thread's loop counters -> counters[0..2] of the launch (counting kernel variants)
DEV void flush_counters(unsigned long long *counters, const Counters &cnt) {
    atomicAdd(counters + 0, (unsigned long long) cnt.n_iter);
    atomicAdd(counters + 1, (unsigned long long) cnt.n_lookup);
    atomicAdd(counters + 2, (unsigned long long) cnt.n_nee_step);
}

#if !defined(MTS_LEAN) || defined(MTS_LEAN_PATH)
// librender/integrator.cpp:233-288 + librender/imageblock.cpp:79-172, fused: the sample is splatted
// straight into the film.  With the default box filter a sample lands in its own pixel and is summed
// in registers in sample order (bit-identical to the reference's block accumulation); the rare
// sample that falls on the left/top pixel edge (u == 0) goes to the neighbour through an atomic.
// MOMENT (rgb / mono general unit): the `moment` wrapper's tail, eleven accumulators (splat_moment_t, volpath_flat.h)
// TEX (rgb / mono general unit): BSDF parameters through their textures (integrator_dev.h: HitBsdf)
template <bool COUNT, int INTEG, bool MOMENT = false, int TEX = TEX_NONE>
__device__ __forceinline__ void render_sample(const DScene &sc, Pcg32 &rng, const DBlock &blk, uint32_t lx, uint32_t ly,
                                              float *__restrict__ film, float acc[5], Counters &cnt) {
    const DSensor &se = sc.sensor;
    float px = (float) (lx + (uint32_t) blk.ox), py = (float) (ly + (uint32_t) blk.oy);
    F2 u = rng.next_2d();
    F2 position_sample; position_sample.x = px + u.x; position_sample.y = py + u.y;
    F2 aperture_sample; aperture_sample.x = .5f; aperture_sample.y = .5f;
    if (se.needs_aperture_sample) aperture_sample = rng.next_2d();
    if (se.shutter_open_time > 0.f) (void) rng.next_1d();        // time sample (integrator.cpp:248-250)
#if MTS_SPEC_N == 3
    (void) rng.next_1d();                                       // wavelength sample (integrator.cpp:252), unused in rgb
#else
    SpecCtx cx = make_ctx(sc);
    Spec wav_weight;
    {
        const float wavelength_sample = rng.next_1d();          // integrator.cpp:252 -> Sensor::sample_ray: perspective.cpp:169-182, distant.cpp:311-313
        if (sc.srf >= 0) cx.wl = sample_wavelengths_srf(sc, wavelength_sample, wav_weight);
        else { float w; cx.wl = sample_wavelengths(wavelength_sample, w); wav_weight = spec_s(w); }
    }
#endif
    F2 adjusted;
    adjusted.x = (position_sample.x - (float) se.crop_x) / (float) se.crop_w;
    adjusted.y = (position_sample.y - (float) se.crop_y) / (float) se.crop_h;
    F3 ray_weight;
    DRay ray = sensor_sample_ray(sc, adjusted, aperture_sample, ray_weight);
    bool valid;
#if MTS_SPEC_N == 3
    F3 L = integrator_sample<COUNT, INTEG, TEX>(sc, rng, ray, se.medium, valid, cnt);
#if !defined(MTS_LEAN)
    if constexpr (MOMENT) { splat_moment_t<true>(sc, blk, lx, ly, position_sample, L, ray_weight.x, valid, as_global(film), acc); return; }
#endif
    L = ray_weight * L;
    splat_sample_t<false>(sc, blk, lx, ly, position_sample, L, valid, as_global(film), acc);
#else
    Spec L = integrator_sample<COUNT, INTEG>(sc, rng, ray, se.medium, valid, cnt, cx);
    float aov[2 * 64]; const int na = 2 * sc.bin_count;        // nbins / bins: the wrapped integrator's own result, before the ray weight
    for (int i = 0; i < sc.bin_count; ++i) bin_aovs(sc, L, cx.wl, i, aov[2 * i], aov[2 * i + 1]);
    L = (wav_weight * ray_weight.x) * L;                        // ray_weight = wav_weight (x the sensor's grey weight), integrator.cpp:265
    float xyz[3];
    spectrum_to_xyz(sc.cie, L, cx.wl, xyz);                     // integrator.cpp:266-269
    const float v[5] = { xyz[0], xyz[1], xyz[2], valid ? 1.f : 0.f, 1.f };
    splat_values_t<false>(sc, blk, lx, ly, position_sample, v, as_global(film), acc, aov, na);
#endif
}

// `path` (integrators/path.cpp:100-211) for one pixel as ONE flat loop over path segments with regeneration: a lane whose path has ended
// splats its sample and starts the pixel's next one at once, instead of idling until the longest path of the wave's 64 pixels has ended
// (path lengths under Russian roulette are roughly geometric: the longest of 64 is several times the mean).  One ray_intersect site
// serves camera rays and BSDF-sampled rays alike.  The lane draws exactly the numbers path_sample (integrator_dev.h) draws, in the
// same order, and sums its samples in the same order: bit-identical to the nested formulation and to the CPU restatement.
// Written over the variant's spectrum type: in the spectral build a sample also draws its four wavelengths (from the sensor's response
// function when there is one), carries the bins' AOV values and reaches the film through spectrum_to_xyz, as render_sample above.
template <bool COUNT, bool MOMENT = false, int TEX = TEX_NONE>
__device__ __forceinline__ void path_pixel_flat(const DScene &sc, Pcg32 &rng, const DBlock &blk, uint32_t lx, uint32_t ly, uint32_t sample_count,
                                                float *__restrict__ film, float acc[5], Counters &cnt, const uint32_t *stop_flag) {
    const DSensor &se = sc.sensor;
    const int max_depth = sc.integrator.max_depth, rr_depth = sc.integrator.rr_depth;
    const float px = (float) (lx + (uint32_t) blk.ox), py = (float) (ly + (uint32_t) blk.oy);
    F2 position_sample; float ray_weight = 1.f;
    DRay ray;
    Spec throughput = spec_s(1.f), result = spec_s(0.f);
    F3 ref_p = f3s(0.f);
    float eta = 1.f, emission_weight = 1.f, bs_pdf = 0.f;
    uint32_t bs_type = 0;
    bool valid_ray = false;
    int depth = 0;                                              // 0: the camera ray of a fresh sample has not been traced yet
    uint32_t j = 0;
#if MTS_SPEC_N != 3
    SpecCtx cx = make_ctx(sc);
    Spec wav_weight = spec_s(0.f);
#endif
    auto begin_sample = [&]() {                                 // integrator.cpp:242-264, path.cpp:106-119
        if (se.wavefront) seed_wavefront_sample(rng, se, blk, lx, ly, j);     // gpu_* streams: one per (pixel, sample)
        F2 u = rng.next_2d();
        position_sample.x = px + u.x; position_sample.y = py + u.y;
        F2 aperture_sample; aperture_sample.x = .5f; aperture_sample.y = .5f;
        if (se.needs_aperture_sample) aperture_sample = rng.next_2d();
        if (se.shutter_open_time > 0.f) (void) rng.next_1d();
#if MTS_SPEC_N == 3
        (void) rng.next_1d();                                   // wavelength sample, unused in rgb
#else
        {
            const float wavelength_sample = rng.next_1d();      // integrator.cpp:252 -> Sensor::sample_ray: perspective.cpp:169-182, distant.cpp:311-313
            if (sc.srf >= 0) cx.wl = sample_wavelengths_srf(sc, wavelength_sample, wav_weight);
            else { float w; cx.wl = sample_wavelengths(wavelength_sample, w); wav_weight = spec_s(w); }
        }
#endif
        F2 adjusted;
        adjusted.x = (position_sample.x - (float) se.crop_x) / (float) se.crop_w;
        adjusted.y = (position_sample.y - (float) se.crop_y) / (float) se.crop_h;
        F3 rw;
        ray = sensor_sample_ray(sc, adjusted, aperture_sample, rw);
        ray_weight = rw.x;
        throughput = spec_s(1.f); result = spec_s(0.f); eta = 1.f; emission_weight = 1.f; depth = 0;
    };
    begin_sample();
    for (uint32_t it = 0;; ++it) {
        if ((it & 1023u) == 1023u && stop_requested(stop_flag)) break;      // should_stop(), integrator.h:143-146
        const Hit si = ray_intersect<false, TEX == TEX_INST>(sc, ray);
        const int emitter = hit_emitter<TEX == TEX_INST>(sc, si);
        if (depth == 0) valid_ray = hit_valid(si);               // path.cpp:113-115
        else if (emitter >= 0) {                                 // :193-205: MIS weight of the emitter the BSDF sample found
            Surf sb; sb.wi = -ray.d; sb.sh.n = f3s(0.f);
            if (hit_valid(si)) complete_surface<TEX == TEX_INST>(sc, si, ray.d, sb);
            DirSample ds;                                        // render/records.h:168-174
            ds.p = si.p; ds.n = sb.sh.n; ds.d = si.p - ref_p; ds.dist = norm(ds.d); ds.d = ds.d / ds.dist;
            if (!hit_valid(si)) ds.d = -sb.wi;
            ds.emitter = emitter; ds.pdf = 0.f; ds.delta = false;
            const float emitter_pdf = !(bs_type & F_Delta) ? pdf_emitter_direction(sc, ref_p, ds) : 0.f;
            emission_weight = mis_weight(bs_pdf, emitter_pdf);
        }
        depth += 1;
        // ---- one iteration of the loop of path.cpp:121-207
        if (COUNT) cnt.n_iter++;
        Surf sf; sf.wi = -ray.d;
        if (hit_valid(si)) complete_surface<TEX == TEX_INST>(sc, si, ray.d, sf);
        if (emitter >= 0) result = result + emission_weight * throughput * emitter_eval(sc, emitter, sf.wi.z MTS_CX);
        bool active = hit_valid(si);
        if (depth > rr_depth) {
            float q = pm_min(hmax(throughput) * (eta * eta), .95f);
            active = active && rng.next_1d() < q;
            throughput = throughput * pm_rcp(q);
        }
        bool ended = (uint32_t) depth >= (uint32_t) max_depth || !active;
        if (!ended) {
            const int bsdf_id = sc.shapes[hit_shape<TEX == TEX_INST>(si)].bsdf;
            HitBsdf<TEX> hit_bsdf;
            const DBsdf &bsdf = hit_bsdf.at(sc, bsdf_id, sc.shapes[hit_shape<TEX == TEX_INST>(si)], si, sf.wi);
            bool active_e = (bsdf.flags & F_Smooth) != 0;
            if (active_e) {
                Spec emitter_val;
                DirSample ds = sample_emitter_direction<TEX == TEX_INST>(sc, si.p, rng.next_2d(), true, emitter_val MTS_CX);
                active_e = active_e && ds.pdf != 0.f;
                F3 wo = to_local(sf.sh, ds.d);
                Spec bsdf_val; float bpdf;
                hit_bsdf.eval_pdf(sc, bsdf, sf.wi, wo, bsdf_val, bpdf MTS_CXI(bsdf_id));
                float mis = ds.delta ? 1.f : mis_weight(ds.pdf, bpdf);
                if (active_e) result = result + mis * throughput * bsdf_val * emitter_val;
            }
            float s1 = rng.next_1d(); F2 s2 = rng.next_2d();
            BSDFSample bs;
            Spec bsdf_val = hit_bsdf.sample(sc, bsdf, sf.wi, s1, s2, bs MTS_CXI(bsdf_id));
            throughput = throughput * bsdf_val;
            ended = !any_nonzero(throughput);
            if (!ended) {
                eta *= bs.eta;
                ref_p = si.p; bs_pdf = bs.pdf; bs_type = bs.sampled_type;
                ray = spawn_ray(si.p, to_world(sf.sh, bs.wo));
            }
        }
        if (ended) {                                             // integrator.cpp:265-288: splat, next sample of this pixel
#if MTS_SPEC_N == 3
#if !defined(MTS_LEAN)
            if constexpr (MOMENT) splat_moment_t<true>(sc, blk, lx, ly, position_sample, result, ray_weight, valid_ray, as_global(film), acc);
            else
#endif
            splat_sample_t<false>(sc, blk, lx, ly, position_sample, f3s(ray_weight) * result, valid_ray, as_global(film), acc);
#else
            float aov[2 * 64]; const int na = 2 * sc.bin_count;  // nbins / bins: the wrapped integrator's own result, before the ray weight
            for (int i = 0; i < sc.bin_count; ++i) bin_aovs(sc, result, cx.wl, i, aov[2 * i], aov[2 * i + 1]);
            const Spec L = (wav_weight * ray_weight) * result;   // integrator.cpp:265
            float xyz[3];
            spectrum_to_xyz(sc.cie, L, cx.wl, xyz);              // integrator.cpp:266-269
            const float v[5] = { xyz[0], xyz[1], xyz[2], valid_ray ? 1.f : 0.f, 1.f };
            splat_values_t<false>(sc, blk, lx, ly, position_sample, v, as_global(film), acc, aov, na);
#endif
            if (++j == sample_count) break;
            begin_sample();
        }
    }
}

// librender/integrator.cpp:181-209 (scalar branch) for every block of this launch at once.
// FLAT = true: volpath as the flat state machine of volpath_flat.h (the production kernel of the metric);
// FLAT = false: the nested formulation of integrator_dev.h (path and volpathmis; volpath cross-check, MTSAMD_KERNEL=nested),
// one instantiation per integrator (INTEG = NI_*).
// Written out, not a call of lane_render (below): through it, with the scene by reference, v_rgb::render_kernel<true, false, 0> spills 78 -> 125 VGPRs
// (the `path` kernel <false, true, 0> 98 -> 89); by value the kernels that share it keep their resources but not their text, which this one must in all nine units.
#define MTS_NESTED_WAVES 1
#if MTS_SPEC_N != 3
#define MTS_PATH_WAVES 3      // four-wide spectra: the register budget of four waves per SIMD is not met
#else
#define MTS_PATH_WAVES 4      // measured on the cornell box: 1 -> 1631, 3 -> 1717, 4 -> 2355, 5 -> 1870, 6 -> 1241 Msamples/s
#endif
template <bool COUNT, bool FLAT, int INTEG>
__global__ void __launch_bounds__(256, (FLAT && INTEG != NI_PATH) ? 1 : (INTEG == NI_PATH ? MTS_PATH_WAVES : MTS_NESTED_WAVES)) render_kernel(DScene sc, const DBlock *__restrict__ blocks, uint32_t n_blocks, uint32_t block_size,
                                                     uint32_t sample_count, float *__restrict__ film_base, unsigned long long *__restrict__ counters,
                                                     const uint32_t *__restrict__ stop_flag) {
    // LDS-staged BVH top: the breadth-first top levels of the host-built BVH (dscene.h), shared by the workgroup's traversals
    __shared__ float bvh_top[MTS_BVH_LDS_NODES * 8];
    {
        const int staged = min(sc.bvh_node_count, MTS_BVH_LDS_NODES);
        for (int k = (int) threadIdx.x; k < staged * 8; k += (int) blockDim.x) bvh_top[k] = sc.bvh_nodes[k];
        pm_tables_to_lds(threadIdx.x);
        __syncthreads();
        sc.bvh_lds = bvh_top; sc.bvh_lds_count = staged;
    }
    const uint32_t ppb = block_size * block_size;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = gid / ppb, i = gid - b * ppb;
    if (b >= n_blocks) return;
    const DBlock blk = blocks[b];
    float *__restrict__ film = film_base + (((size_t) blk.film_off_hi << 32) | blk.film_off_lo);      // the film slot of the entry's pass (mts_render)
    const uint32_t lx = compact_bits(i), ly = compact_bits(i >> 1);                           // morton_decode, integrator.cpp:200
    if (lx >= (uint32_t) blk.sx || ly >= (uint32_t) blk.sy) return;
    Pcg32 rng;
    rng.seed(sc.sensor.seed + (uint64_t) blk.id * ppb + i, PCG32_DEFAULT_STREAM);             // sampler.cpp:83-96, integrator.cpp:198
    Counters cnt = {};
#if MTS_SPEC_N == 3
    if (FLAT && INTEG != NI_PATH) {
        __shared__ float cold_lds[C_COUNT * 256];
        ColdStore cold; cold.base = cold_lds + threadIdx.x; cold.stride = 256;
        volpath_pixel_flat<COUNT>(sc, rng, blk, lx, ly, sample_count, film, cold, cnt, stop_flag);
    } else
#endif
    {
        float acc[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
        if (INTEG == NI_PATH && FLAT) path_pixel_flat<COUNT>(sc, rng, blk, lx, ly, sample_count, film, acc, cnt, stop_flag);
        else
        for (uint32_t j = 0; j < sample_count; ++j) {
            // should_stop(), integrator.h:143-146: the reference looks at its flag once per sample; here one lane of the wave reads the
            // host-visible word every 64 samples
            if ((j & 63u) == 63u && stop_requested(stop_flag)) break;
            if (sc.sensor.wavefront) seed_wavefront_sample(rng, sc.sensor, blk, lx, ly, j);       // gpu_* streams: one per (pixel, sample)
            render_sample<COUNT, INTEG>(sc, rng, blk, lx, ly, film, acc, cnt);
        }
        float *dst = film_entry(sc, blk, lx, ly, as_global(film));
        for (int k = 0; k < 5; ++k) atomicAdd(dst + k, acc[k]);
    }
    if (COUNT) flush_counters(counters, cnt);
}

#endif // !MTS_LEAN || MTS_LEAN_PATH

// Asynchronous-regrouping variant of the volpath render kernel (ring_driver.h on the blocks of volpath_flat.h).  The parameter list of every ring
// kernel is MTS_WG_PARAMS, stated next to the WgArgs it mirrors: the block functions re-read it from the kernarg segment with scalar loads.  WG paths are served by NT threads;
// WPE = waves per SIMD the register budget is sized for (512 / WPE VGPRs).
template <bool COUNT, int WG, int NT, int WPE, bool WF = false>
__global__ void __launch_bounds__(NT, WPE) render_kernel_wga(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathRing<COUNT, WG, WF>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
    if (COUNT) flush_counters(counters, cnt);
}

// The same driver for volpathmis (volpathmis_flat.h): four weight matrices per path, 512 paths per workgroup, two waves per SIMD.
template <bool COUNT, bool SPEC, int WG, int NT>
__global__ void __launch_bounds__(NT, NT <= 256 ? 2 : 1) render_kernel_wga_mis(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathMisRing<COUNT, SPEC, WG>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
    if (COUNT) flush_counters(counters, cnt);
}

#if MTS_SPEC_N == 3 && !defined(MTS_LEAN)
// ---- The lane of the per-lane kernels of the `moment` integrator, of textured and of instanced scenes (below): render_kernel's, with the
// sample tail (MOMENT) and the BSDF / traversal (TEX) of the family; `bvh_top` is the kernel's own LDS array.
// The scene record comes BY VALUE.  By reference the body is optimised on its own, before it is inlined, against a record that any store may
// alias: v_rgb::render_kernel_tex<false, true> then spills 344 -> 433 VGPRs, <true, true> 359 -> 417, render_kernel_moment<true, false> 310 -> 312 SGPRs.
template <bool COUNT, bool FLAT, bool MOMENT, int TEX>
__device__ __forceinline__ void lane_render(DScene sc, float *bvh_top, const DBlock *blocks, uint32_t n_blocks, uint32_t block_size,
                                            uint32_t sample_count, float *film_base, unsigned long long *counters, const uint32_t *stop_flag) {
    {                                                          // the BVH's top nodes (an instanced scene: of the SCENE level, which bvh_node_count counts alone) and the pmath tables
        const int staged = min(sc.bvh_node_count, MTS_BVH_LDS_NODES);
        for (int k = (int) threadIdx.x; k < staged * 8; k += (int) blockDim.x) bvh_top[k] = sc.bvh_nodes[k];
        pm_tables_to_lds(threadIdx.x);
        __syncthreads();
        sc.bvh_lds = bvh_top; sc.bvh_lds_count = staged;
    }
    const uint32_t ppb = block_size * block_size;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t b = gid / ppb, i = gid - b * ppb;
    if (b >= n_blocks) return;
    const DBlock blk = blocks[b];
    float *__restrict__ film = film_base + (((size_t) blk.film_off_hi << 32) | blk.film_off_lo);
    const uint32_t lx = compact_bits(i), ly = compact_bits(i >> 1);
    if (lx >= (uint32_t) blk.sx || ly >= (uint32_t) blk.sy) return;
    Pcg32 rng;
    rng.seed(sc.sensor.seed + (uint64_t) blk.id * ppb + i, PCG32_DEFAULT_STREAM);
    Counters cnt = {};
    constexpr int CH = MOMENT ? MTS_MOMENT_CHANNELS : 5;
    float acc[CH] = {};
    if (FLAT) path_pixel_flat<COUNT, MOMENT, TEX>(sc, rng, blk, lx, ly, sample_count, film, acc, cnt, stop_flag);
    else
    for (uint32_t j = 0; j < sample_count; ++j) {
        if ((j & 63u) == 63u && stop_requested(stop_flag)) break;
        if (sc.sensor.wavefront) seed_wavefront_sample(rng, sc.sensor, blk, lx, ly, j);
        render_sample<COUNT, NI_ANY, MOMENT, TEX>(sc, rng, blk, lx, ly, film, acc, cnt);
    }
    float *dst = film_entry_of<MOMENT>(sc, blk, lx, ly, as_global(film));
    for (int k = 0; k < CH; ++k) atomicAdd(dst + k, acc[k]);
    if (COUNT) flush_counters(counters, cnt);
}

// ---- the `moment` integrator (integrators/moment.cpp): the kernels above with the eleven-channel sample tail (splat_moment_t,
// volpath_flat.h), under names of their own -- the plain instantiations stay what they are.  launch_render maps a row of the kernel
// table to one of these (kernel_names.h: kv::moment_variant).
// Per lane.  FLAT: `path` as the flat loop with regeneration; otherwise the nested formulation of whichever integrator the scene has
// (decided at run time: one kernel serves the three), which is also the fallback of every row without a moment instantiation.
template <bool COUNT, bool FLAT>
__global__ void __launch_bounds__(256, FLAT ? MTS_PATH_WAVES : MTS_NESTED_WAVES) render_kernel_moment(DScene sc, const DBlock *__restrict__ blocks, uint32_t n_blocks, uint32_t block_size,
                                                     uint32_t sample_count, float *__restrict__ film_base, unsigned long long *__restrict__ counters,
                                                     const uint32_t *__restrict__ stop_flag) {
    __shared__ float bvh_top[MTS_BVH_LDS_NODES * 8];
    lane_render<COUNT, FLAT, true, TEX_NONE>(sc, bvh_top, blocks, n_blocks, block_size, sample_count, film_base, counters, stop_flag);
}
// The ring machines (render_kernel_wga / render_kernel_wga_mis) with the moment tail in their NEW block; scalar streams, no counters.
template <int WG, int NT, int WPE>
__global__ void __launch_bounds__(NT, WPE) render_kernel_wga_moment(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathRingMoment<WG>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
}
template <bool SPEC, int WG, int NT>
__global__ void __launch_bounds__(NT, NT <= 256 ? 2 : 1) render_kernel_wga_mis_moment(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathMisRingMoment<SPEC, WG>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
}

// ---- textured scenes (mts_scene_desc.textures) and scenes with a blendbsdf or a twosided: the per-lane kernels above with TEX = true -- every BSDF parameter of a hit goes
// through its texture (integrator_dev.h: HitBsdf) -- under a name of their own: the plain instantiations stay what they are.
// launch_render maps a row of the kernel table to one of these or to render_kernel_wga_tex below (kernel_names.h: kv::textured_variant).  FLAT: `path` as the flat
// loop with regeneration; otherwise the nested formulation of whichever integrator the scene has, decided at run time.
template <bool COUNT, bool FLAT>
__global__ void __launch_bounds__(256, FLAT ? MTS_PATH_WAVES : MTS_NESTED_WAVES) render_kernel_tex(DScene sc, const DBlock *__restrict__ blocks, uint32_t n_blocks, uint32_t block_size,
                                                     uint32_t sample_count, float *__restrict__ film_base, unsigned long long *__restrict__ counters,
                                                     const uint32_t *__restrict__ stop_flag) {
    __shared__ float bvh_top[MTS_BVH_LDS_NODES * 8];
    lane_render<COUNT, FLAT, false, TEX_ON>(sc, bvh_top, blocks, n_blocks, block_size, sample_count, film_base, counters, stop_flag);
}

// `volpath` of a textured scene on the 1024-path rings (render_kernel_wga): the machine's SURFACE and BSDF blocks take the hit's BSDF
// record through its textures; scalar streams, no counters.
template <int WG, int NT, int WPE>
__global__ void __launch_bounds__(NT, WPE) render_kernel_wga_tex(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathRingTex<WG>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
}

// SamplingIntegrator::sample for caller-supplied rays (librender/python/integrator_v.cpp:62-78); TEX: of a plain, a textured or an instanced scene
template <int TEX>
__global__ void __launch_bounds__(256) sample_kernel(DScene sc, int32_t n, uint64_t seed_offset, const float *__restrict__ rays /* 6 SoA rows */,
                                                     float *__restrict__ out_rgb, uint8_t *__restrict__ out_valid) {
    pm_tables_to_lds(threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pcg32 rng; rng.seed(sc.sensor.seed + seed_offset + (uint64_t) i, PCG32_DEFAULT_STREAM);
    DRay ray = make_ray(f3(rays[i], rays[n + i], rays[2 * n + i]), f3(rays[3 * n + i], rays[4 * n + i], rays[5 * n + i]), MTS_RAY_EPSILON, pm_inf());
    bool valid; Counters cnt;
    F3 L = integrator_sample<false, NI_ANY, TEX>(sc, rng, ray, sc.sensor.medium, valid, cnt);
    out_rgb[3 * i] = L.x; out_rgb[3 * i + 1] = L.y; out_rgb[3 * i + 2] = L.z; out_valid[i] = valid ? 1 : 0;
}

// Scene::ray_intersect for caller-supplied rays (librender/scene.cpp:117-125).  INST: of an instanced scene (the two-level traversal of the INST kernels
// below); a hit reports the member's index in mts_scene_desc.shapes, a miss -1 -- where the plain kernel reports what ray_intersect left in Hit::shape
template <bool INST>
__global__ void __launch_bounds__(256) intersect_kernel(DScene sc, int32_t n, const float *__restrict__ o, const float *__restrict__ d,
                                                        const float *__restrict__ mint, const float *__restrict__ maxt,
                                                        float *__restrict__ out_t, int32_t *__restrict__ out_shape, int32_t *__restrict__ out_prim,
                                                        float *__restrict__ out_p, float *__restrict__ out_n) {
    pm_tables_to_lds(threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    DRay ray = make_ray(f3(o + 3 * i), f3(d + 3 * i), mint[i], maxt[i]);
    Hit h = ray_intersect<false, INST>(sc, ray);
    F3 nn = f3s(0.f);
    int prim = -1, shape = -1;
    if constexpr (!INST) shape = h.shape;
    if (hit_valid(h)) {
        Surf sf; complete_surface<INST>(sc, h, ray.d, sf); nn = sf.n;
        shape = hit_shape<INST>(h);
        prim = sc.shapes[shape].type == MTS_SHAPE_SPHERE || (INST && sc.shapes[shape].type == MTS_SHAPE_CONE) ? 0 : h.prim;     // both park a float's bits there; cones: INST only
    }
    out_t[i] = h.t; out_shape[i] = shape; out_prim[i] = prim;
    out_p[3 * i] = h.p.x; out_p[3 * i + 1] = h.p.y; out_p[3 * i + 2] = h.p.z;
    out_n[3 * i] = nn.x; out_n[3 * i + 1] = nn.y; out_n[3 * i + 2] = nn.z;
}

// ---- instanced scenes (MTS_SHAPE_INSTANCE; shapes/shapegroup.cpp, shapes/instance.cpp): the kernels of textured scenes above with TEX = TEX_INST -- the two-level
// traversal (integrator_dev.h: inst_intersect), the instance of a hit in the upper bits of Hit::shape, a member's surface carried from group space to world space
// (complete_surface) -- under names of their own: the plain, MOMENT and TEX instantiations stay what they are, and only these pay for the traversal's registers.
// launch_render maps a row of the kernel table to them as to the TEX kernels (kv::textured_variant); mts_stats.textured reports 2.
// The flat loop: two waves per SIMD is what inst_intersect's registers leave it.
template <bool COUNT, bool FLAT>
__global__ void __launch_bounds__(256, FLAT ? 2 : MTS_NESTED_WAVES) render_kernel_inst(DScene sc, const DBlock *__restrict__ blocks, uint32_t n_blocks, uint32_t block_size,
                                                     uint32_t sample_count, float *__restrict__ film_base, unsigned long long *__restrict__ counters,
                                                     const uint32_t *__restrict__ stop_flag) {
    __shared__ float bvh_top[MTS_BVH_LDS_NODES * 8];
    lane_render<COUNT, FLAT, false, TEX_INST>(sc, bvh_top, blocks, n_blocks, block_size, sample_count, film_base, counters, stop_flag);
}
// `volpath` of an instanced scene on the 1024-path rings: the INTERSECT block runs the two-level traversal, the SURFACE and BSDF blocks resolve
// the instance per lane ahead of their waterfalls over shapes; scalar streams, no counters.
template <int WG, int NT, int WPE>
__global__ void __launch_bounds__(NT, WPE) render_kernel_wga_inst(MTS_WG_PARAMS) {
    Counters cnt = {};
    ring_workgroup_async<VolpathRingInst<WG>, NT>((const MTS_CONST_AS void *) __builtin_amdgcn_kernarg_segment_ptr(), cnt);
}

// sample_tea_32 / sample_tea_64 / sample_tea_float32 for n (v0, v1) pairs (core/random.h:75-140)
__global__ void __launch_bounds__(256) tea_kernel(int32_t n, const uint32_t *__restrict__ v0, const uint32_t *__restrict__ v1, int rounds,
                                                  uint32_t *__restrict__ out32, uint64_t *__restrict__ out64, float *__restrict__ outf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out32[i] = sample_tea_32(v0[i], v1[i], rounds); out64[i] = sample_tea_64(v0[i], v1[i], rounds); outf[i] = sample_tea_float32(v0[i], v1[i], rounds);
}
// PCG32Sampler::seed of the wavefront variants (librender/sampler.cpp:83-92): lane idx of a wavefront gets
// rng.seed(tea64(seed_value, idx), tea64(idx, seed_value)); the first `count` next_1d() of every lane are written lane-major.
__global__ void __launch_bounds__(256) wavefront_sampler_kernel(int32_t lanes, uint64_t seed_value, int32_t count, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lanes) return;
    Pcg32 rng;
    rng.seed(sample_tea_64_u64(seed_value, (uint64_t) i), sample_tea_64_u64((uint64_t) i, seed_value));        // UInt64 instantiation, dmath.h
    for (int k = 0; k < count; ++k) out[(size_t) i * count + k] = rng.next_1d();
}

#endif // MTS_SPEC_N == 3
} // inline namespace

// ---------------------------------------------------------------- launchers
#if MTS_SPEC_N == 3 && !defined(MTS_LEAN)
hipError_t launch_tea(int32_t n, const uint32_t *v0, const uint32_t *v1, int rounds, uint32_t *out32, uint64_t *out64, float *outf, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(tea_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, v0, v1, rounds, out32, out64, outf);
    return hipGetLastError();
}
hipError_t launch_wavefront_sampler(int32_t lanes, uint64_t seed_value, int32_t count, float *out, hipStream_t stream) {
    if (lanes <= 0 || count <= 0) return hipSuccess;
    hipLaunchKernelGGL(wavefront_sampler_kernel, dim3((lanes + 255) / 256), dim3(256), 0, stream, lanes, seed_value, count, out);
    return hipGetLastError();
}

// film[i] = ((slot 0 [i] + slot 1 [i]) + slot 2 [i]) + ... : the passes of a render added in pass order, as Film::put(block) adds the
// blocks of pass after pass (integrator.cpp:98-107 -> hdrfilm.cpp:205-217 -> imageblock.cpp:59-77)
__global__ void __launch_bounds__(256) film_sum_slots_kernel(float *__restrict__ film, const float *__restrict__ slots, size_t n, uint32_t count) {
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = slots[i];
    for (uint32_t k = 1; k < count; ++k) v += slots[(size_t) k * n + i];
    film[i] = v;
}
hipError_t launch_film_sum_slots(float *d_film, const float *d_slots, size_t film_floats, uint32_t count, hipStream_t stream) {
    if (film_floats == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(film_sum_slots_kernel, dim3((unsigned) ((film_floats + 255) / 256)), dim3(256), 0, stream, d_film, d_slots, film_floats, count);
    return hipGetLastError();
}

// ---- scene updates (mts_scene_update, capi.cpp): what Volume's constructor derives from a grid's data (scene_host.cpp: grid_stats) and
// build_pair_grid's interleaving, in one pass over a grid that already lies in the scene's device memory.  Memory bound: 16-byte loads and
// stores over a grid-stride loop, a scalar tail for the last count % 4 values; a bounded launch (launch_grid_update), one atomic per workgroup.
__device__ __forceinline__ uint32_t grid_float_key(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : u | 0x80000000u; }
// value k differs bitwise from the same channel of column (0, 0) of its z slice
__device__ __forceinline__ bool grid_differs(const float *__restrict__ grid, uint32_t k, float v, uint32_t plane, uint32_t channels) {
    const uint32_t r = k % plane, c = channels == 1 ? 0u : r % channels;
    return __float_as_uint(grid[k - r + c]) != __float_as_uint(v);
}
__device__ __forceinline__ void grid_pair_store(const GridUpdateJob &j, uint32_t k, float v) {      // voxel k of a single-channel grid -> its slot(s) of the pair grid
    const float o = j.partner[k];
    const float s = j.slot == 0 ? v : o, a = j.slot == 0 ? o : v;
    if (j.nx == 1) *reinterpret_cast<float4 *>(j.pair + 4 * (size_t) k) = make_float4(s, a, s, a);
    else *reinterpret_cast<float2 *>(j.pair + 2 * (size_t) k) = make_float2(s, a);
}
__global__ void __launch_bounds__(256) grid_update_kernel(GridUpdateJob j) {
    __shared__ uint32_t wave_key[4], wave_differs[4];
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u, quads = j.count / 4u;
    uint32_t key = 0u; bool differs = false;
    for (uint32_t q = tid; q < quads; q += stride) {
        const float4 v = reinterpret_cast<const float4 *>(j.grid)[q];
        const float e[4] = { v.x, v.y, v.z, v.w };
        if (j.stats) for (int i = 0; i < 4; ++i) { key = max(key, grid_float_key(e[i])); differs = differs || grid_differs(j.grid, 4u * q + i, e[i], j.plane, j.channels); }
        if (j.pair) {
            if (j.nx == 1) for (int i = 0; i < 4; ++i) grid_pair_store(j, 4u * q + i, e[i]);
            else {                                                  // rows of nx >= 2 voxels: the pair grid is the two grids interleaved value by value
                const float4 o = reinterpret_cast<const float4 *>(j.partner)[q];
                const float4 s = j.slot == 0 ? v : o, a = j.slot == 0 ? o : v;
                float4 *out = reinterpret_cast<float4 *>(j.pair + 8 * (size_t) q);
                out[0] = make_float4(s.x, a.x, s.y, a.y); out[1] = make_float4(s.z, a.z, s.w, a.w);
            }
        }
    }
    if (tid < j.count - 4u * quads) {                              // the tail
        const uint32_t k = 4u * quads + tid; const float v = j.grid[k];
        if (j.stats) { key = max(key, grid_float_key(v)); differs = differs || grid_differs(j.grid, k, v, j.plane, j.channels); }
        if (j.pair) grid_pair_store(j, k, v);
    }
    if (j.pair && tid == 0) {                                       // the padding voxel behind the last row
        const size_t end = 2 * (size_t) (j.nx == 1 ? 2u * j.count : j.count);
        j.pair[end] = 0.f; j.pair[end + 1] = 0.f;
    }
    if (!j.stats) return;                                           // uniform over the launch
    for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t) __shfl_xor((int) key, o, 64));
    const bool wave_diff = __any(differs);
    if ((threadIdx.x & 63u) == 0) { wave_key[threadIdx.x >> 6] = key; wave_differs[threadIdx.x >> 6] = wave_diff ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(j.stats, max(max(wave_key[0], wave_key[1]), max(wave_key[2], wave_key[3])));
        if (wave_differs[0] | wave_differs[1] | wave_differs[2] | wave_differs[3]) atomicAnd(j.stats + 1, 0u);
    }
}
hipError_t launch_grid_update(const GridUpdateJob &job, int compute_units, hipStream_t stream) {
    if (job.count == 0 || !job.grid || (job.pair && (!job.partner || job.channels != 1 || job.nx == 0)) || job.plane == 0 || job.channels == 0) return hipErrorInvalidValue;
    // enough workgroups to fill the device (eight of 256 threads per CU), never more than the data gives work to
    const uint32_t quads = job.count / 4u, wanted = (quads + 255u) / 256u, bound = (uint32_t) (compute_units > 0 ? compute_units : 256) * 8u;
    hipLaunchKernelGGL(grid_update_kernel, dim3(wanted < 1u ? 1u : (wanted < bound ? wanted : bound)), dim3(256), 0, stream, job);
    return hipGetLastError();
}

size_t render_workspace_floats(uint64_t threads, int variant) {
    if (!kv::is_ring(variant)) return 0;
    const uint64_t wg = (uint64_t) kv::ring_paths(variant), padded = (threads + wg - 1) / wg * wg;
    return (size_t) padded * MTS_COLD_RECORD + 32;      // workgroup drivers: one 128-byte record per path
}

#endif // MTS_SPEC_N == 3

// ---- the render launchers: one per translation unit (launch.h), each choosing among the kernels of its unit by a.variant (render_plan.cpp: KERNEL_ROWS)
typedef void (*WgKernel)(DScene, const DBlock *, uint32_t, uint32_t, uint32_t, float *, float *, uint32_t, unsigned long long *,
                         const uint32_t *, const uint32_t *, uint32_t);
typedef void (*LaneKernel)(DScene, const DBlock *, uint32_t, uint32_t, uint32_t, float *, unsigned long long *, const uint32_t *);
#define MTS_BY_COUNT(kernel, ...) (a.count ? kernel<true, __VA_ARGS__> : kernel<false, __VA_ARGS__>)
// the regrouping kernels: `wg` paths per workgroup served by `nt` threads; the cold records of the launch's paths are `stride` apart
static hipError_t launch_wg(const RenderArgs &a, uint64_t threads, uint32_t wg, uint32_t nt, WgKernel k) {
    const uint32_t grid = (uint32_t) ((threads + wg - 1) / wg), stride = grid * wg;
    hipLaunchKernelGGL(k, dim3(grid), dim3(nt), 0, a.stream, *a.sc, a.blocks, a.n_blocks, a.block_size, a.sample_count, a.film, a.workspace, stride,
                       a.counters, a.stop_flag, a.tiles, a.n_tiles);
    return hipGetLastError();
}
// the per-lane kernels: one thread per pixel
static hipError_t launch_lane(const RenderArgs &a, uint64_t threads, LaneKernel k) {
    hipLaunchKernelGGL(k, dim3((uint32_t) ((threads + 255) / 256)), dim3(256), 0, a.stream, *a.sc, a.blocks, a.n_blocks, a.block_size, a.sample_count,
                       a.film, a.counters, a.stop_flag);
    return hipGetLastError();
}

hipError_t MTS_LAUNCHER(launch_render)(const RenderArgs &a) {
    if (a.n_blocks == 0) return hipSuccess;
    // cost-sorted tiles (regrouping kernels only): the launch covers n_tiles slots of 16 paths instead of the blocks' concatenated Morton orders
    const uint64_t threads = a.tiles != nullptr ? (uint64_t) a.n_tiles * MTS_TILE_PIXELS : (uint64_t) a.n_blocks * a.block_size * a.block_size;
    if (a.tiles != nullptr && !kv::is_ring(a.variant)) return hipErrorInvalidConfiguration;
    if (threads + 1024 >= ((uint64_t) 1 << 32)) return hipErrorInvalidValue;      // thread and path indices are 32 bit (mts_render launches in chunks)
    const int integ = a.sc->integrator.type;
    const bool volpath = integ == MTS_INTEGRATOR_VOLPATH, mis = integ == MTS_INTEGRATOR_VOLPATHMIS, spec_mis = a.sc->integrator.use_spectral_mis != 0;
#if defined(MTS_LEAN)
    if (a.moment || a.textured || a.instanced) return hipErrorInvalidConfiguration;      // a moment, textured or instanced scene presents no traits: the general unit renders it
#endif
#if defined(MTS_LEAN_PATH)    // kernels_lean_p.hip / _ps.hip: `path` as the flat loop with regeneration, nothing else
    (void) volpath; (void) mis; (void) spec_mis;
    if (a.variant == kv::FLAT && integ == MTS_INTEGRATOR_PATH) return launch_lane(a, threads, MTS_BY_COUNT(render_kernel, true, NI_PATH));
    return hipErrorInvalidConfiguration;
#elif defined(MTS_LEAN)       // the other lean units: the regrouping machines of `volpath` and of `volpathmis` with spectral MIS, nothing else
    if (a.sc->sensor.wavefront) return hipErrorInvalidConfiguration;
#if MTS_SPEC_N != 3           // the spectral variant's machines: 256-path workgroups
    // register budget of three waves per SIMD (three 256-path workgroups per CU): with the spectral grid lookups inline the allocator needs the bound
    if (a.variant == kv::ring(256) && volpath) return launch_wg(a, threads, 256, 256, MTS_BY_COUNT(render_kernel_wga, 256, 256, 3));
    if (a.variant == kv::ring(256) && mis && spec_mis) return launch_wg(a, threads, 256, MTS_MIS_THREADS, MTS_BY_COUNT(render_kernel_wga_mis, true, 256, MTS_MIS_THREADS));
#else
    if (a.variant == kv::ring(1024) && volpath) return launch_wg(a, threads, 1024, 1024, MTS_BY_COUNT(render_kernel_wga, 1024, 1024, 4));
    // the 512 paths are served by as many threads as the unit's kernel has registers for (unit_config.h: 768 in unit a)
    if (a.variant == kv::ring(512) && mis && spec_mis) return launch_wg(a, threads, 512, MTS_MIS_THREADS, MTS_BY_COUNT(render_kernel_wga_mis, true, 512, MTS_MIS_THREADS));
#endif
    return hipErrorInvalidConfiguration;
#else                         // the general kernels
#if MTS_SPEC_N == 3
    // The kernel families with names of their own: the `moment` wrapper (it goes first), instanced scenes -- mapped from the table's row as textured scenes are,
    // to the INST kernels -- and textured scenes.  a.variant is kv::moment_variant() or kv::textured_variant() of the table's row (capi.cpp).
    if (a.moment || a.instanced || a.textured) {
        if (!a.moment && a.instanced && (!a.textured || a.sc->instances == nullptr)) return hipErrorInvalidConfiguration;
        const bool wavefront = a.sc->sensor.wavefront != 0;
        if (a.variant != (a.moment ? kv::moment_variant(a.variant, integ, wavefront, a.count) : kv::textured_variant(a.variant, integ, wavefront, a.count))) return hipErrorInvalidConfiguration;
        struct Family { WgKernel ring; LaneKernel flat, nested; };      // a family's 1024-path ring kernel, flat `path` loop and nested kernel
        const Family f = a.moment    ? Family{ render_kernel_wga_moment<1024, 1024, 4>, render_kernel_moment<false, true>, MTS_BY_COUNT(render_kernel_moment, false) }   // its flat row never counts (kv::moment_variant)
                       : a.instanced ? Family{ render_kernel_wga_inst<1024, 1024, 4>, MTS_BY_COUNT(render_kernel_inst, true), MTS_BY_COUNT(render_kernel_inst, false) }
                                     : Family{ render_kernel_wga_tex<1024, 1024, 4>, MTS_BY_COUNT(render_kernel_tex, true), MTS_BY_COUNT(render_kernel_tex, false) };
        if (a.variant == kv::ring(1024)) return launch_wg(a, threads, 1024, 1024, f.ring);
        if (a.variant == kv::ring(512))                        // `moment` alone: kv::textured_variant() maps to no such ring
            return launch_wg(a, threads, 512, 512, spec_mis ? render_kernel_wga_mis_moment<true, 512, 512> : render_kernel_wga_mis_moment<false, 512, 512>);
        return launch_lane(a, threads, a.variant == kv::FLAT ? f.flat : f.nested);
    }
    if (kv::is_ring(a.variant) && volpath) {                      // asynchronous regrouping
        if (a.sc->sensor.wavefront)                           // gpu_* streams: the instantiation that recomputes the generator's increment (wg_block, WF)
            return a.variant == kv::ring(1024) ? launch_wg(a, threads, 1024, 1024, MTS_BY_COUNT(render_kernel_wga, 1024, 1024, 4, true)) : hipErrorInvalidConfiguration;
        if (a.variant == kv::ring(1024)) return launch_wg(a, threads, 1024, 1024, MTS_BY_COUNT(render_kernel_wga, 1024, 1024, 4));
        if (a.variant == kv::ring(256)) return launch_wg(a, threads, 256, 256, MTS_BY_COUNT(render_kernel_wga, 256, 256, 4));
        return hipErrorInvalidConfiguration;
    }
    if (kv::is_ring(a.variant) && mis) {                          // the same machinery, 512 or 256 paths per workgroup
        if (a.variant == kv::ring(512))
            return launch_wg(a, threads, 512, MTS_MIS_THREADS, spec_mis ? MTS_BY_COUNT(render_kernel_wga_mis, true, 512, MTS_MIS_THREADS) : MTS_BY_COUNT(render_kernel_wga_mis, false, 512, MTS_MIS_THREADS));
        if (a.variant == kv::ring(256))
            return launch_wg(a, threads, 256, 256, spec_mis ? MTS_BY_COUNT(render_kernel_wga_mis, true, 256, 256) : MTS_BY_COUNT(render_kernel_wga_mis, false, 256, 256));
        return hipErrorInvalidConfiguration;
    }
    if (a.variant != kv::NESTED && volpath) return launch_lane(a, threads, MTS_BY_COUNT(render_kernel, true, NI_VOLPATH));     // the flat state machine per lane
#else
    if (a.moment || a.textured || a.instanced) return hipErrorInvalidConfiguration;      // rgb / mono only (scene_host.cpp refuses the description)
    // four-wide state: `volpath` 42 hot dwords per path; `volpathmis` 69 with spectral MIS (round 4: the path's matrices are parked during
    // walks), 53 without -- 256 paths per workgroup, two or three workgroups per CU
    if (kv::is_ring(a.variant) && volpath)
        return a.variant == kv::ring(256) ? launch_wg(a, threads, 256, 256, MTS_BY_COUNT(render_kernel_wga, 256, 256, 2)) : hipErrorInvalidConfiguration;
    if (kv::is_ring(a.variant) && mis)
        return a.variant == kv::ring(256) ? launch_wg(a, threads, 256, MTS_MIS_THREADS, spec_mis ? MTS_BY_COUNT(render_kernel_wga_mis, true, 256, MTS_MIS_THREADS) : MTS_BY_COUNT(render_kernel_wga_mis, false, 256, MTS_MIS_THREADS))
                                  : hipErrorInvalidConfiguration;
#endif
    if (integ == MTS_INTEGRATOR_PATH)                         // flat: one loop over path segments with regeneration (path_pixel_flat)
        return launch_lane(a, threads, a.variant != kv::NESTED ? MTS_BY_COUNT(render_kernel, true, NI_PATH) : MTS_BY_COUNT(render_kernel, false, NI_PATH));
    if (volpath) return launch_lane(a, threads, MTS_BY_COUNT(render_kernel, false, NI_VOLPATH));
    return launch_lane(a, threads, spec_mis ? MTS_BY_COUNT(render_kernel, false, NI_VOLPATHMIS) : MTS_BY_COUNT(render_kernel, false, NI_VOLPATHMIS_NOSPEC));
#endif
}
#undef MTS_BY_COUNT

#if MTS_SPEC_N == 3 && !defined(MTS_LEAN)

hipError_t launch_sample(const DScene &sc, int32_t n, uint64_t seed_offset, const float *d_rays, float *d_rgb, uint8_t *d_valid, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (sc.instances != nullptr && sc.bsdf_tex == nullptr) return hipErrorInvalidConfiguration;      // an instanced scene renders as a textured one
    hipLaunchKernelGGL(sc.instances != nullptr ? sample_kernel<TEX_INST> : sc.bsdf_tex != nullptr ? sample_kernel<TEX_ON> : sample_kernel<TEX_NONE>,
                       dim3((n + 255) / 256), dim3(256), 0, stream, sc, n, seed_offset, d_rays, d_rgb, d_valid);
    return hipGetLastError();
}

hipError_t launch_intersect(const DScene &sc, int32_t n, const float *o, const float *d, const float *mint, const float *maxt,
                            float *t, int32_t *shape, int32_t *prim, float *p, float *nn, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sc.instances != nullptr ? intersect_kernel<true> : intersect_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, stream, sc, n, o, d, mint, maxt, t, shape, prim, p, nn);
    return hipGetLastError();
}
#endif // MTS_SPEC_N == 3

#if MTS_SPEC_N != 3 && !defined(MTS_LEAN)
// SamplingIntegrator::sample in the spectral variant (librender/python/integrator_v.cpp:62-78): the caller's rays carry their wavelengths
__global__ void __launch_bounds__(256) sample_spectral_kernel(DScene sc, int32_t n, uint64_t seed_offset, const float *__restrict__ rays /* 6 SoA rows */,
                                                              const float *__restrict__ wavelengths /* 4 per ray */,
                                                              float *__restrict__ out_spec, uint8_t *__restrict__ out_valid) {
    pm_tables_to_lds(threadIdx.x);
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pcg32 rng; rng.seed(sc.sensor.seed + seed_offset + (uint64_t) i, PCG32_DEFAULT_STREAM);
    DRay ray = make_ray(f3(rays[i], rays[n + i], rays[2 * n + i]), f3(rays[3 * n + i], rays[4 * n + i], rays[5 * n + i]), MTS_RAY_EPSILON, pm_inf());
    SpecCtx cx = make_ctx(sc);
    cx.wl = spec4(wavelengths[4 * i], wavelengths[4 * i + 1], wavelengths[4 * i + 2], wavelengths[4 * i + 3]);
    bool valid; Counters cnt;
    const Spec L = integrator_sample<false>(sc, rng, ray, sc.sensor.medium, valid, cnt, cx);
    out_spec[4 * i] = L.x; out_spec[4 * i + 1] = L.y; out_spec[4 * i + 2] = L.z; out_spec[4 * i + 3] = L.w; out_valid[i] = valid ? 1 : 0;
}

hipError_t launch_sample_spectral(const DScene &sc, int32_t n, uint64_t seed_offset, const float *d_rays, const float *d_wavelengths, float *d_spec, uint8_t *d_valid,
                                  hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(sample_spectral_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, sc, n, seed_offset, d_rays, d_wavelengths, d_spec, d_valid);
    return hipGetLastError();
}
#endif

} // namespace mtsamd

#if defined(MTSAMD_BLOCKSTATS)
// diagnostic build only (python eradiate-kernel_amd/build.py with MTSAMD_EXTRA_FLAGS=-DMTSAMD_BLOCKSTATS); one copy per variant
#if MTS_SPEC_N == 3
extern "C" int mts_debug_blockstats(unsigned long long *out32, int reset) {
#else
extern "C" int mts_debug_blockstats_spectral(unsigned long long *out32, int reset) {
#endif
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(mtsamd::g_blockstats), 48 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) { unsigned long long z[48] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(mtsamd::g_blockstats), z, sizeof(z)) != hipSuccess) return 1; }
    return 0;
}
#endif
