// volpath_flat.h -- volpath (integrators/volpath.cpp:38-465) as ONE flat state machine over explicit path state.
//
// Why: the reference nests three loops (main loop :72, NEE ratio tracking :282, direct-light walk :385).
// Compiled as written, a wave serialises them: while a few lanes run an inner tracking loop to
// completion the other lanes of the wave idle.  Here every path carries (mode, state); the work is cut
// into small blocks (INTERSECT, MEDIUM step, SCATTER, walk SURFACE step, main SURFACE + BSDF, PHASE, NEW
// sample) and a path advances by one block at a time -- whichever of the three reference loops that block
// belongs to -- so the expensive block (free-flight sample + grid gathers) is shared by all of them.
//
// Two drivers schedule the blocks:
//   1. volpath_pixel_flat: one lane = one pixel, state in registers, per-wave census (__ballot/__popcll)
//      and a vote for the block most lanes wait for (measured: ~40 % of the lanes served per block).
//   2. ring_workgroup_async (ring_driver.h, shared with volpathmis_flat.h): the hot state of a workgroup's paths lives in LDS
//      (struct of arrays), one LDS ring of path ids per block class; a wave claims 64 paths that wait for the same block (wg_block), runs
//      it with every lane active, and appends the paths to the rings of their next blocks.  No barriers, no sort.
//      (A barrier-synchronised counting-sort driver was measured at half the speed and removed; so was a lane-affine driver
//      with mask claims instead of rings: 365 vs 546 Msamples/s on C3)
//
// The random draws happen in exactly the order of the scalar_rgb variant (SURVEY.md 8(a')); results are
// bit-identical to the nested formulation in integrator_dev.h and to the CPU restatement.
// Citations are relative to /root/reference.
#pragma once
#include "integrator_dev.h"

namespace mtsamd {
inline namespace MTS_VARIANT_NS {

// The machine is written once for both builds (MTS_SPEC_N = 3: rgb / mono, 4: spectral).  In the rgb build `Spec` is F3, the
// wavelength context is an empty struct and the macros below vanish, so its kernels are compiled from the same expressions as ever.
#if MTS_SPEC_N == 3
#define MTS_CX
#define MTS_CXI(id)
#define MTS_SPEC_DW 3
#else
#define MTS_CX , cx
#define MTS_CXI(id) , cx, (id)
#define MTS_SPEC_DW 4
#endif

#if MTS_SPEC_N == 3
#define MTS_FILM_STRIDE(sc) ((size_t) 5)
#else
#define MTS_FILM_STRIDE(sc) ((size_t) (sc).film_channels)          // X, Y, Z, A, W (+ two AOV channels per spectral bin: nbins / bins)
#endif
// A block that runs a path's NEXT block in the same visit (wg_block, mis_block) saves a ring push, a claim and an LDS round trip of the
// state, but what runs in place runs on the lanes that want it only.  One such continuation is built in: walk SURFACE twice -- a walk
// that leaves through a boundary face with nothing behind it (queue_intersection: the new ray misses the scene's box, no INTERSECT
// visit) comes straight back to this class, only to end; its second round is a handful of instructions (C3 547 -> 569 Msamples/s).
// Four others (the PHASE sample after the ended walk, the walk's SURFACE steps and SCATTER inside the MEDIUM blocks, main-path SURFACE
// twice) ran real work on a thinned wave and measured slower; they were removed with their switch.
#define MTS_REPEAT_MIN_W 32        // MTS_REPEAT_MIN for the walks' class: 16 and 48 measured 539 / 265 and 536 / 265
#define MTS_REPEAT_MIN 32          // lanes that must stay in a MEDIUM class for the block to run again in place (wg_block)

enum : uint32_t { S_TOP = 0, S_MED = 1, S_SURF = 2, S_PHASE = 3, S_BSDF = 4, S_DIRB = 5, S_NEW = 6, S_DONE = 7, S_SCATTER = 8,
                  S_ENDNEE = 9, S_ENDDIR0 = 10 };   // transient (workgroup drivers): end_nee / end_direct(0, 0) still to run on the full state
enum : uint32_t { M_MAIN = 0, M_NEE = 1, M_DIR = 2 };
enum : uint32_t { FL_ALIVE = 1, FL_VALID_RAY = 2, FL_SPEC_CHAIN = 4, FL_NEEDS_INT = 8, FL_FROM_MEDIUM = 16 };

// MTS_STEP_FAST (unit_config.h: lean units a, b, c): the tracking step of the ring driver as straight-line code
// (VolpathMachine::step_fast).  It relies on media that are all heterogeneous, grey and on a pair grid:
static_assert(!MTS_STEP_FAST || ((MTS_TRAITS & MT_MEDIA) && MTS_SPEC_N == 3), "step_fast is written for MT_MEDIA in the rgb / mono build");
// Every other unit keeps blk_med + top + classify in wg_block.

// Result of one free-flight sample (librender/medium.cpp:34-75); sigma_n is derived by the caller
// (heterogeneous.cpp:46: combined - sigma_t, homogeneous.cpp:44: 0).
struct MedStep { float t, mint; F3 p; Spec sigma_t, sigma_s, combined; uint32_t info; float inv_combined /* DMedium::inv_max_density */; };

// x / d by the majorant through rd = DMedium::inv_max_density: pm_div_by_invariant (pmath.h), the IEEE quotient bit for bit
// (tests/test_pmath.py::test_div_by_invariant_*, tests/test_gpu_pmath.py::test_div_by_invariant_*; film level:
// tests/test_gpu_numeric_edges.py).  rd == 0: plain division.
DEV float div_by_invariant(float x, float d, float rd) { return pm_div_by_invariant(x, d, rd); }
DEV Spec div_by_invariant(Spec x, Spec d, float rd) {          // every channel of d holds the same value when rd != 0
    if (rd == 0.f) return x / d;
#if MTS_SPEC_N == 3
    return f3(div_by_invariant(x.x, d.x, rd), div_by_invariant(x.y, d.x, rd), div_by_invariant(x.z, d.x, rd));
#else
    return spec4(div_by_invariant(x.x, d.x, rd), div_by_invariant(x.y, d.x, rd), div_by_invariant(x.z, d.x, rd), div_by_invariant(x.w, d.x, rd));
#endif
}
enum : uint32_t { MI_HOMOGENEOUS = 1, MI_SPECTRAL = 2, MI_SAMPLE_EMITTERS = 4, MI_GREY = 8, MI_PHASE_SHIFT = 8 + 8 };

#if defined(MTSAMD_BLOCKSTATS)
__device__ unsigned long long g_blockstats[48];    // class b < 12: [b] executions, [12+b] lanes served, [24+b] cycles; [36..41] MEDIUM segments, [42] idle, [43] push, [44] claim / vote
#endif

// textures/grid3d.cpp:259-341 split in two: cell coordinates / weights (shared by grids with the same
// transform and resolution) and the 8 gathers + trilinear blend of one grid.
struct GridCell { int32_t r00, r10, r01, r11, x0, x1; F3 w0, w1; };
DEV GridCell grid_cell_clamp(const float *w2l, int affine, int nx, int ny, int nz, int sx /* voxels per stored row */, F3 p_world) {      // clamp mode (pair grids)
    F3 p = affine ? mat_point_affine(w2l, p_world) : mat_point(w2l, p_world);
    p = f3(pm_fma(p.x, (float) nx, -.5f), pm_fma(p.y, (float) ny, -.5f), pm_fma(p.z, (float) nz, -.5f));
    int ix = (int) pm_floor(p.x), iy = (int) pm_floor(p.y), iz = (int) pm_floor(p.z);
    GridCell c;
    c.w1 = p - f3((float) ix, (float) iy, (float) iz); c.w0 = f3(1.f - c.w1.x, 1.f - c.w1.y, 1.f - c.w1.z);
    c.x0 = min(max(ix, 0), nx - 1); c.x1 = min(max(ix + 1, 0), nx - 1);                                  // grid3d.cpp:234-250, clamp
    int y0 = min(max(iy, 0), ny - 1), y1 = min(max(iy + 1, 0), ny - 1), z0 = min(max(iz, 0), nz - 1), z1 = min(max(iz + 1, 0), nz - 1);
    c.r00 = (z0 * ny + y0) * sx; c.r10 = (z0 * ny + y1) * sx; c.r01 = (z1 * ny + y0) * sx; c.r11 = (z1 * ny + y1) * sx;
    return c;
}
DEV GridCell grid_cell(const DVolume &v, F3 p_world) {
    F3 p = v.affine ? mat_point_affine(v.w2l, p_world) : mat_point(v.w2l, p_world);
    const int nx = v.nx, ny = v.ny, nz = v.nz;
    p = f3(pm_fma(p.x, (float) nx, -.5f), pm_fma(p.y, (float) ny, -.5f), pm_fma(p.z, (float) nz, -.5f));
    int ix = (int) pm_floor(p.x), iy = (int) pm_floor(p.y), iz = (int) pm_floor(p.z);
    GridCell c;
    c.w1 = p - f3((float) ix, (float) iy, (float) iz); c.w0 = f3(1.f - c.w1.x, 1.f - c.w1.y, 1.f - c.w1.z);
    c.x0 = wrap_coord(v.wrap, ix, nx); c.x1 = wrap_coord(v.wrap, ix + 1, nx);
    int y0 = wrap_coord(v.wrap, iy, ny), y1 = wrap_coord(v.wrap, iy + 1, ny), z0 = wrap_coord(v.wrap, iz, nz), z1 = wrap_coord(v.wrap, iz + 1, nz);
    c.r00 = (z0 * ny + y0) * nx; c.r10 = (z0 * ny + y1) * nx; c.r01 = (z1 * ny + y0) * nx; c.r11 = (z1 * ny + y1) * nx;
    return c;
}
DEV float grid_fetch1(const MTS_GLOBAL_AS float *__restrict__ D, const GridCell &c) {
    return trilerp(D[c.r00 + c.x0], D[c.r00 + c.x1], D[c.r10 + c.x0], D[c.r10 + c.x1],
                   D[c.r01 + c.x0], D[c.r01 + c.x1], D[c.r11 + c.x0], D[c.r11 + c.x1], c.w0, c.w1);
}

// Both grids of a medium from the interleaved copy (DMedium::pair_grid): one 16-byte gather per (z, y) row covers the two
// x-neighbours of sigma_t and albedo.  Clamp mode only: x1 is x0 + 1 except on the last column, where both are nx - 1.
// `nx` here is the stored row length: a one-column grid (the 1-D atmospheres: nz x 1 x 1) is stored two voxels wide.
typedef float mts_float4 __attribute__((ext_vector_type(4)));
// columns_equal (wave-uniform): a profile in z only -- the two rows of a z-level hold the same voxels, two gathers serve the lookup.
// The order of the gathers and of the one wait is PINNED in assembly: all loads of a lookup go out before the first wait on any of
// them.  Left to the compiler, `q10 = q00; if (!columns_equal) q10 = load` becomes a move ahead of the branch, which waits for q00 and
// q01 before the other two are issued -- two dependent round trips on every grid whose columns differ -- and every rewording of it
// in C++ (a select behind the join, the conditional pair first, a diamond) came back to that order in at least one of the repeat
// loops (tools/step_loop_stats.py --trips, tests/test_step_round_trips.py).  The compiler does not count these
// loads in vmcnt, which only makes its own waits stricter (loads return in order); the values may be read only behind grid_gather_wait,
// which every one of them passes through.
DEV mts_float4 grid_gather_issue(const MTS_GLOBAL_AS float *p) {
    mts_float4 q;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(q) : "v"(p) : "memory");
    return q;
}
DEV void grid_gather_wait(mts_float4 &a, mts_float4 &b, mts_float4 &c, mts_float4 &d) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
}
// The same wait for a caller that has work of its own between the issue and the wait (step_fast): k0 .. k3 are results of that work,
// which the wait takes as operands so that they are complete ahead of it -- without that the scheduler is free to sink the
// arithmetic that forms them behind the wait, where it stands on the voxels' chain again.
DEV void grid_gather_wait(mts_float4 &a, mts_float4 &b, mts_float4 &c, mts_float4 &d, float &k0, float &k1, float &k2, float &k3) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(k0), "+v"(k1), "+v"(k2), "+v"(k3));
}
// A lookup in two halves: the gathers go out (grid_pair_issue), the caller does what does not read a voxel, the one wait and the
// trilinear blend follow (grid_pair_blend; grid_gather_wait, between them, is the caller's, which may pin values of its own to it).
struct GridPairLoads { mts_float4 q00, q01, q10, q11; bool hi0, hi1; };
DEV GridPairLoads grid_pair_issue(const MTS_GLOBAL_AS float *__restrict__ P, const GridCell &c, int nx, bool columns_equal) {
    const int xb = min(c.x0, nx - 2);
    GridPairLoads g;
    g.hi0 = c.x0 != xb; g.hi1 = c.x1 != xb;                    // take the second voxel of the pair
    g.q00 = grid_gather_issue(P + 2 * (c.r00 + xb)); g.q01 = grid_gather_issue(P + 2 * (c.r01 + xb));
    g.q10 = mts_float4{0.f, 0.f, 0.f, 0.f}; g.q11 = mts_float4{0.f, 0.f, 0.f, 0.f};
    if (!columns_equal) { g.q10 = grid_gather_issue(P + 2 * (c.r10 + xb)); g.q11 = grid_gather_issue(P + 2 * (c.r11 + xb)); }
    return g;
}
DEV void grid_pair_blend(GridPairLoads &g, const GridCell &c, bool columns_equal, float &sigma_t, float &albedo) {      // behind the wait
    const bool hi0 = g.hi0, hi1 = g.hi1;
    mts_float4 q00 = g.q00, q01 = g.q01, q10 = g.q10, q11 = g.q11;
    if (columns_equal) { q10 = q00; q11 = q01; }
    sigma_t = trilerp(hi0 ? q00.z : q00.x, hi1 ? q00.z : q00.x, hi0 ? q10.z : q10.x, hi1 ? q10.z : q10.x,
                      hi0 ? q01.z : q01.x, hi1 ? q01.z : q01.x, hi0 ? q11.z : q11.x, hi1 ? q11.z : q11.x, c.w0, c.w1);
    albedo = trilerp(hi0 ? q00.w : q00.y, hi1 ? q00.w : q00.y, hi0 ? q10.w : q10.y, hi1 ? q10.w : q10.y,
                     hi0 ? q01.w : q01.y, hi1 ? q01.w : q01.y, hi0 ? q11.w : q11.y, hi1 ? q11.w : q11.y, c.w0, c.w1);
}
DEV void grid_fetch_pair(const MTS_GLOBAL_AS float *__restrict__ P, const GridCell &c, int nx, bool columns_equal, float &sigma_t, float &albedo) {
    GridPairLoads g = grid_pair_issue(P, c, nx, columns_equal);
    grid_gather_wait(g.q00, g.q01, g.q10, g.q11);
    grid_pair_blend(g, c, columns_equal, sigma_t, albedo);
}

template <bool COUNT>
DEV MedStep medium_step(const DScene &sc, const DMedium m, const DRay &ray, float sample, uint32_t channel, bool want_albedo, Counters &cnt,
                        const SpecCtx &cx = SpecCtx()) {
    MedStep mi;
#if (MTS_TRAITS & MT_MEDIA) && MTS_SPEC_N == 3      // promised: every medium heterogeneous, grey, on a pair grid, with spectral extinction
    const bool m_homogeneous = false, m_pair = true, m_grey = true, m_spectral = true;
#elif MTS_TRAITS & MT_MEDIA                         // spectral variant: heterogeneous, two gridvolume_spectral grids on one geometry and interval
    const bool m_homogeneous = false, m_pair = false, m_grey = false, m_spectral = true;
#elif MTS_TRAITS & MT_HOMOG                         // promised: every medium homogeneous
    const bool m_homogeneous = true, m_pair = false, m_grey = m.grey != 0, m_spectral = m.has_spectral_extinction != 0;
#else
    const bool m_homogeneous = m.is_homogeneous != 0, m_pair = m.pair_grid != nullptr, m_grey = m.grey != 0, m_spectral = m.has_spectral_extinction != 0;
#endif
    bool active = true; float mint = 0.f, maxt = pm_inf();
    if (!m_homogeneous) {
        active = bbox_ray_intersect(m.aabb, ray, mint, maxt);
        active = active && (pm_isfinite(mint) || pm_isfinite(maxt));
        if (!active) { mint = 0.f; maxt = pm_inf(); }
    }
    mint = pm_max(ray.mint, mint);
    maxt = pm_min(ray.maxt, maxt);
    Spec combined = m_homogeneous ? volume_eval(cload(sc.volumes + m.sigma_t), ray.o MTS_CXI(m.sigma_t)) * m.scale : spec_s(m.max_density);
    float mext = pick(combined, channel);
    const float inv_mext = m_homogeneous ? 0.f : m.inv_max_density;
    float sampled_t = mint + div_by_invariant(-pm_log(1.f - sample), mext, inv_mext);
    bool valid_mi = active && (sampled_t <= maxt);
    mi.t = valid_mi ? sampled_t : pm_inf();
    mi.p = ray_at(ray, sampled_t);
    mi.mint = mint;
    mi.sigma_t = mi.sigma_s = spec_s(0.f);
    if (m_homogeneous) {
        Spec st = volume_eval(cload(sc.volumes + m.sigma_t), mi.p MTS_CXI(m.sigma_t)) * m.scale;
        mi.sigma_t = st;
        if (want_albedo) mi.sigma_s = st * volume_eval(cload(sc.volumes + m.albedo), mi.p MTS_CXI(m.albedo));
    } else if (valid_mi) {
        if (COUNT) MTS_SEG(cnt, 1);
        if (m_pair) {                          // everything comes from the medium record and the interleaved grid
            const int sx = m.pair_nx < 2 ? 2 : m.pair_nx;
            GridCell c = grid_cell_clamp(m.pair_w2l, m.pair_affine & 1, m.pair_nx, m.pair_ny, m.pair_nz, sx, mi.p);
            float st_raw, al_raw;
            grid_fetch_pair(as_global(m.pair_grid), c, sx, (m.pair_affine & 2) != 0, st_raw, al_raw);
            float st = m.scale * st_raw;
            mi.sigma_t = spec_s(st);
            if (want_albedo) mi.sigma_s = spec_s(st * al_raw);
        } else {
            const DVolume vs = cload(sc.volumes + m.sigma_t), va = cload(sc.volumes + m.albedo);
            if (m.shared_grid && m_grey && vs.filter == MTS_FILTER_TRILINEAR) {
                // both grids share one cell / one set of weights; single channel: one value serves the three channels
                GridCell c = grid_cell(vs, mi.p);
                float st = m.scale * grid_fetch1(as_global(vs.data), c);
                mi.sigma_t = spec_s(st);
                if (want_albedo) mi.sigma_s = spec_s(st * grid_fetch1(as_global(va.data), c));    // the tracking walks never read sigma_s
#if MTS_SPEC_N != 3
            } else if ((MTS_TRAITS & MT_MEDIA) != 0 || m.shared_grid == 2) {
                // gridvolume_spectral for both, same geometry and spectral interval: one cell, one set of weights and spectral nodes
                GridRef g;
                for (int k = 0; k < 16; ++k) g.w2l[k] = vs.w2l[k];
                g.data = vs.data; g.nx = vs.nx; g.ny = vs.ny; g.nz = vs.nz;
                g.channels_affine_filter_wrap = (uint32_t) vs.channels | ((uint32_t) (vs.affine != 0) << 8) | ((uint32_t) vs.filter << 16) | ((uint32_t) vs.wrap << 24) |
                                                ((uint32_t) (vs.columns_equal != 0 && (!want_albedo || va.columns_equal != 0)) << 9);
                const DVolumeSp sp = cload(cx.volume_sp + m.sigma_t);
                if (want_albedo) {
                    const SpecPair r = volume_eval_grid_spectral_pair(g, va.data, mi.p, cx.wl, sp.lambda_min, sp.lambda_max);
                    const Spec st = m.scale * r.a;
                    mi.sigma_t = st; mi.sigma_s = st * r.b;
                } else
                    mi.sigma_t = m.scale * volume_eval_grid_spectral(g, mi.p, cx.wl, sp.lambda_min, sp.lambda_max);
#endif
            } else {
                Spec st = m.scale * volume_eval(vs, mi.p MTS_CXI(m.sigma_t));
                mi.sigma_t = st;
                if (want_albedo) mi.sigma_s = st * volume_eval(va, mi.p MTS_CXI(m.albedo));
            }
        }
        if (COUNT) cnt.n_lookup++;
        if (COUNT) MTS_SEG(cnt, 2);
    }
    mi.combined = combined;
    mi.inv_combined = inv_mext;
    mi.info = (m_homogeneous ? MI_HOMOGENEOUS : 0u) | (m_spectral ? MI_SPECTRAL : 0u) |
              (m.sample_emitters ? MI_SAMPLE_EMITTERS : 0u) | (m_grey ? MI_GREY : 0u) | ((uint32_t) m.phase << MI_PHASE_SHIFT);
    return mi;
}

// exp(-t * combined) per channel (medium.cpp:84); grey media evaluate it once
DEV Spec transmittance_exp_g(float t, Spec combined, bool grey) {
    if (grey) return spec_s(pm_exp(-t * combined.x));
    return transmittance_exp(t, combined);
}

#if MTS_SPEC_N == 3
// Film splat of one finished sample: librender/integrator.cpp:265-285 + librender/imageblock.cpp:79-172
// (The spectral build's splat_values_t in integrator_dev.h is this function's second half; sharing it changed the register allocation of
// the regrouping kernel -- 170 -> 197 SGPR spills -- so the rgb kernels keep their own copy.)
// `own` receives the samples that land in the lane's own pixel: either register accumulators (nested
// formulation) or the pixel's film entry itself, updated with float atomics in sample order.
template <bool OWN_ATOMIC>
DEV void splat_sample_t(const DScene &sc, const DBlock &blk, uint32_t lx, uint32_t ly, F2 position_sample, F3 L, bool valid,
                        MTS_GLOBAL_AS float *film, float *own) {
    const DSensor &se = sc.sensor;
    float v[5];                                                 // srgb_to_xyz, core/spectrum.h:221-227
    v[0] = pm_fma(0.180423f, L.z, pm_fma(0.357580f, L.y, 0.412453f * L.x));
    v[1] = pm_fma(0.072169f, L.z, pm_fma(0.715160f, L.y, 0.212671f * L.x));
    v[2] = pm_fma(0.950227f, L.z, pm_fma(0.119193f, L.y, 0.019334f * L.x));
    if (sc.integrator.monochrome)                               // integrator.cpp:270-271: xyz = spec_u.x()
        v[0] = v[1] = v[2] = L.x;
    v[3] = valid ? 1.f : 0.f;
    v[4] = 1.f;
    bool ok = true;                                             // imageblock.cpp:85-109: invalid samples are dropped
    for (int k = 0; k < 5; ++k) ok = ok && v[k] >= -1e-5f && pm_isfinite(v[k]);
    if (!ok) return;
    const DRFilter &rf = se.rfilter;
    const int border = rf.border_size;
    const int sx = blk.sx + 2 * border, sy = blk.sy + 2 * border;
    float posx = position_sample.x - ((float) (blk.ox - border) + .5f), posy = position_sample.y - ((float) (blk.oy - border) + .5f);
    if (rf.radius > 0.5f + MTS_RAY_EPSILON) {
        int lox = max((int) pm_ceil(posx - rf.radius), 0), loy = max((int) pm_ceil(posy - rf.radius), 0);
        int hix = min((int) pm_floor(posx + rf.radius), sx - 1), hiy = min((int) pm_floor(posy + rf.radius), sy - 1);
        uint32_t n = (uint32_t) pm_ceil((rf.radius - 2.f * MTS_RAY_EPSILON) * 2.f);
        float basex = (float) lox - posx, basey = (float) loy - posy;
        for (uint32_t yr = 0; yr < n; ++yr) {
            int y = loy + (int) yr;
            if (y > hiy) break;
            float wy = as_global(rf.values)[min((int) pm_abs((basey + (float) yr) * rf.scale_factor), 31)];     // eval_discretized, core/rfilter.h:62-65
            int fy = blk.oy - border + y - se.crop_y;
            for (uint32_t xr = 0; xr < n; ++xr) {
                int x = lox + (int) xr;
                if (x > hix) break;
                float wx = as_global(rf.values)[min((int) pm_abs((basex + (float) xr) * rf.scale_factor), 31)];
                float weight = wy * wx;
                int fx = blk.ox - border + x - se.crop_x;
                if (fx >= 0 && fy >= 0 && fx < se.crop_w && fy < se.crop_h) {                         // film clipping, imageblock.cpp:49-77
                    float *dst = (float *) (film + 5 * ((size_t) fy * se.crop_w + fx));
                    for (int k = 0; k < 5; ++k) atomicAdd(dst + k, v[k] * weight);
                }
            }
        }
    } else {
        int lox = (int) pm_ceil(posx - .5f), loy = (int) pm_ceil(posy - .5f);
        if (lox == (int) lx && loy == (int) ly) {
            if (OWN_ATOMIC) { for (int k = 0; k < 5; ++k) atomicAdd(own + k, v[k]); }
            else { for (int k = 0; k < 5; ++k) own[k] += v[k]; }
        } else if (lox >= 0 && loy >= 0 && lox < sx && loy < sy) {
            float *dst = (float *) (film + 5 * ((size_t) (blk.oy + loy - se.crop_y) * se.crop_w + (blk.ox + lox - se.crop_x)));
            for (int k = 0; k < 5; ++k) atomicAdd(dst + k, v[k]);
        }
    }
}

#if !defined(MTS_LEAN)
#define MTS_MOMENT_CHANNELS 11
// The `moment` integrator's film splat (integrators/moment.cpp:60-90 around the nested integrator's sample(), then
// librender/integrator.cpp:265-285 + librender/imageblock.cpp:79-172): eleven values per sample -- X, Y, Z, A, W of ray_weight * L as
// splat_sample_t forms them, then xyz of L itself (BEFORE the sensor's ray weight; mono: L.x three times) and the squares of those
// three, each rounded once.  A film with AOV channels is created with warn_negative = false (integrator.cpp:114-116), so a sample is
// dropped iff one of the eleven is not finite; the -1e-5 test of the plain film does not apply.  Every channel takes the same filter
// weights, eleven floats per film pixel.  A sibling of splat_sample_t on purpose: the plain kernels keep their five-channel copy.
// OWN_ALL: `own` holds eleven register accumulators (per-lane kernels); otherwise five (the ring machines' cold record), and the six
// AOV values of a sample that lands in the lane's own pixel join its film entry by atomics -- one path writes them in sample order, so
// the sum is the block's (as splat_values_bins, integrator_dev.h).
template <bool OWN_ALL>
DEV void splat_moment_t(const DScene &sc, const DBlock &blk, uint32_t lx, uint32_t ly, F2 position_sample, F3 L, float ray_weight, bool valid,
                        MTS_GLOBAL_AS float *film, float *own) {
    const DSensor &se = sc.sensor;
    constexpr int C = MTS_MOMENT_CHANNELS;
    const F3 Lw = f3s(ray_weight) * L;
    float v[C];                                                 // srgb_to_xyz, core/spectrum.h:221-227
    v[0] = pm_fma(0.180423f, Lw.z, pm_fma(0.357580f, Lw.y, 0.412453f * Lw.x));
    v[1] = pm_fma(0.072169f, Lw.z, pm_fma(0.715160f, Lw.y, 0.212671f * Lw.x));
    v[2] = pm_fma(0.950227f, Lw.z, pm_fma(0.119193f, Lw.y, 0.019334f * Lw.x));
    v[5] = pm_fma(0.180423f, L.z, pm_fma(0.357580f, L.y, 0.412453f * L.x));      // moment.cpp:74-79
    v[6] = pm_fma(0.072169f, L.z, pm_fma(0.715160f, L.y, 0.212671f * L.x));
    v[7] = pm_fma(0.950227f, L.z, pm_fma(0.119193f, L.y, 0.019334f * L.x));
    if (sc.integrator.monochrome) { v[0] = v[1] = v[2] = Lw.x; v[5] = v[6] = v[7] = L.x; }
    v[3] = valid ? 1.f : 0.f;
    v[4] = 1.f;
    for (int k = 0; k < 3; ++k) v[8 + k] = v[5 + k] * v[5 + k];
    bool ok = true;
    for (int k = 0; k < C; ++k) ok = ok && pm_isfinite(v[k]);
    if (!ok) return;
    const DRFilter &rf = se.rfilter;
    const int border = rf.border_size;
    const int sx = blk.sx + 2 * border, sy = blk.sy + 2 * border;
    float posx = position_sample.x - ((float) (blk.ox - border) + .5f), posy = position_sample.y - ((float) (blk.oy - border) + .5f);
    if (rf.radius > 0.5f + MTS_RAY_EPSILON) {
        int lox = max((int) pm_ceil(posx - rf.radius), 0), loy = max((int) pm_ceil(posy - rf.radius), 0);
        int hix = min((int) pm_floor(posx + rf.radius), sx - 1), hiy = min((int) pm_floor(posy + rf.radius), sy - 1);
        uint32_t n = (uint32_t) pm_ceil((rf.radius - 2.f * MTS_RAY_EPSILON) * 2.f);
        float basex = (float) lox - posx, basey = (float) loy - posy;
        for (uint32_t yr = 0; yr < n; ++yr) {
            int y = loy + (int) yr;
            if (y > hiy) break;
            float wy = as_global(rf.values)[min((int) pm_abs((basey + (float) yr) * rf.scale_factor), 31)];     // eval_discretized, core/rfilter.h:62-65
            int fy = blk.oy - border + y - se.crop_y;
            for (uint32_t xr = 0; xr < n; ++xr) {
                int x = lox + (int) xr;
                if (x > hix) break;
                float wx = as_global(rf.values)[min((int) pm_abs((basex + (float) xr) * rf.scale_factor), 31)];
                float weight = wy * wx;
                int fx = blk.ox - border + x - se.crop_x;
                if (fx >= 0 && fy >= 0 && fx < se.crop_w && fy < se.crop_h) {                         // film clipping, imageblock.cpp:49-77
                    float *dst = (float *) (film + C * ((size_t) fy * se.crop_w + fx));
                    for (int k = 0; k < C; ++k) atomicAdd(dst + k, v[k] * weight);
                }
            }
        }
    } else {
        int lox = (int) pm_ceil(posx - .5f), loy = (int) pm_ceil(posy - .5f);
        if (!(lox >= 0 && loy >= 0 && lox < sx && loy < sy)) return;
        float *dst = (float *) (film + C * ((size_t) (blk.oy + loy - se.crop_y) * se.crop_w + (blk.ox + lox - se.crop_x)));
        if (lox == (int) lx && loy == (int) ly) {
            for (int k = 0; k < (OWN_ALL ? C : 5); ++k) own[k] += v[k];
            if (!OWN_ALL) for (int k = 5; k < C; ++k) atomicAdd(dst + k, v[k]);
        } else {
            for (int k = 0; k < C; ++k) atomicAdd(dst + k, v[k]);
        }
    }
}
#endif // !MTS_LEAN

#endif // MTS_SPEC_N == 3 (the spectral build splats through splat_values_t, integrator_dev.h)

// block -> film (hdrfilm.cpp:207-211): the film entry of pixel (lx, ly) of a block, which its accumulators X, Y, Z, A, W join by atomics
DEV float *film_entry(const DScene &sc, const DBlock &blk, uint32_t lx, uint32_t ly, MTS_GLOBAL_AS float *film) {
    return (float *) (film + MTS_FILM_STRIDE(sc) * ((size_t) (blk.oy + (int) ly - sc.sensor.crop_y) * sc.sensor.crop_w + (blk.ox + (int) lx - sc.sensor.crop_x)));
}

#if MTS_SPEC_N == 3 && !defined(MTS_LEAN)
// the same entry of a `moment` film (eleven floats per pixel, splat_moment_t)
DEV float *film_entry_moment(const DScene &sc, const DBlock &blk, uint32_t lx, uint32_t ly, MTS_GLOBAL_AS float *film) {
    return (float *) (film + MTS_MOMENT_CHANNELS * ((size_t) (blk.oy + (int) ly - sc.sensor.crop_y) * sc.sensor.crop_w + (blk.ox + (int) lx - sc.sensor.crop_x)));
}
#endif
// which film a ring machine writes: MOMENT machines (rgb / mono general unit only) the eleven-channel one
template <bool MOMENT>
DEV float *film_entry_of(const DScene &sc, const DBlock &blk, uint32_t lx, uint32_t ly, MTS_GLOBAL_AS float *film) {
#if MTS_SPEC_N == 3 && !defined(MTS_LEAN)
    if constexpr (MOMENT) return film_entry_moment(sc, blk, lx, ly, film);
    else
#endif
    return film_entry(sc, blk, lx, ly, film);
}

// ---------------------------------------------------------------------------------------------------------
// Per-path state.  "Hot" fields are touched by every tracking step; "cold" fields (ColdStore) only once per
// sample or per NEE / direct-light walk.
struct PathState {
    Pcg32 rng;
    DRay ray;                       // the ray being tracked now (main path, or the NEE / direct-light walk)
    Hit si;                         // cached closest hit of `ray`
    int medium;                     // medium containing ray.o
    Spec thr, res; float eta; uint32_t depth, channel;       // main path (volpath.cpp:54-67)
    Spec trans; float wa, wb;       // walk: transmittance; NEE: wa = total_dist, wb = ds.dist; direct: wb = bs.pdf
#if MTS_SPEC_N != 3
    Spec wl;                        // the sample's wavelengths (integrator.cpp:252)
#endif
    uint32_t st, mode, flags;
};
// cold field offsets (floats)
enum { C_POS = 0,            // 2: film position of the current sample
       C_RAYW = 2,           // 1: sensor ray weight
       C_SO = 3, C_SD = 6,   // 3 + 3: parked main-path origin / direction
       C_SHIT = 9,           // 8: parked main-path hit (t, p, uv, shape, prim)
       C_SMED = 17,          // 1: parked medium id
       C_CW = 18,                           // 3 (spectral: 4): pending NEE weight
       C_EMIT = C_CW + MTS_SPEC_DW,         // 3 (4): emitter value of the NEE sample
       C_ACC = C_EMIT + MTS_SPEC_DW,        // 5: this path's film accumulators X, Y, Z, A, W (the reference's per-block ImageBlock entry)
       C_SAMPLE = C_ACC + 5,                // 1: index of the sample in flight (bits of a uint32)
       C_COUNT = C_SAMPLE + 1 };            // 30 (32)
static_assert(C_COUNT <= 32, "the cold record is one 128-byte line");
// Struct-of-arrays store addressed as base[k * stride]: LDS (stride 256, one workgroup) or HBM (stride = paths in flight)
// or as one 128-byte record per path (AOS: the workgroup driver, whose lanes hold arbitrary paths -- a record is written by one
// lane as whole cache lines instead of 30 scattered dwords)
#define MTS_COLD_RECORD 32      // floats per path record (C_COUNT rounded up to a 128-byte line)
template <class Ptr /* float* into LDS, or MTS_GLOBAL_AS float* into HBM */, bool AOS = false>
struct ColdStoreT {
    Ptr base; uint32_t stride;
    DEV auto &f(int k) const { return AOS ? base[k] : base[(size_t) k * stride]; }
    DEV void put3(int k, F3 v) const { f(k) = v.x; f(k + 1) = v.y; f(k + 2) = v.z; }
    DEV F3 get3(int k) const { return f3(f(k), f(k + 1), f(k + 2)); }
#if MTS_SPEC_N == 3
    DEV void put_spec(int k, Spec v) const { put3(k, v); }
    DEV Spec get_spec(int k) const { return get3(k); }
#else
    DEV void put_spec(int k, Spec v) const { f(k) = v.x; f(k + 1) = v.y; f(k + 2) = v.z; f(k + 3) = v.w; }
    DEV Spec get_spec(int k) const { return spec4(f(k), f(k + 1), f(k + 2), f(k + 3)); }
#endif
    DEV void put_hit(const Hit &h) const {
        f(C_SHIT) = h.t; put3(C_SHIT + 1, h.p); f(C_SHIT + 4) = h.uv.x; f(C_SHIT + 5) = h.uv.y;
        f(C_SHIT + 6) = __int_as_float(h.shape); f(C_SHIT + 7) = __int_as_float(h.prim);
    }
    DEV Hit get_hit() const {
        Hit h; h.t = f(C_SHIT); h.p = get3(C_SHIT + 1); h.uv.x = f(C_SHIT + 4); h.uv.y = f(C_SHIT + 5);
        h.shape = __float_as_int(f(C_SHIT + 6)); h.prim = __float_as_int(f(C_SHIT + 7)); return h;
    }
};
// What a path needs from its surroundings
typedef ColdStoreT<float *> ColdStore;                       // generic pointer (the per-lane driver parks cold state in LDS)
typedef ColdStoreT<MTS_GLOBAL_AS float *, true> ColdStoreHbm;
// (workgroup driver: cold state in HBM, addressed with GLOBAL instructions)
template <class Cold>
struct PathEnvT {
    DBlock blk; uint32_t lx, ly, sample_count; MTS_GLOBAL_AS float *film; Cold cold;
    MTS_GLOBAL_AS float *park;     // volpathmis: a second 128-byte record per path -- p_over_f / p_over_f_nee while an emitter-sampling walk runs (volpathmis_flat.h)
    uint32_t index;                // the pixel's Morton index inside its spiral block (seeds its stream, integrator.cpp:198)
};
// Scheduling classes: the block a path is waiting for
enum { B_INT = 0, B_MED /* free-flight step of the main path */, B_SCATTER, B_WSURF, B_SURF, B_PHASE, B_NEW,
       B_MEDW /* free-flight step of an NEE / direct-light walk */,
       B_CROSS /* the main path crosses a null-BSDF boundary that emits nothing: B_SURF's work for such a hit and no more (wg_block) */,
       B_DONE, B_COUNT };
// MTS_CROSS_CLASS (unit_config.h): the `volpath` ring machines of the unit, scalar streams, sort their crossings into B_CROSS (wg_block:
// cross_class).  Everywhere else the class exists and stays empty: B_SURF is the general block and serves every hit.
// MTS_HOT_DRCP (unit_config.h): the hot state holds 1 / d (HotFront).  0: the unit's ring kernels form it from d, and their init loop
// loads the kernel arguments inside its body (ring_driver.h: M::OPAQUE_INIT = MTS_OPAQUE_INIT) -- two changes of the same kind
// (registers and LDS against instructions) that were measured together, unit by unit.  The ninth ring takes its LDS from the 12 KiB:
static_assert(!MTS_CROSS_CLASS || (!MTS_HOT_DRCP && MTS_SPEC_N == 3), "B_CROSS: rgb / mono, and the ring's 2 KiB come out of H_DRCP's 12");

// What a MEDIUM block reads of MedStep::info.  constexpr accessors: a lean unit's promises (MTS_TRAITS) are constants the front end folds,
// as in the #if ladders this replaces (three plain bools: 1086 differing assembly lines in lean unit a).
struct MediumKind {
    uint32_t info;
    constexpr bool spectral() const { return (MTS_TRAITS & MT_MEDIA) ? true : (info & MI_SPECTRAL) != 0; }
    constexpr bool homogeneous() const { return (MTS_TRAITS & MT_MEDIA) ? false : (MTS_TRAITS & MT_HOMOG) ? true : (info & MI_HOMOGENEOUS) != 0; }
    constexpr bool grey() const { return (MTS_TRAITS & MT_MEDIA) ? MTS_SPEC_N == 3 : (info & MI_GREY) != 0; }
};
// What the two ring machines share (VolpathMachine below, VolpathMisMachine of volpathmis_flat.h), as a CRTP base: M supplies
// begin_sample, P is its path state.  DIRB: the machine has direct-light walks, whose start (S_DIRB) waits for an intersection too.
template <class M, class P, bool DIRB>
struct RingMachine {
    const DScene &sc;
    Counters &cnt;
    DEV RingMachine(const DScene &sc_, Counters &cnt_) : sc(sc_), cnt(cnt_) {}
    // wavelength context of a path (empty in the rgb build)
#if MTS_SPEC_N == 3
    DEV SpecCtx ctx(const P &) const { return SpecCtx(); }
#else
    DEV SpecCtx ctx(const P &p) const { SpecCtx cx = make_ctx(sc); cx.wl = p.wl; return cx; }
#endif

    // A freshly spawned ray that cannot reach the scene's bounding box is resolved on the spot (the first
    // test of ShapeKDTree::ray_intersect_scalar, kdtree.h:2095-2098); everything else queues for INTERSECT.
    DEV void queue_intersection(P &p) const {
        float bmint, bmaxt;
        bbox_ray_intersect(sc.bbox, p.ray, bmint, bmaxt);
        p.si.t = pm_inf();                                     // si.shape etc. are only read behind hit_valid()
        if (pm_max(p.ray.mint, bmint) <= bmaxt) p.flags |= FL_NEEDS_INT; else p.flags &= ~FL_NEEDS_INT;
    }
    // the end of an emitter-sampling walk, second half: the parked main path comes back from the cold record
    template <class E> DEV void resume_main(P &p, const E &e) const {
        p.mode = M_MAIN; p.medium = __float_as_int(e.cold.f(C_SMED));
        F3 d = e.cold.get3(C_SD);
        p.ray.d = d; p.ray.d_rcp = vrcp(d);
        if (p.flags & FL_FROM_MEDIUM) { p.ray.o = e.cold.get3(C_SO); p.st = S_PHASE; }
        else { p.si = e.cold.get_hit(); p.st = S_BSDF; }
    }
    DEV static bool wants_int(const P &p) { return (p.st == S_MED || p.st == S_SURF || (DIRB && p.st == S_DIRB)) && (p.flags & FL_NEEDS_INT); }
    // block this path waits for (valid once top() has run)
    DEV static int classify(const P &p) {
        if (p.st == S_DONE) return B_DONE;
        if (wants_int(p)) return B_INT;
        if (p.st == S_MED) return p.mode == M_MAIN ? B_MED : B_MEDW;
        if (p.st == S_SCATTER) return B_SCATTER;
        if (p.st == S_SURF) return p.mode == M_MAIN ? B_SURF : B_WSURF;
        if (p.st == S_BSDF) return B_SURF;
        if (p.st == S_PHASE) return B_PHASE;
        return B_NEW;
    }
    // ================================================================= INTERSECT, the core (volpath.cpp:109,182,241,298,339,395,425)
    DEV bool intersect(P &p) const {
        if (!wants_int(p)) return false;
        p.si = ray_intersect<M::GEOM_TABLE, M::INST>(sc, p.ray);      // ring kernels of the lean units a, h: hit points from the LDS table
        p.flags &= ~FL_NEEDS_INT;
        return true;
    }
    // ================================================================= NEW: finish a sample, start the next (integrator.cpp:265-288)
    // (The per-lane kernels keep their own result -> XYZ -> splat lines, kernels.hip.  One function for them and this block, taking a record:
    // v_spectral_lean_p::render_kernel<false, true, 0> 560 -> 576 B of scratch, <true, true, 0> 245 -> 253 SGPR spills and 560 -> 576 B.
    // One for the per-lane kernels alone, taking scalars: <false, true, 0> 255 -> 257 SGPR spills, 560 -> 576 B.)
    template <class E> DEV void blk_new(P &p, const E &e) const {
        if (p.st != S_NEW) return;
        F2 position_sample; position_sample.x = e.cold.f(C_POS); position_sample.y = e.cold.f(C_POS + 1);
        float acc[5];                                          // summed in sample order like the block entry (imageblock.cpp:163-168)
        for (int k = 0; k < 5; ++k) acc[k] = e.cold.f(C_ACC + k);
#if MTS_SPEC_N == 3
#if !defined(MTS_LEAN)
        // M::MOMENT: the `moment` wrapper's tail -- the same five accumulators, the six AOV values straight to the film entry
        if constexpr (M::MOMENT) splat_moment_t<false>(sc, e.blk, e.lx, e.ly, position_sample, p.res, e.cold.f(C_RAYW), (p.flags & FL_VALID_RAY) != 0, e.film, acc);
        else
#endif
        splat_sample_t<false>(sc, e.blk, e.lx, e.ly, position_sample, f3s(e.cold.f(C_RAYW)) * p.res, (p.flags & FL_VALID_RAY) != 0, e.film, acc);
#else
        {
            float wav_weight; (void) sample_wavelengths(0.f, wav_weight);
            const Spec ww = sc.srf >= 0 ? srf_weights_of(sc, p.wl) : spec_s(wav_weight);
            const Spec L = (ww * e.cold.f(C_RAYW)) * p.res;             // ray_weight = wav_weight (x the sensor's grey weight), integrator.cpp:265
            float xyz[3];
            spectrum_to_xyz(sc.cie, L, p.wl, xyz);                      // integrator.cpp:266-269
            const float v[5] = { xyz[0], xyz[1], xyz[2], (p.flags & FL_VALID_RAY) != 0 ? 1.f : 0.f, 1.f };
            if (sc.bin_count == 0) splat_values_t<false>(sc, e.blk, e.lx, e.ly, position_sample, v, e.film, acc);
            else splat_values_bins(sc, e.blk, e.lx, e.ly, position_sample, v, p.res, p.wl, e.film, acc);
        }
#endif
        const uint32_t sample_idx = __float_as_uint(e.cold.f(C_SAMPLE)) + 1u;
        if (sample_idx == e.sample_count) {                    // block -> film (hdrfilm.cpp:207-211)
            float *own = film_entry_of<M::MOMENT>(sc, e.blk, e.lx, e.ly, e.film);
            for (int k = 0; k < 5; ++k) atomicAdd(own + k, acc[k]);
            p.st = S_DONE;
        } else {
            for (int k = 0; k < 5; ++k) e.cold.f(C_ACC + k) = acc[k];
            e.cold.f(C_SAMPLE) = __uint_as_float(sample_idx);
            static_cast<const M &>(*this).begin_sample(p, e);
        }
    }
};

// GEOM_: the machine runs under the ring driver of a unit with the geometry table in LDS (integrator_dev.h: MTS_GEOM_LDS)
// TEX_: the BSDF record of a hit goes through its textures (integrator_dev.h: bsdf_apply_textures; general rgb / mono unit only)
template <bool COUNT, bool MOMENT_ = false, bool GEOM_ = false, int TEX_ = TEX_NONE>
struct VolpathMachine : RingMachine<VolpathMachine<COUNT, MOMENT_, GEOM_, TEX_>, PathState, true> {
    typedef RingMachine<VolpathMachine<COUNT, MOMENT_, GEOM_, TEX_>, PathState, true> Base;
    static constexpr bool MOMENT = MOMENT_;                    // RingMachine::blk_new: the `moment` wrapper's eleven-channel tail
    static constexpr int TEX = TEX_;
    static constexpr bool INST = TEX_ == TEX_INST;      // an instanced scene: two-level traversal, the instance resolved per lane (integrator_dev.h)
    static constexpr bool GEOM_TABLE = GEOM_;
    using Base::sc; using Base::cnt; using Base::ctx; using Base::queue_intersection; using Base::wants_int;
    DEV VolpathMachine(const DScene &sc_, Counters &cnt_) : Base(sc_, cnt_) {}
    // The head of a sample (the draws up to the camera ray) stays written out here, in VolpathMisMachine::begin_sample and in render_sample
    // and path_pixel_flat (kernels.hip).  As one function returning a record, called from the four, 24 of the 72 kernels need more:
    // scratch of the spectral ring kernels 28 -> 60 B (v_spectral_lean::render_kernel_wga<false, 256, 256, 3>) and 496 -> 528 B (v_spectral::),
    // spilled VGPRs of the flat `path` kernels 98 -> 138 (v_rgb::render_kernel<false, true, 0>) and 40 -> 105 (v_spectral::).  Filling
    // references, or as a member of RingMachine holding these very lines, it still changed the ring kernels of lean unit a.
    template <class E> DEV void begin_sample(PathState &p, const E &e) const {      // integrator.cpp:242-264, volpath.cpp:48-71
        const DSensor &se = sc.sensor;
        const float px = (float) (e.lx + (uint32_t) e.blk.ox), py = (float) (e.ly + (uint32_t) e.blk.oy);
        if (se.wavefront) seed_wavefront_sample(p.rng, se, e.blk, e.lx, e.ly, __float_as_uint(e.cold.f(C_SAMPLE)));   // gpu_* streams: one per (pixel, sample)
        F2 u = p.rng.next_2d();
        F2 position_sample; position_sample.x = px + u.x; position_sample.y = py + u.y;
        F2 aperture_sample; aperture_sample.x = .5f; aperture_sample.y = .5f;
        if (se.needs_aperture_sample) aperture_sample = p.rng.next_2d();
        if (se.shutter_open_time > 0.f) (void) p.rng.next_1d();   // time sample (integrator.cpp:248-250)
#if MTS_SPEC_N == 3
        (void) p.rng.next_1d();                                // wavelength sample, unused in rgb
#else
        {                                                      // integrator.cpp:252 -> perspective.cpp:169-182, distant.cpp:311-313; blk_new recomputes the weights
            const float wavelength_sample = p.rng.next_1d();
            float wav_weight; Spec srf_weight;
            p.wl = sc.srf >= 0 ? sample_wavelengths_srf(sc, wavelength_sample, srf_weight) : sample_wavelengths(wavelength_sample, wav_weight);
        }
#endif
        F2 adjusted;
        adjusted.x = (position_sample.x - (float) se.crop_x) / (float) se.crop_w;
        adjusted.y = (position_sample.y - (float) se.crop_y) / (float) se.crop_h;
        F3 rw;
        p.ray = sensor_sample_ray(sc, adjusted, aperture_sample, rw);
        e.cold.f(C_POS) = position_sample.x; e.cold.f(C_POS + 1) = position_sample.y; e.cold.f(C_RAYW) = rw.x;   // grey weight
        p.medium = se.medium;
        p.thr = spec_s(1.f); p.res = spec_s(0.f); p.eta = 1.f; p.depth = 0;
#if MTS_SPEC_N == 3
        p.channel = sc.integrator.monochrome ? 0u : (uint32_t) pm_min(p.rng.next_1d() * 3.f, 2.f);     // volpath.cpp:64-67: rgb variants only
#else
        p.channel = 0u;                                        // volpath.cpp:63-67: no draw outside the rgb variants
#endif
        p.si.p = f3s(0.f); p.si.uv.x = p.si.uv.y = 0.f; p.si.prim = 0;
        const bool hide_emitters = sc.integrator.hide_emitters != 0;
        p.flags = FL_ALIVE | ((!hide_emitters && sc.environment >= 0) ? FL_VALID_RAY : 0u) | (!hide_emitters ? FL_SPEC_CHAIN : 0u);
        p.trans = spec_s(1.f); p.wa = p.wb = 0.f;
        queue_intersection(p);
        p.mode = M_MAIN; p.st = S_TOP;
    }
    // NEE walk finished (volpath.cpp:366 + :165-166 / :211): add the contribution, resume the main path
    template <class E> DEV void end_nee(PathState &p, const E &e) const {
        Spec emitted = p.trans * e.cold.get_spec(C_EMIT);
        p.res = p.res + e.cold.get_spec(C_CW) * emitted;
        this->resume_main(p, e);
    }
    // direct-light walk finished (volpath.cpp:464 + :246-252): MIS-weighted emitter hit, resume the main path
    template <class E> DEV void end_direct(PathState &p, const E &e, Spec emitter_val, float emitter_pdf) const {
        Spec emitted = p.trans * emitter_val;
        if (emitter_pdf != 0.f) p.res = p.res + mis_weight(p.wb, emitter_pdf) * p.thr * emitted;
        p.ray = spawn_ray(e.cold.get3(C_SO), e.cold.get3(C_SD));
        p.si = e.cold.get_hit(); p.medium = __float_as_int(e.cold.f(C_SMED));
        p.flags = (p.flags & ~FL_NEEDS_INT) | FL_ALIVE;
        p.mode = M_MAIN; p.st = S_TOP;
    }

    // Loop heads of the three reference loops (cheap): volpath.cpp:79-87, :283-287, :385-388
    template <bool DEFER = false, class E> DEV void top(PathState &p, const E &e) const {
        if (p.st != S_TOP) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth, rr_depth = (uint32_t) sc.integrator.rr_depth;
        if (p.mode == M_MAIN) {
            bool active = (p.flags & FL_ALIVE) && any_nonzero(p.thr);
            float q = pm_min(hmax(p.thr) * (p.eta * p.eta), .95f);
            bool perform_rr = p.depth > rr_depth;
            active = active && (p.rng.next_1d() < q || !perform_rr);
            if (perform_rr) p.thr = p.thr * pm_rcp(q);
            if (!active || p.depth >= max_depth) p.st = S_NEW;
            else { if (COUNT) cnt.n_iter++; p.st = p.medium >= 0 ? S_MED : S_SURF; }
        } else if (p.mode == M_NEE) {
            float remaining_dist = p.wb * (1.f - MTS_SHADOW_EPSILON) - p.wa;
            p.ray.maxt = remaining_dist;
            if (!(remaining_dist > 0.f)) { if (DEFER) p.st = S_ENDNEE; else end_nee(p, e); }
            else { if (COUNT) cnt.n_nee_step++; p.st = p.medium >= 0 ? S_MED : S_SURF; }
        } else {
            if (COUNT) cnt.n_nee_step++;
            p.st = p.medium >= 0 ? S_MED : S_SURF;
        }
    }
    // ================================================================= INTERSECT (volpath.cpp:109,182,241,298,339,395,425)
    template <class E> DEV void blk_int(PathState &p, const E &e) const {
        if (this->intersect(p)) start_direct(p, e);
    }
    template <class E> DEV void start_direct(PathState &p, const E &e) const {      // volpath.cpp:239-245: the direct-light walk runs on a copy
        if (p.st != S_DIRB || (p.flags & FL_NEEDS_INT)) return;
        e.cold.put3(C_SO, p.ray.o); e.cold.put3(C_SD, p.ray.d); e.cold.put_hit(p.si);
        p.trans = spec_s(1.f);
        p.mode = M_DIR; p.st = S_TOP;
    }
    // ================================================================= MEDIUM: one free-flight step of any of the three loops
    // MODEK: 0 = lanes of the main path only, 1 = lanes of a walk only (workgroup driver: one class each), -1 = any
    template <bool DEFER = false, int MODEK = -1, class E> DEV void blk_med(PathState &p, const E &e) const {
        if (p.st != S_MED || (p.flags & FL_NEEDS_INT)) return;
        if (MODEK == 0 && p.mode != M_MAIN) return;
        if (MODEK == 1 && p.mode == M_MAIN) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth;
        const float u = p.rng.next_1d();                       // volpath.cpp:105 / :294 / :391
        MedStep mi;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(p.medium, mu)
            mi = medium_step<COUNT>(sc, cload(sc.media + mu), p.ray, u, p.channel, MODEK == 0 ? true : (MODEK == 1 ? false : p.mode == M_MAIN), cnt MTS_CX);
        WATERFALL_END
        if (p.si.t < mi.t) mi.t = pm_inf();                    // volpath.cpp:112 / :300 / :397
        const MediumKind mk = { mi.info };
        const bool spectral = mk.spectral(), homogeneous = mk.homogeneous(), grey = mk.grey();
        const Spec sigma_n = homogeneous ? spec_s(0.f) : mi.combined - mi.sigma_t;
        const uint32_t channel = p.channel;
        const bool is_main = MODEK == 0 ? true : (MODEK == 1 ? false : p.mode == M_MAIN), is_nee = MODEK == 0 ? false : p.mode == M_NEE;
        // transmittance / free-flight pdf of this step, one formula for the three loops:
        // medium.cpp:77-89 (volpath.cpp:113-117, :401-405) and the NEE variant bounded by remaining_dist (:305-311)
        const float remaining_dist = is_nee ? p.ray.maxt : pm_inf();
        Spec weight = is_main ? p.thr : p.trans;
        if (spectral) {
            float t = pm_min(mi.t, p.si.t);
            if (is_nee) t = pm_min(remaining_dist, t);
            t = t - mi.mint;
            const bool surface_first = p.si.t < mi.t || mi.t > remaining_dist;
            if (grey || !homogeneous) {                        // the combined extinction is one value for every channel (a grey medium, or a
                float tr = pm_exp(-t * mi.combined.x);          // heterogeneous one: its majorant is a scalar, heterogeneous.cpp:29): one exp, one division
                float tr_pdf = surface_first ? tr : tr * mi.combined.x;
                weight = weight * (tr_pdf > 0.f ? tr * pm_rcp(tr_pdf) : 0.f);     // spectrum / scalar = spectrum * (1 / scalar), dmath.h
            } else {
                Spec tr = transmittance_exp(t, mi.combined);
                Spec free_flight_pdf = surface_first ? tr : tr * mi.combined;
                float tr_pdf = pick(free_flight_pdf, channel);
                weight = weight * (tr_pdf > 0.f ? tr / tr_pdf : spec_s(0.f));
            }
        }
        float u2 = 0.f;
        if (is_main) u2 = p.rng.next_1d();                     // volpath.cpp:123 (drawn even when the medium was left)
        if (is_nee) {                                          // volpath.cpp:313-315
            if (mi.t > remaining_dist && mi.t != pm_inf()) p.wa = p.wb;
            if (mi.t > remaining_dist) mi.t = pm_inf();
        }
        const bool valid = mi.t != pm_inf();
        if (!valid) {                                          // escaped_medium: surface part of this iteration
            if (is_main) p.thr = weight; else p.trans = weight;
            p.st = S_SURF;
            return;
        }
        const bool real_scatter = is_main && !(u2 >= (grey ? div_by_invariant(mi.sigma_t.x, mi.combined.x, mi.inv_combined)
                                                                : div_by_invariant(pick(mi.sigma_t, channel), pick(mi.combined, channel), mi.inv_combined)));
        if (!real_scatter) {
            // null collision of the main path (volpath.cpp:128-131,140-144) or a step of a walk (:322-333, :411-420)
            if (grey) {
                if (is_main) { if (spectral) weight = weight * ((sigma_n.x * mi.combined.x) * pm_rcp(sigma_n.x)); }
                else { if (spectral) weight = weight * sigma_n.x; else weight = weight * div_by_invariant(sigma_n.x, mi.combined.x, mi.inv_combined); }
            } else {
                if (is_main) { if (spectral) weight = weight * (sigma_n * pick(mi.combined, channel) / pick(sigma_n, channel)); }
                else { if (spectral) weight = weight * sigma_n; else weight = weight * div_by_invariant(sigma_n, mi.combined, mi.inv_combined); }
            }
            if (is_nee) p.wa += mi.t;
            p.ray.o = mi.p; p.ray.mint = 0.f; p.si.t = p.si.t - mi.t;
            p.st = S_TOP;
            if (is_main) p.thr = weight;
            else {
                p.trans = weight;
                if (!any_nonzero(weight)) {                        // volpath.cpp:358 / :456
                    if (DEFER) p.st = is_nee ? S_ENDNEE : S_ENDDIR0;
                    else if (is_nee) end_nee(p, e); else end_direct(p, e, spec_s(0.f), 0.f);
                }
            }
            return;
        }
        // real scattering event of the main path, volpath.cpp:133-160
        p.depth += 1;
        if (!(p.depth < max_depth)) { p.thr = weight; p.flags &= ~FL_ALIVE; p.st = S_TOP; return; }
        if (grey) {
            if (spectral) weight = weight * ((mi.sigma_s.x * mi.combined.x) * pm_rcp(mi.sigma_t.x));
            else weight = weight * (mi.sigma_s.x / mi.sigma_t.x);
        } else {
            if (spectral) weight = weight * (mi.sigma_s * pick(mi.combined, channel) / pick(mi.sigma_t, channel));
            else weight = weight * (mi.sigma_s / mi.sigma_t);
        }
        p.thr = weight;
        const bool sample_emitters = (mi.info & MI_SAMPLE_EMITTERS) != 0;
        p.flags |= FL_VALID_RAY;
        p.flags = sample_emitters ? (p.flags & ~FL_SPEC_CHAIN) : (p.flags | FL_SPEC_CHAIN);
        p.ray.o = mi.p;                                        // scattering position; ray.d stays the incident direction
        p.st = sample_emitters ? S_SCATTER : S_PHASE;
    }
#if MTS_STEP_FAST
    // ================================================================= MEDIUM + loop head as straight-line code (ring driver, lean units a / b / c)
    // blk_med<true, MODEK> followed by top<true> and classify for a path of class B_MED (MODEK 0) or B_MEDW (MODEK 1), where the unit
    // promises the kind of every medium (MT_MEDIA, rgb / mono: heterogeneous, grey, on a pair grid).  Every such path has st == S_MED,
    // no pending intersection and the class's mode(s), in the first round (classify put it in the ring) and in every repeat (wg_block
    // repeats only the lanes that classify sent back here), so none of blk_med's state tests can fail and they are not made.
    // The arithmetic, its order and the draws are blk_med's and top's; what changes is the control structure: no early return, every lane
    // runs the same instructions, the grid lookup of a lane without a collision reads the voxels around its ray origin and drops them,
    // the outcome (escaped / null collision / real collision) picks the new state with selects, and the class follows from the outcome.
    // What blk_med meets on its uncommon paths makes a lane RARE: a medium whose majorant has no invariant reciprocal (rd == 0, found by
    // value: a branch on it would split the record's scalar loads into two round trips), an argument outside the common range of pm_log /
    // pm_exp / pm_div_by_invariant (their *_flag forms), the depth limit at a real collision, a walk whose transmittance became zero.  A rare lane commits nothing -- p still holds the state
    // it came with -- and one wave-uniform branch at the end runs blk_med, top and classify themselves for the rare lanes.  So a lane
    // either runs the general code, or instructions that are the general code's common path.
    template <int MODEK, class E> DEV int step_fast(PathState &p, const E &e) const {
        static_assert(MODEK == 0 || MODEK == 1, "one class of the ring driver");
        constexpr bool is_main = MODEK == 0;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth, rr_depth = (uint32_t) sc.integrator.rr_depth;
        Pcg32 rng = p.rng;
        const float u = rng.next_1d();                         // volpath.cpp:105 / :294 / :391
        bool rare = false, valid_mi = false, sample_emitters = false;
        float mext = 0.f, rd = 0.f, mi_t = pm_inf(), sig_t = 0.f, sig_s = 0.f;
        F3 mi_p = f3s(0.f);
        const float si_t = p.si.t;
        const bool is_nee = !is_main && p.mode == M_NEE;
        const float remaining_dist = is_nee ? p.ray.maxt : pm_inf();
        float w_step = 0.f, u2 = 0.f, u_rr = 0.f, wa = p.wa;   // formed under the gathers, below
        Pcg32 rng_head = rng;
        WATERFALL_BEGIN(p.medium, mu)
            const DMedium m = cload(sc.media + mu);            // medium_step, pair-grid arm
            {                                                  // a majorant without an invariant reciprocal (rd == 0) makes the lane rare by value: no branch splits the record's loads
                float bmint, bmaxt;
                bool active = bbox_ray_intersect(m.aabb, p.ray, bmint, bmaxt);
                active = active && (pm_isfinite(bmint) || pm_isfinite(bmaxt));
                bmint = active ? bmint : 0.f; bmaxt = active ? bmaxt : pm_inf();
                const float mint = pm_max(p.ray.mint, bmint);
                const float maxt = pm_min(p.ray.maxt, bmaxt);
                mext = m.max_density; rd = m.inv_max_density;
                bool ok_log, ok_div;
                const float sampled_t = mint + pm_div_by_invariant_flag(-pm_log_flag(1.f - u, &ok_log), mext, rd, &ok_div);
                rare = !(ok_log && ok_div) || rd == 0.f;
                valid_mi = active && (sampled_t <= maxt);
                mi_t = valid_mi ? sampled_t : pm_inf();
                mi_p = ray_at(p.ray, sampled_t);
                const bool look = valid_mi && !rare;           // every other lane looks up the cell of its ray origin: a valid address, value unused
                const F3 at = f3(look ? mi_p.x : p.ray.o.x, look ? mi_p.y : p.ray.o.y, look ? mi_p.z : p.ray.o.z);
                const int sx = m.pair_nx < 2 ? 2 : m.pair_nx;
                const GridCell c = grid_cell_clamp(m.pair_w2l, m.pair_affine & 1, m.pair_nx, m.pair_ny, m.pair_nz, sx, at);
                const bool columns_equal = (m.pair_affine & 2) != 0;
                GridPairLoads g = grid_pair_issue(as_global(m.pair_grid), c, sx, columns_equal);
                // In the shadow of the gathers: what the step does not need a voxel for -- the distance, its transmittance and
                // sampling weight, the walk's bound, the main path's draws.  The waterfall's loop end is a block boundary that the
                // scheduler does not cross, so this stands inside the body (mext is wave-uniform here); the wait takes the results as
                // operands, which keeps the arithmetic ahead of it.
                mi_t = si_t < mi_t ? pm_inf() : mi_t;          // volpath.cpp:112 / :300 / :397
                float t = pm_min(mi_t, si_t);
                if (!is_main) t = is_nee ? pm_min(remaining_dist, t) : t;
                t = t - mint;
                const bool surface_first = si_t < mi_t || mi_t > remaining_dist;
                bool ok_exp;
                float tr = pm_exp_flag(-t * mext, &ok_exp);
                rare = rare || !ok_exp;
                const float tr_pdf = surface_first ? tr : tr * mext;
                w_step = tr_pdf > 0.f ? tr * pm_rcp(tr_pdf) : 0.f;
                if constexpr (is_main) {
                    u2 = rng.next_1d();                        // volpath.cpp:123 (drawn even when the medium was left)
                    rng_head = rng;
                    u_rr = rng_head.next_1d();                 // the roulette sample of the loop head, used after a null collision
                    grid_gather_wait(g.q00, g.q01, g.q10, g.q11, w_step, mi_t, u2, u_rr);
                } else {                                       // volpath.cpp:313-315 (a direct-light walk has no bound: both tests fail)
                    wa = (mi_t > remaining_dist && mi_t != pm_inf()) ? p.wb : wa;
                    mi_t = mi_t > remaining_dist ? pm_inf() : mi_t;
                    grid_gather_wait(g.q00, g.q01, g.q10, g.q11, w_step, mi_t, wa, tr);
                }
                float st_raw, al_raw;
                grid_pair_blend(g, c, columns_equal, st_raw, al_raw);
                sig_t = m.scale * st_raw;
                if (is_main) sig_s = sig_t * al_raw;
                sample_emitters = m.sample_emitters != 0;
            }
        WATERFALL_END
        Spec weight = is_main ? p.thr : p.trans;
        weight = weight * w_step;
        const bool valid = mi_t != pm_inf();                   // false: escaped_medium, the surface part of this iteration
        const float sigma_n = mext - sig_t;
        int cls;
        if (is_main) {
            bool ok_div2;
            const float ratio = pm_div_by_invariant_flag(sig_t, mext, rd, &ok_div2);
            const bool real = valid && !(u2 >= ratio);         // real scattering event, volpath.cpp:133-160 -- else a null collision, :128-131,140-144
            const uint32_t depth1 = p.depth + 1u;
            rare = rare || (valid && !ok_div2) || (real && !(depth1 < max_depth));
            const float factor = real ? (sig_s * mext) * pm_rcp(sig_t) : (sigma_n * mext) * pm_rcp(sigma_n);
            const Spec stepped = weight * factor;
            Spec thr = f3(valid ? stepped.x : weight.x, valid ? stepped.y : weight.y, valid ? stepped.z : weight.z);
            // the loop head of a null collision: top(), main arm (volpath.cpp:79-87)
            bool alive = (p.flags & FL_ALIVE) && any_nonzero(thr);
            const float q = pm_min(hmax(thr) * (p.eta * p.eta), .95f);
            const bool perform_rr = p.depth > rr_depth;
            alive = alive && (u_rr < q || !perform_rr);
            const Spec thr_rr = thr * pm_rcp(q);
            const bool null_c = valid && !real, rr_c = null_c && perform_rr;
            const bool ends = !alive || p.depth >= max_depth;
            thr = f3(rr_c ? thr_rr.x : thr.x, rr_c ? thr_rr.y : thr.y, rr_c ? thr_rr.z : thr.z);
            const uint32_t fl = p.flags | FL_VALID_RAY;
            const uint32_t st_real = sample_emitters ? S_SCATTER : S_PHASE, st_null = ends ? S_NEW : S_MED;
            const int cls_real = sample_emitters ? B_SCATTER : B_PHASE, cls_null = ends ? B_NEW : B_MED;
            cls = valid ? (real ? cls_real : cls_null) : B_SURF;
            if (!rare) {                                       // commit
                if (COUNT) { cnt.n_lookup += valid_mi ? 1u : 0u; cnt.n_iter += (null_c && !ends) ? 1u : 0u; }
                p.thr = thr;
                p.rng.state = null_c ? rng_head.state : rng.state;
                p.ray.o = f3(valid ? mi_p.x : p.ray.o.x, valid ? mi_p.y : p.ray.o.y, valid ? mi_p.z : p.ray.o.z);
                p.ray.mint = null_c ? 0.f : p.ray.mint;
                p.si.t = null_c ? si_t - mi_t : si_t;
                p.depth = real ? depth1 : p.depth;
                p.flags = real ? (sample_emitters ? (fl & ~FL_SPEC_CHAIN) : (fl | FL_SPEC_CHAIN)) : p.flags;
                p.st = valid ? (real ? st_real : st_null) : S_SURF;
            }
        } else {
            // a step of a walk, volpath.cpp:322-333 / :411-420, and its loop head: top(), NEE and direct arms (:283-287, :385-388)
            const Spec stepped = weight * sigma_n;
            rare = rare || (valid && !any_nonzero(stepped));   // volpath.cpp:358 / :456: the walk is dead
            const float wa_step = is_nee ? wa + mi_t : wa;
            const float left = p.wb * (1.f - MTS_SHADOW_EPSILON) - wa_step;
            const bool ends = is_nee && !(left > 0.f);
            cls = valid ? (ends ? B_NEW /* classify(S_ENDNEE); wg_block's deferred tail ends the walk */ : B_MEDW) : B_WSURF;
            if (!rare) {                                       // commit
                if (COUNT) { cnt.n_lookup += valid_mi ? 1u : 0u; cnt.n_nee_step += (valid && !ends) ? 1u : 0u; }
                p.trans = f3(valid ? stepped.x : weight.x, valid ? stepped.y : weight.y, valid ? stepped.z : weight.z);
                p.rng.state = rng.state;
                p.wa = valid ? wa_step : wa;
                p.ray.o = f3(valid ? mi_p.x : p.ray.o.x, valid ? mi_p.y : p.ray.o.y, valid ? mi_p.z : p.ray.o.z);
                p.ray.mint = valid ? 0.f : p.ray.mint;
                p.ray.maxt = (valid && is_nee) ? left : p.ray.maxt;
                p.si.t = valid ? si_t - mi_t : si_t;
                p.st = valid ? (ends ? S_ENDNEE : S_MED) : S_SURF;
            }
        }
        // the one rare path: the general step from the state the lane came with.  Marked unlikely, so that its blocks leave the loop's layout.
        // (tools/step_loop_stats.py tells the common path from the rare one by the text `__ballot(rare)` of this line.)
        if (__builtin_expect(__ballot(rare) != 0ull, 0)) {
            if (rare) {
                blk_med<true, MODEK>(p, e);
                top<true>(p, e);
                cls = Base::classify(p);
            }
        }
        return cls;
    }
#endif // MTS_STEP_FAST
    // ================================================================= SCATTER: emitter sampling at a medium interaction
    // (volpath.cpp:162-167 -> sample_emitter :261-281); the walk itself runs as M_NEE steps
    template <class E> DEV void blk_scatter(PathState &p, const E &e) const {
        if (p.st != S_SCATTER) return;
        p.st = S_PHASE;
        Spec emitter_val;
        const SpecCtx cx = ctx(p); (void) cx;
        DirSample ds = sample_emitter_direction<INST>(sc, p.ray.o, p.rng.next_2d(), false, emitter_val MTS_CX);
        if (ds.pdf == 0.f) return;
        float phase_val = 0.f;
        WATERFALL_BEGIN(p.medium, mu)
            phase_val = phase_eval<true>(sc, cload(sc.media + mu).phase, -p.ray.d, p.ray.o, ds.d MTS_CX);
        WATERFALL_END
        e.cold.put_spec(C_CW, p.thr * phase_val); e.cold.put_spec(C_EMIT, emitter_val);
        e.cold.put3(C_SO, p.ray.o); e.cold.put3(C_SD, p.ray.d); e.cold.f(C_SMED) = __int_as_float(p.medium);
        p.trans = spec_s(1.f); p.wa = 0.f; p.wb = ds.dist;
        p.ray = spawn_ray(p.ray.o, ds.d); p.ray.mint = 0.f;
        queue_intersection(p);
        p.flags |= FL_FROM_MEDIUM;
        p.mode = M_NEE; p.st = S_TOP;
    }
    // ================================================================= SURFACE step of a walk (volpath.cpp:336-364, :423-462)
    template <class E> DEV void blk_wsurf(PathState &p, const E &e) const {
        if (p.st != S_SURF || p.mode == M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const bool hit = hit_valid(p.si);
        const bool is_nee = p.mode == M_NEE;
        if (is_nee) p.wa += p.si.t;
        int emitter = is_nee ? -1 : sc.environment;
        Surf sf; sf.wi = -p.ray.d; sf.sh.n = f3s(0.f); sf.n = f3s(0.f);
        Spec nt = spec_s(0.f); int is_tr = 0, ext = -1, inte = -1;
        if (hit) {
            WATERFALL_BEGIN(hit_shape<INST>(p.si), su)
                const DShape s = cload(sc.shapes + su);
                if (!is_nee) emitter = s.emitter;
                nt = s.bsdf_type == MTS_BSDF_NULL ? spec_s(1.f) : spec_s(0.f);                // null.cpp:70-73, bsdf.cpp:11-14
                is_tr = s.is_medium_transition; ext = s.exterior; inte = s.interior;
                if (emitter >= 0) complete_surface<GEOM_TABLE, INST>(sc, s, p.si, p.ray.d, sf);
                else if (is_tr) sf.n = hit_geo_normal<GEOM_TABLE, INST>(sc, s, p.si);
            WATERFALL_END
        }
        if (emitter >= 0) {                                    // direct-light walk reached an emitter, volpath.cpp:430-440
            const F3 ref_p = e.cold.get3(C_SO);
            DirSample ds;                                      // render/records.h:168-174
            ds.p = p.si.p; ds.n = sf.sh.n; ds.d = p.si.p - ref_p; ds.dist = norm(ds.d); ds.d = ds.d / ds.dist;
            if (!hit) ds.d = -sf.wi;
            ds.emitter = emitter; ds.pdf = 0.f; ds.delta = false;
            const SpecCtx cx = ctx(p); (void) cx;
            end_direct(p, e, emitter_eval(sc, emitter, sf.wi.z MTS_CX), pdf_emitter_direction(sc, ref_p, ds));
            return;
        }
        if (hit) {
            p.trans = p.trans * nt;
            p.ray = spawn_ray(p.si.p, p.ray.d);
            queue_intersection(p);
            if (is_tr) p.medium = dot(p.ray.d, sf.n) > 0 ? ext : inte;         // interaction.h:178-200
        }
        if (hit && any_nonzero(p.trans)) p.st = S_TOP;
        else if (is_nee) end_nee(p, e);
        else end_direct(p, e, spec_s(0.f), 0.f);
    }
    // ================================================================= SURFACE interaction of the main path (volpath.cpp:184-212)
    // CROSSING (class B_CROSS, wg_block): every lane has a valid hit on a shape with a null BSDF, which is not smooth, and without an
    // emitter (DScene::cross_mask) -- the same statements with those facts as constants: no shape record, no emitter term, no NEE.
    template <bool CROSSING = false, class E> DEV void blk_surf(PathState &p, const E &e) const {
        if (p.st != S_SURF || p.mode != M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth;
        const bool hit = CROSSING ? true : hit_valid(p.si);
        Surf sf; sf.wi = -p.ray.d; sf.n = f3s(0.f); sf.sh.s = sf.sh.t = sf.sh.n = f3s(0.f);
        int emitter = CROSSING ? -1 : sc.environment, bsdf_id = 0;
        F2 tex_uv; tex_uv.x = tex_uv.y = 0.f;                  // TEX: si.uv of the hit
        if (!CROSSING && hit) {
            WATERFALL_BEGIN(hit_shape<INST>(p.si), su)
                const DShape s = cload(sc.shapes + su);
                emitter = s.emitter; bsdf_id = s.bsdf;
                if constexpr (TEX != 0) tex_uv = surface_uv<INST>(sc, s, p.si);
                // the shading frame is only read by emitter evaluation and by the NEE of a smooth BSDF: a null boundary needs neither.
                // Nor does a dielectric or a conductor: its record has no smooth bit, so no emitter sample is drawn here, and blk_bsdf
                // completes the surface itself before it samples; where a specular sheet carries an emitter, the first test completes it.
                // bsdf_flags are the hit's own record's: under a twosided with a smooth side the frame is completed for both sides.
                if (s.emitter >= 0 || (s.bsdf_flags & F_Smooth) != 0) complete_surface<GEOM_TABLE, INST>(sc, s, p.si, p.ray.d, sf);
            WATERFALL_END
        }
        const SpecCtx cx = ctx(p); (void) cx;
        if ((p.flags & FL_SPEC_CHAIN) && emitter >= 0) p.res = p.res + p.thr * emitter_eval(sc, emitter, sf.wi.z MTS_CX);
        if (!hit) { p.flags &= ~FL_ALIVE; p.st = S_TOP; return; }
        p.st = S_BSDF;
        bool active_e = false;
        if constexpr (!CROSSING) {
            WATERFALL_BEGIN(bsdf_id, bu)
                active_e = (cload(sc.bsdfs + bu).flags & F_Smooth) != 0 && (p.depth + 1 < max_depth);
            WATERFALL_END
        }
        if (!active_e) return;
        Spec emitter_val;                                      // volpath.cpp:200-212 -> sample_emitter :261-281
        DirSample ds = sample_emitter_direction<INST>(sc, p.si.p, p.rng.next_2d(), false, emitter_val MTS_CX);
        if (ds.pdf == 0.f) return;
        F3 wo = to_local(sf.sh, ds.d), wi = sf.wi;
        Spec bsdf_val; float bpdf;
        // TEX: a twosided's child depends on the lane -- its side of incidence -- so it is resolved per lane, with three per-lane
        // dword loads of the hit's own record, BEFORE the waterfall; that then runs over the resolved id and its record loads stay
        // wave-uniform (scalar loads into SGPRs).  The flips are per lane too; emitter_eval above read the unflipped sf.wi.z.
        // active_e above read the flags of the hit's own record, the union of both sides' (twosided.cpp:78-88).
        if constexpr (TEX != 0) {
            const BsdfSide side = twosided_side(sc, bsdf_id, wi);
            bsdf_id = side.id;
            if (side.back) { wi.z = -wi.z; wo.z = -wo.z; }
        }
        WATERFALL_BEGIN(bsdf_id, bu)
            DBsdf bsdf = cload(sc.bsdfs + bu);
            float blend_w = 0.f;                               // TEX: a blendbsdf's weight at the hit (the BSDF block evaluates the same again)
            if constexpr (TEX != 0) { if (bsdf.type == MTS_BSDF_BLEND) blend_w = blend_weight(sc, bu, bsdf, tex_uv); else bsdf_apply_textures(sc, bu, bsdf, [&]() { return tex_uv; }); }
            hit_bsdf_eval_pdf<TEX, true>(sc, bsdf, blend_w, tex_uv, wi, wo, bsdf_val, bpdf MTS_CXI(bu));
        WATERFALL_END
        e.cold.put_spec(C_CW, p.thr * bsdf_val * mis_weight(ds.pdf, ds.delta ? 0.f : bpdf)); e.cold.put_spec(C_EMIT, emitter_val);
        e.cold.put_hit(p.si); e.cold.put3(C_SD, p.ray.d); e.cold.f(C_SMED) = __int_as_float(p.medium);
        p.trans = spec_s(1.f); p.wa = 0.f; p.wb = ds.dist;
        p.ray = spawn_ray(p.si.p, ds.d);
        queue_intersection(p);
        p.flags &= ~FL_FROM_MEDIUM;
        p.mode = M_NEE; p.st = S_TOP;
    }
    // ================================================================= BSDF sampling (volpath.cpp:214-252)
    // CROSSING: the BSDF is the null one (blk_surf) -- bsdf_sample on a record that says so, instead of the shape's own
    template <bool CROSSING = false, class E> DEV void blk_bsdf(PathState &p, const E &e) const {
        if (p.st != S_BSDF) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth;
        Surf sf; int bsdf_id = 0, is_tr = 0, ext = -1, inte = -1;
        F2 tex_uv; tex_uv.x = tex_uv.y = 0.f;                  // TEX: si.uv of the hit
        WATERFALL_BEGIN(hit_shape<INST>(p.si), su)
            const DShape s = cload(sc.shapes + su);
            complete_surface<GEOM_TABLE, INST>(sc, s, p.si, p.ray.d, sf);
            if constexpr (TEX != 0) tex_uv = surface_uv<INST>(sc, s, p.si);
            bsdf_id = s.bsdf; is_tr = s.is_medium_transition; ext = s.exterior; inte = s.interior;
        WATERFALL_END
        const float s1 = p.rng.next_1d(); const F2 s2 = p.rng.next_2d();
        BSDFSample bs; Spec bsdf_val;
        const SpecCtx cx = ctx(p); (void) cx;
        if constexpr (CROSSING) {
            DBsdf bsdf = {}; bsdf.type = MTS_BSDF_NULL;            // null.cpp:41-58 reads nothing else of it
            bsdf_val = bsdf_sample(bsdf, sf.wi, s1, s2, bs MTS_CXI(bsdf_id));
        } else {
            F3 wi = sf.wi;
            BsdfSide side; side.id = bsdf_id; side.back = side.none = false;
            if constexpr (TEX != 0) {                               // a twosided's child, per lane and before the waterfall, as in blk_surf
                side = twosided_side(sc, bsdf_id, wi);
                if (side.back) wi.z = -wi.z;
            }
            WATERFALL_BEGIN(side.id, bu)
                DBsdf bsdf = cload(sc.bsdfs + bu);
                float blend_w = 0.f;                           // TEX: a blendbsdf's weight at the hit
                if constexpr (TEX != 0) { if (bsdf.type == MTS_BSDF_BLEND) blend_w = blend_weight(sc, bu, bsdf, tex_uv); else bsdf_apply_textures(sc, bu, bsdf, [&]() { return tex_uv; }); }
                bsdf_val = hit_bsdf_sample<TEX, true>(sc, bsdf, blend_w, tex_uv, wi, s1, s2, bs MTS_CXI(bu));
            WATERFALL_END
            if constexpr (TEX != 0) {
                if (side.back) bs.wo.z = -bs.wo.z;             // twosided.cpp:121
                if (side.none) { zero_bsdf_sample(bs); bsdf_val = spec_s(0.f); }     // wi.z == 0: neither side (:109)
            }
        }
        p.thr = p.thr * bsdf_val;
        p.eta *= bs.eta;
        p.ray = spawn_ray(p.si.p, to_world(sf.sh, bs.wo));
        p.flags |= FL_ALIVE;
        const bool non_null_bsdf = !(bs.sampled_type & F_Null);
        if (non_null_bsdf) { p.depth += 1; p.flags |= FL_VALID_RAY; }
        if (non_null_bsdf && (bs.sampled_type & F_Delta)) p.flags |= FL_SPEC_CHAIN;
        if (bs.sampled_type & F_Smooth) p.flags &= ~FL_SPEC_CHAIN;
        const bool add_emitter = !(bs.sampled_type & F_Delta) && any_nonzero(p.thr) && (p.depth < max_depth);
        const int new_medium = is_tr ? (dot(p.ray.d, sf.n) > 0 ? ext : inte) : p.medium;     // volpath.cpp:249-250
        queue_intersection(p);
        if (add_emitter) { e.cold.f(C_SMED) = __int_as_float(new_medium); p.wb = bs.pdf; p.st = S_DIRB; start_direct(p, e); }   // the walk runs in the old medium
        else { p.medium = new_medium; p.st = S_TOP; }
    }
    // ================================================================= PHASE sampling (volpath.cpp:169-175)
    template <class E> DEV void blk_phase(PathState &p, const E &e) const {
        if (p.st != S_PHASE) return;
        const float s1 = p.rng.next_1d(); const F2 s2 = p.rng.next_2d();      // left-to-right (SURVEY.md 8(a'))
        F3 wo;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(p.medium, mu)
            wo = phase_sample<true>(sc, cload(sc.media + mu).phase, make_frame(p.ray.d), p.ray.o, s1, s2 MTS_CX);   // mi.sh_frame = Frame3f(ray.d), medium.cpp:42
        WATERFALL_END
        p.ray = spawn_ray(p.ray.o, wo); p.ray.mint = 0.0f;
        queue_intersection(p);
        p.flags |= FL_ALIVE;
        p.st = S_TOP;
    }

    // Run the block(s) of class `sel` for this lane (a lane whose state does not match falls through)
    // the deferred tail of a block that ran with DEFER (p holds the full state here)
    template <class E> DEV void finish(PathState &p, const E &e) const {
        if (p.st == S_ENDNEE) end_nee(p, e);
        else if (p.st == S_ENDDIR0) end_direct(p, e, spec_s(0.f), 0.f);
    }
    template <bool DEFER = false, bool SPLIT = false, class E> DEV void run(PathState &p, const E &e, int sel) const {
        switch (sel) {
            case B_NEW: this->blk_new(p, e); break;
            case B_INT: blk_int(p, e); break;
            case B_MED: if (SPLIT) blk_med<DEFER, 0>(p, e); else blk_med<DEFER, -1>(p, e); break;
            case B_MEDW: if (SPLIT) blk_med<DEFER, 1>(p, e); else blk_med<DEFER, -1>(p, e); break;
            case B_SCATTER: blk_scatter(p, e); break;
            case B_WSURF: blk_wsurf(p, e); break;
            case B_SURF: blk_surf(p, e); blk_bsdf(p, e); break;     // no NEE at this surface: the BSDF is sampled in the same visit
            case B_CROSS: blk_surf<true>(p, e); blk_bsdf<true>(p, e); break;
            case B_PHASE: blk_phase(p, e); break;
            default: break;
        }
    }
};

#if MTS_SPEC_N == 3
// ---------------------------------------------------------------------------------------------------------
// Driver 1: one lane = one pixel, state in registers, cold state in LDS, blocks chosen by a per-wave vote.
template <bool COUNT>
DEV void volpath_pixel_flat(const DScene &sc, Pcg32 &rng, const DBlock &blk, uint32_t lx, uint32_t ly, uint32_t sample_count,
                            float *__restrict__ film, ColdStore cold, Counters &cnt, const uint32_t *stop_flag) {
    VolpathMachine<COUNT> vm(sc, cnt);
    PathEnvT<ColdStore> e; e.blk = blk; e.lx = lx; e.ly = ly; e.sample_count = sample_count; e.film = as_global(film); e.cold = cold;
    PathState p; p.rng = rng;
    for (int k = 0; k < 5; ++k) e.cold.f(C_ACC + k) = 0.f;
    e.cold.f(C_SAMPLE) = __uint_as_float(0u);
    vm.begin_sample(p, e);
#if defined(MTSAMD_BLOCKSTATS)
    long long bs_t0 = clock64(); int bs_prev_sel = 20;
    unsigned long long bs_loc[45] = {};                      // laid out like g_blockstats
#endif
    for (uint32_t iter = 0; __ballot(p.st != S_DONE); ++iter) {
        if ((iter & 1023u) == 1023u && stop_requested(stop_flag)) break;       // should_stop(), integrator.h:143-146
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) { long long t = clock64(); bs_loc[24 + bs_prev_sel] += (unsigned long long) (t - bs_t0); bs_t0 = t; bs_prev_sel = 20; }
#endif
        vm.top(p, e);
        // census + vote: run the ONE block most lanes of this wave are waiting for
        int cls = vm.classify(p);
        if (cls == B_MEDW) cls = B_MED;                        // this driver runs the generic MEDIUM block for both
        int sel = B_MED, best = -1;
        for (int b = 0; b < B_CROSS; ++b) { int v = __popcll(__ballot(cls == b)); if (v > best) { best = v; sel = b; } }     // classify() never says B_CROSS
        if (best == 0) continue;
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) {
            bs_loc[sel] += 1ull; bs_loc[12 + sel] += (unsigned long long) best;
            long long t = clock64(); bs_loc[44] += (unsigned long long) (t - bs_t0); bs_t0 = t; bs_prev_sel = sel;
        }
#endif
        vm.run(p, e, sel);
    }
    if (p.st != S_DONE) {                                     // stopped (should_stop()): the finished samples of this pixel go to the film, integrator.cpp:120-130
        float *own = film_entry(sc, blk, lx, ly, e.film);
        for (int k = 0; k < 5; ++k) atomicAdd(own + k, e.cold.f(C_ACC + k));
    }
#if defined(MTSAMD_BLOCKSTATS)
    if (COUNT && __builtin_amdgcn_readfirstlane((int) (threadIdx.x & 63)) == (int) (threadIdx.x & 63))
        for (int k = 0; k < 45; ++k) atomicAdd(&g_blockstats[k], bs_loc[k]);
#endif
}

#endif // MTS_SPEC_N == 3

// ---------------------------------------------------------------------------------------------------------
// Hot path state of the workgroup driver: WG paths (pixels) per workgroup, struct-of-arrays in LDS; cold state lives in HBM.
// Every block class loads / stores only the fields it can touch (ClassFields), which keeps the blocks' register budget small.
// depth shares a dword with the packed small fields (15 bits: a path of more than 32767 scattering events would need to
// survive Russian roulette with probability < 0.95^32000).
// The dwords every tracking step touches come first: an LDS instruction reaches 64 KB (16 fields of 1024 paths) from its address
// register, later fields cost an address computation each.
// MTS_HOT_DRCP: whether 1 / d is part of the state.  It is vrcp(d) wherever a ray is made (make_ray, resume_main) and pm_rcp is a
// function of its argument's bits alone (tests/micro/rcp_exhaustive.hip), so a block that loads d can form it again -- 12 vector
// instructions in place of three LDS reads, three LDS writes less wherever d is stored, 12 KiB of LDS at 1024 paths.  Which units do
// is unit_config.h: those with the ninth ring (MTS_CROSS_CLASS), which is where that ring's 2 KiB come from, and two more; then the front
// is thirteen dwords and the main path's throughput sits inside the 64 KB reach as well.  The other units keep the three dwords.
enum { H_RNG = 0, H_O = 2, H_D = 5, H_DRCP = 8 /* MTS_HOT_DRCP: three dwords, else none */, H_MINT = 8 + 3 * MTS_HOT_DRCP, H_MAXT = H_MINT + 1,
       H_SIT = H_MAXT + 1, H_MEDIUM = H_SIT + 1, H_PACKED = H_MEDIUM + 1 /* st, mode, channel, flags, class, depth */,
       H_FRONT = H_PACKED + 1 /* 16 or 13: the dwords of HotFront; a machine's own fields follow */,
       H_THR = H_FRONT, H_TRANS = H_THR + MTS_SPEC_DW, H_WA = H_TRANS + MTS_SPEC_DW,
       H_WB = H_WA + 1, H_ETA = H_WB + 1, H_RES = H_ETA + 1, H_SIX = H_RES + MTS_SPEC_DW /* si.p, si.uv, si.shape, si.prim */,
#if MTS_SPEC_N == 3
       H_COUNT = H_SIX + 7 };                                   // 35, or 32 without 1 / d
#else
       H_WL = H_SIX + 7 /* the sample's four wavelengths */, H_COUNT = H_WL + 4 };      // 42
#endif

enum : uint32_t { G_RNG = 1, G_O = 2, G_D = 4 /* d and 1/d (stored, or formed on load: MTS_HOT_DRCP) */, G_MINT = 8, G_MAXT = 16, G_SIT = 32 /* si.t */, G_SIX = 64 /* rest of si */,
                  G_MED = 128, G_THR = 256, G_RES = 512, G_ETA = 1024, G_TRANS = 2048, G_WA = 4096, G_WB = 8192,
#if MTS_SPEC_N == 3
                  G_WL = 0, G_ALL = 16383 };
#else
                  G_WL = 16384 /* read by every block that evaluates a spectrum, written by NEW */, G_ALL = 32767 };
#endif
// What block class C (followed by top()) may read (`load`, a superset of `store`) and write (`store`).  end_nee / end_direct touch
// almost everything; the classes with partial sets run them deferred (VolpathMachine::finish on the full state).
template <int C> struct ClassFields { static constexpr uint32_t load = G_ALL, store = G_ALL; static constexpr bool defer = false; };
template <> struct ClassFields<B_MED> {          // main path: tracks thr
    static constexpr uint32_t load = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_MED | G_THR | G_ETA | G_WL,
                              store = G_RNG | G_O | G_MINT | G_SIT | G_THR;
    static constexpr bool defer = true; };
template <> struct ClassFields<B_MEDW> {         // NEE / direct-light walk: tracks trans, the NEE walk also its distance budget
    static constexpr uint32_t load = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_MED | G_TRANS | G_WA | G_WB | G_WL,
                              store = G_RNG | G_O | G_MINT | G_MAXT | G_SIT | G_TRANS | G_WA;
    static constexpr bool defer = true; };
template <> struct ClassFields<B_INT> {          // every lane of the class wants the intersection: si is written, never read
    static constexpr uint32_t load = G_O | G_D | G_MINT | G_MAXT | G_MED | G_TRANS, store = G_SIT | G_SIX | G_TRANS;
    static constexpr bool defer = true; };
template <> struct ClassFields<B_SCATTER> {
    static constexpr uint32_t load = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_MED | G_THR | G_TRANS | G_WA | G_WB | G_WL,
                              store = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_TRANS | G_WA | G_WB;
    static constexpr bool defer = true; };
template <> struct ClassFields<B_CROSS> {        // no emitter sample, no walk, no cold record: the smallest set that samples the null BSDF and spawns the ray
    static constexpr uint32_t load = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_SIX | G_MED | G_THR | G_ETA | G_WL,
                              store = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_MED | G_THR | G_ETA;
    static constexpr bool defer = false; };
template <> struct ClassFields<B_PHASE> {
    static constexpr uint32_t load = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_MED | G_THR | G_ETA | G_WL,
                              store = G_RNG | G_O | G_D | G_MINT | G_MAXT | G_SIT | G_THR;
    static constexpr bool defer = true; };

// The front of a ring machine's hot store, shared by HotStore below and MisHotStore (volpathmis_flat.h): the LDS accessors, the packed
// dword, and the eight field groups G_RNG .. G_MED over the layout H_RNG .. H_PACKED (sixteen dwords, thirteen without 1 / d).  SIX: where the machine keeps the
// rest of the hit (behind its own fields).  The packed dword is stored / unpacked by the derived store, where its own order has it.
template <int WG, int SIX>
struct HotFront {
    uint32_t *base;                                          // &lds[0][path]
    DEV uint32_t &u(int k) const { return base[k * WG]; }
    DEV float f(int k) const { return __uint_as_float(base[k * WG]); }
    DEV void putf(int k, float v) const { base[k * WG] = __float_as_uint(v); }
    DEV void put3(int k, F3 v) const { putf(k, v.x); putf(k + 1, v.y); putf(k + 2, v.z); }
    DEV F3 get3(int k) const { return f3(f(k), f(k + 1), f(k + 2)); }
#if MTS_SPEC_N == 3
    DEV void put_spec(int k, Spec v) const { put3(k, v); }
    DEV Spec get_spec(int k) const { return get3(k); }
#else
    DEV void put_spec(int k, Spec v) const { putf(k, v.x); putf(k + 1, v.y); putf(k + 2, v.z); putf(k + 3, v.w); }
    DEV Spec get_spec(int k) const { return spec4(f(k), f(k + 1), f(k + 2), f(k + 3)); }
#endif
    template <class P> DEV static uint32_t pack(const P &p, int cls) {
        return p.st | (p.mode << 4) | (p.channel << 6) | (p.flags << 8) | ((uint32_t) cls << 13) | ((p.depth < 32767u ? p.depth : 32767u) << 17);
    }
    DEV static int cls_of(uint32_t packed) { return (int) (packed >> 13) & 15; }
    template <class P> DEV static void unpack(uint32_t pk, P &p) {
        p.st = pk & 15u; p.mode = (pk >> 4) & 3u; p.channel = (pk >> 6) & 3u; p.flags = (pk >> 8) & 31u; p.depth = pk >> 17;
    }
    // field groups: a block loads / stores only what it can read / write (ClassFields below)
    template <uint32_t M, class P> DEV void store_front(const P &p) const {
        if (M & G_RNG) { u(H_RNG) = (uint32_t) p.rng.state; u(H_RNG + 1) = (uint32_t) (p.rng.state >> 32); }
        if (M & G_O) put3(H_O, p.ray.o);
        if (M & G_D) { put3(H_D, p.ray.d); if (MTS_HOT_DRCP) put3(H_DRCP, p.ray.d_rcp); }
        if (M & G_MINT) putf(H_MINT, p.ray.mint);
        if (M & G_MAXT) putf(H_MAXT, p.ray.maxt);
        if (M & G_SIT) putf(H_SIT, p.si.t);
        if (M & G_SIX) { put3(SIX, p.si.p); putf(SIX + 3, p.si.uv.x); putf(SIX + 4, p.si.uv.y); u(SIX + 5) = (uint32_t) p.si.shape; u(SIX + 6) = (uint32_t) p.si.prim; }
        if (M & G_MED) u(H_MEDIUM) = (uint32_t) p.medium;
    }
    // ... and loads them; a block that does not load a group finds idle values in its place.  (Written as `if (M & G_X) field = load`
    // over idle values set first, instead of the selects below: lean unit a's volpath kernels 122 -> 121 and 128 -> 127 VGPRs, 23000
    // differing assembly lines.)
    template <uint32_t M, class P> DEV void load_front(P &p) const {
        p.rng.state = 0; p.rng.inc = (PCG32_DEFAULT_STREAM << 1u) | 1u;
        if (M & G_RNG) p.rng.state = (uint64_t) u(H_RNG) | ((uint64_t) u(H_RNG + 1) << 32);
        p.ray.o = (M & G_O) ? get3(H_O) : f3s(0.f);
        p.ray.d = (M & G_D) ? get3(H_D) : f3s(0.f); p.ray.d_rcp = (M & G_D) ? (MTS_HOT_DRCP ? get3(H_DRCP) : vrcp(p.ray.d)) : f3s(0.f);
        p.ray.mint = (M & G_MINT) ? f(H_MINT) : 0.f; p.ray.maxt = (M & G_MAXT) ? f(H_MAXT) : 0.f;
        p.si.t = (M & G_SIT) ? f(H_SIT) : pm_inf();
        p.si.p = f3s(0.f); p.si.uv.x = p.si.uv.y = 0.f; p.si.shape = -1; p.si.prim = 0;
        if (M & G_SIX) { p.si.p = get3(SIX); p.si.uv.x = f(SIX + 3); p.si.uv.y = f(SIX + 4); p.si.shape = (int) u(SIX + 5); p.si.prim = (int) u(SIX + 6); }
        p.medium = (M & G_MED) ? (int) u(H_MEDIUM) : -1;
    }
};

template <int WG>
struct HotStore : HotFront<WG, H_SIX> {
    typedef HotFront<WG, H_SIX> Front;
    using Front::u; using Front::f; using Front::putf; using Front::get3; using Front::put_spec; using Front::get_spec;
    template <uint32_t M> DEV void store_m(const PathState &p, int cls) const {
        this->template store_front<M>(p);
        if (M & G_THR) put_spec(H_THR, p.thr);
        if (M & G_RES) put_spec(H_RES, p.res);
        if (M & G_ETA) putf(H_ETA, p.eta);
        if (M & G_TRANS) put_spec(H_TRANS, p.trans);
#if MTS_SPEC_N != 3
        if (M & G_WL) put_spec(H_WL, p.wl);
#endif
        if (M & G_WA) putf(H_WA, p.wa);
        if (M & G_WB) putf(H_WB, p.wb);
        u(H_PACKED) = Front::pack(p, cls);
    }
    template <uint32_t M> DEV void load_m(PathState &p) const {
        this->template load_front<M>(p);
        p.thr = (M & G_THR) ? get_spec(H_THR) : spec_s(0.f); p.res = (M & G_RES) ? get_spec(H_RES) : spec_s(0.f);
        p.eta = (M & G_ETA) ? f(H_ETA) : 1.f;
        p.trans = (M & G_TRANS) ? get_spec(H_TRANS) : spec_s(0.f); p.wa = (M & G_WA) ? f(H_WA) : 0.f; p.wb = (M & G_WB) ? f(H_WB) : 0.f;
#if MTS_SPEC_N != 3
        p.wl = (M & G_WL) ? get_spec(H_WL) : spec_s(0.f);
#endif
        Front::unpack(u(H_PACKED), p);
    }
    DEV void store(const PathState &p, int cls) const { store_m<G_ALL>(p, cls); }
    DEV void load(PathState &p) const { load_m<G_ALL>(p); }
};

// kernel arguments of render_kernel_wga, re-read by the block functions through the constant address space
struct WgArgs {
    DScene sc; const DBlock *blocks; uint32_t n_blocks, block_size, sample_count; float *film; float *cold_g; uint32_t cold_stride;
    unsigned long long *counters;            // [0..2] loop counters, [MTS_DIAG_BASE ..] ring-stall record
    const uint32_t *stop_flag;               // host-visible word: non-zero = Integrator::cancel() / timeout (integrator.h:143-146)
    // Cost-sorted tiles (round 4).  NULL: workgroup w renders paths w WG .. w WG + WG - 1 of the blocks' concatenated Morton orders (a
    // workgroup sits in ONE spiral block).  Otherwise slot s = (w WG + pid) / 16 holds (block index << 12) | tile: sixteen
    // Morton-consecutive pixels (a 4 x 4 square) of that block; 0xFFFFFFFF = padding.  mts_render sorts the tiles of a launch by the
    // cost its calibration launch measured, so that a workgroup holds pixels of EQUAL cost and its paths finish together -- in a
    // spatial block of an atmosphere seen by a distant sensor the costs differ by a multiple near the horizon, the cheap pixels
    // finished early and four fifths of the paths of such a workgroup were done while the rest kept it (and its 16 waves) resident.
    const uint32_t *tiles; uint32_t n_tiles;
};
// ... and the parameter list of every ring kernel (kernels.hip), which WgArgs mirrors field by field
#define MTS_WG_PARAMS DScene sc, const DBlock *blocks, uint32_t n_blocks, uint32_t block_size, uint32_t sample_count, float *film, float *cold_g, uint32_t cold_stride, \
                      unsigned long long *counters, const uint32_t *stop_flag, const uint32_t *tiles, uint32_t n_tiles
static_assert(sizeof(WgArgs) % 4 == 0, "WgArgs mirrors the kernel parameters");
#define MTS_TILE_PIXELS 16u

template <int WG>
DEV bool wg_env(const WgArgs &a, uint32_t wg_base, uint32_t pid, PathEnvT<ColdStoreHbm> &e) {     // pixel owned by path `pid`; false: outside the block
    const uint32_t ppb = a.block_size * a.block_size;       // a multiple of WG (checked by the launcher)
    e.sample_count = a.sample_count; e.film = as_global(a.film);
    e.cold.base = as_global(a.cold_g) + (size_t) (wg_base + pid) * MTS_COLD_RECORD; e.cold.stride = 1;
    __builtin_assume(((uintptr_t) e.cold.base & 127u) == 0);       // hipMalloc'ed base, 128-byte records: lets neighbouring fields share one wide access
    e.park = as_global(a.cold_g) + ((size_t) a.cold_stride + wg_base + pid) * MTS_COLD_RECORD;      // behind the cold records (volpathmis launches allocate it)
    e.lx = e.ly = 0; e.index = 0;
    if (a.tiles != nullptr) {                               // cost-sorted tiles: the block is per lane (vector loads; only NEW and the start need them)
        const uint32_t slot = (wg_base + pid) / MTS_TILE_PIXELS;
        if (slot >= a.n_tiles) return false;
        const uint32_t ent = as_global(a.tiles)[slot];
        if (ent == 0xFFFFFFFFu) return false;
        const MTS_GLOBAL_AS int32_t *bp = (const MTS_GLOBAL_AS int32_t *) as_global(a.blocks + (ent >> 12));
        e.blk.ox = bp[0]; e.blk.oy = bp[1]; e.blk.sx = bp[2]; e.blk.sy = bp[3]; e.blk.id = (uint32_t) bp[4]; e.blk.sample_base = (uint32_t) bp[5];
        e.blk.film_off_lo = (uint32_t) bp[6]; e.blk.film_off_hi = (uint32_t) bp[7];
        e.index = ((ent & 4095u) * MTS_TILE_PIXELS) | (pid & (MTS_TILE_PIXELS - 1u));
    } else {
        // one spiral block per workgroup.  block_size is a power of two (mts_render rounds it up, as integrator.cpp:91-97 does): shift
        // and mask instead of the ~30 instructions of a 32-bit division, on every block visit
        const uint32_t b = wg_base >> (uint32_t) __builtin_ctz(ppb);   // uniform
        e.index = (wg_base & (ppb - 1u)) + pid;
        if (b >= a.n_blocks) return false;
        e.blk = cload(a.blocks + b);
    }
    e.film += ((size_t) e.blk.film_off_hi << 32) | e.blk.film_off_lo;     // the film slot of the entry's pass (mts_render; 0 with a single pass)
    e.lx = compact_bits(e.index); e.ly = compact_bits(e.index >> 1);      // morton_decode, integrator.cpp:200
    return e.lx < (uint32_t) e.blk.sx && e.ly < (uint32_t) e.blk.sy;
}

// Head of a block function (wg_block, mis_block): the arguments of a non-kernel function arrive in VGPRs; tell the compiler which
// ones are wave-uniform.  Returns the kernarg pointer as an opaque copy and sets the uniform workgroup base.
DEV const MTS_CONST_AS void *block_uniforms(const MTS_CONST_AS void *kernarg_, uint32_t wg_base_, uint32_t &wg_base) {
    const uint64_t ka = (uint64_t) (uintptr_t) kernarg_;
    uint32_t ka_lo = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) ka), ka_hi = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) (ka >> 32));
    asm volatile("" : "+s"(ka_lo), "+s"(ka_hi));             // opaque: scene loads stay inside this block (no hoisting when inlined)
    const MTS_CONST_AS void *kernarg = (const MTS_CONST_AS void *) (uintptr_t) ((uint64_t) ka_lo | ((uint64_t) ka_hi << 32));
    wg_base = (uint32_t) __builtin_amdgcn_readfirstlane((int) wg_base_);
    return kernarg;
}

// The class of a main-path lane that classify() sends to B_SURF: B_CROSS when it arrives there from S_SURF with a valid hit on a shape
// of DScene::cross_mask (null BSDF, not smooth, no emitter; shapes 0 .. 63), else B_SURF -- which is always right, being the general block,
// so every doubtful case (no hit, S_BSDF, a shape beyond the mask) stays there.  HAVE_SHAPE: the block holds si.shape in registers; a
// tracking block does not, and its leaving lanes read that one dword.
// The mask is fetched where it is needed (two dwords of the kernel arguments, a scalar load), not kept from the head of the block.
struct MaskWords { uint32_t lo, hi; };
template <bool HAVE_SHAPE, int WG>
DEV int cross_class(int cls, const PathState &p, const HotStore<WG> &hs, const MTS_CONST_AS void *kernarg) {
    if (cls == B_SURF && p.st == S_SURF && hit_valid(p.si)) {
        // the word as it is stored: in an INST instantiation a member's hit carries 1 + its instance above MTS_INST_SHAPE_BITS bits, so it
        // is >= 64 and stays in B_SURF, and the mask holds bits of the scene's own shapes alone (scene_host.cpp: add_shape)
        static_assert(MTS_INST_SHAPE_BITS >= 6, "a packed member hit must lie beyond the 64 shapes of DScene::cross_mask");
        const uint32_t shape = HAVE_SHAPE ? (uint32_t) p.si.shape : hs.u(H_SIX + 5);
        const MaskWords m = cload_k<MaskWords>((const MTS_CONST_AS char *) kernarg + offsetof(WgArgs, sc) + offsetof(DScene, cross_mask));
        if (shape < 64u && (((shape < 32u ? m.lo : m.hi) >> (shape & 31u)) & 1u) != 0u) cls = B_CROSS;
    }
    return cls;
}

// One block of class C for the path `pid`: load, run (repeat while the path stays in class C and enough lanes do), store.
// WF: wavefront (gpu_*) streams -- one PCG32 per (pixel, sample), seeded with TEA (sampler.cpp:89-92).  The hot state holds only the
// generator's 64-bit state; its increment, which for the scalar variants' streams is the default stream's constant, is recomputed here
// from (pixel, sample index) on every load: a 64-bit TEA of four rounds, ~60 instructions, and one dword of the cold record -- in an
// instantiation of its own, so that the kernels of the scalar streams do not change by an instruction.
// __forceinline__: a real call costs 48 callee-saved VGPR spills + reloads per block visit (measured: 5 TB of scratch writes per render)
template <bool COUNT, int WG, int C, bool WF = false, bool MOMENT = false, int TEX = TEX_NONE>
static __device__ __forceinline__ int wg_block(const MTS_CONST_AS void *kernarg_, uint32_t *hot_lds, uint32_t wg_base_, uint32_t pid, Counters *cnt) {
    uint32_t wg_base;
    const MTS_CONST_AS void *kernarg = block_uniforms(kernarg_, wg_base_, wg_base);
    const WgArgs a = cload_k<WgArgs>(kernarg);
    VolpathMachine<COUNT, MOMENT, MTS_GEOM_LDS != 0, TEX> vm(a.sc, *cnt);
    PathEnvT<ColdStoreHbm> e; wg_env<WG>(a, wg_base, pid, e);
    HotStore<WG> hs; hs.base = hot_lds + pid;
    typedef ClassFields<C> CF;
    // VolpathRing::CROSS, in the blocks a main path can leave towards a surface WITH a hit: the intersection itself, a tracking step
    // that ends at the cached hit, and the end of a direct-light walk, which hands the parked hit back.  Every other block spawns a ray
    // (si.t = inf) or starts a walk; the rare deferred tail could (end_direct) and leaves its crossings to B_SURF.
    constexpr bool CROSS = MTS_CROSS_CLASS && !WF && !MOMENT && (C == B_INT || C == B_MED || C == B_WSURF);
    constexpr bool HAVE_SHAPE = ((CF::load | CF::store) & G_SIX) != 0;
    PathState p;
    if (COUNT && C == B_MED) MTS_SEG_BEGIN(*cnt);
    hs.template load_m<CF::load>(p);
    if (WF && C != B_INT) p.rng.inc = wavefront_increment(a.sc.sensor, e.blk, e.lx, e.ly, __float_as_uint(e.cold.f(C_SAMPLE)));
    if (COUNT && C == B_MED) MTS_SEG(*cnt, 0);
#if defined(MTSAMD_BLOCKSTATS)
    if (COUNT && C == B_SURF) {                               // [9]: the lane-visits of this class that are null-boundary crossings (tools/cross_class_stats.py)
        bool cross = p.st == S_SURF && hit_valid(p.si);
        if (cross) { const DShape &s = a.sc.shapes[hit_shape<TEX == TEX_INST>(p.si)]; cross = s.bsdf_type == MTS_BSDF_NULL && (s.bsdf_flags & F_Smooth) == 0 && s.emitter < 0; }     // DScene::cross_mask's condition
        const unsigned long long m = __ballot(cross);
        if (__builtin_amdgcn_readfirstlane((int) (threadIdx.x & 63)) == (int) (threadIdx.x & 63)) atomicAdd(&g_blockstats[9], (unsigned long long) __popcll(m));
    }
#endif
    int cls;
    // A tracking step is most often followed by another one (null collisions): while at least half of the wave's lanes stay in this
    // class the block runs again on the registers it holds -- no LDS round trip, no ring push, no claim for those paths; lanes that
    // leave wait at the store below.  Measured (C3 / C4, Msamples/s): never 535 / 224, from 32 lanes 548 / 259, from 44 lanes
    // 546 / 255, from 16 lanes 526 / 255, always 397 / 239.
#pragma nounroll
    for (int rounds = 0;; ++rounds) {
#if MTS_STEP_FAST
        if constexpr (C == B_MED || C == B_MEDW) cls = vm.template step_fast<C == B_MED ? 0 : 1>(p, e);      // step, loop head and class in one
        else
#endif
        {
            vm.template run<CF::defer, true>(p, e, C);
            if (COUNT && C == B_MED) MTS_SEG(*cnt, 3);
            vm.template top<CF::defer>(p, e);
            if (COUNT && C == B_MED) MTS_SEG(*cnt, 4);
            cls = vm.classify(p);
        }
        if (C == B_WSURF) {                                     // a walk that left through a boundary face with nothing behind it (queue_intersection:
            if (cls != C || rounds >= 1) break;                 // the ray misses the scene's box) comes straight back to this class to end
            continue;
        }
        if (!(C == B_MED || C == B_MEDW) || cls != C || rounds >= 16) break;
        // tools/step_loop_stats.py finds the repeat loops in the assembly by the text of the next line (`MTS_REPEAT_MIN_W : MTS_REPEAT_MIN`), and
        // tells B_MED from B_MEDW by the text of the lines that form the roulette probability (`(p.eta * p.eta), .95f)`) and an NEE walk's
        // remaining distance (`(1.f - MTS_SHADOW_EPSILON) - `) in top() and step_fast: reword those lines and its anchors together.
        if (__popcll(__ballot(true)) < (C == B_MEDW ? MTS_REPEAT_MIN_W : MTS_REPEAT_MIN)) break;
    }
    if constexpr (CROSS) cls = cross_class<HAVE_SHAPE>(cls, p, hs, kernarg);
    hs.template store_m<CF::store>(p, cls);
    if (COUNT && C == B_MED) MTS_SEG(*cnt, 5);
    if (CF::defer && (p.st == S_ENDNEE || p.st == S_ENDDIR0)) {     // rare tail on the full state
        PathState q;
        hs.template load_m<G_ALL>(q);
        if (WF) q.rng.inc = wavefront_increment(a.sc.sensor, e.blk, e.lx, e.ly, __float_as_uint(e.cold.f(C_SAMPLE)));     // top() draws the roulette sample
        vm.finish(q, e);
        vm.top(q, e);
        cls = vm.classify(q);
        hs.template store_m<G_ALL>(q, cls);
    }
    return cls;
}

// Driver 2, the asynchronous regrouping of a workgroup's paths through LDS rings, is ring_driver.h; this is what it needs to know of
// `volpath`.  WF: wavefront streams (wg_block).
template <bool COUNT_, int WG_, bool WF, bool MOMENT = false, int TEX = TEX_NONE>
struct VolpathRing {
    static constexpr bool COUNT = COUNT_;
    static constexpr int WG = WG_, HOT_DWORDS = H_COUNT, PACKED = H_PACKED;
    typedef PathState State;
    typedef HotStore<WG_> Hot;
    typedef VolpathMachine<COUNT_, MOMENT, MTS_GEOM_LDS != 0, TEX> Machine;
    static constexpr bool GEOM_TABLE = Machine::GEOM_TABLE;      // the driver fills the geometry table
    static constexpr bool CROSS = MTS_CROSS_CLASS && !WF && !MOMENT;      // the machine fills the ring of B_CROSS (wg_block); else the driver keeps eight rings
    static constexpr bool OPAQUE_INIT = MTS_OPAQUE_INIT;                  // unit_config.h: travels with MTS_HOT_DRCP
    template <int NT> DEV static void check_shape() { static_assert(NT <= WG_, "a thread per path at most"); }
    DEV static void init_idle(State &p) {
        p.medium = -1; p.thr = p.res = p.trans = spec_s(0.f); p.eta = 1.f; p.depth = 0; p.channel = 0; p.mode = M_MAIN; p.flags = 0; p.wa = p.wb = 0.f;
#if MTS_SPEC_N != 3
        p.wl = spec_s(0.f);
#endif
    }
    // the block function itself, not a forwarding function: one more layer of inlining changed the code of the flagship kernel
    template <int C> static constexpr auto block = &wg_block<COUNT_, WG_, C, WF, MOMENT, TEX>;
};
// the machines of render_kernel_wga_moment / _tex / _inst (rgb / mono general unit): scalar streams, no counters
template <int WG> using VolpathRingMoment = VolpathRing<false, WG, false, true>;
template <int WG> using VolpathRingTex = VolpathRing<false, WG, false, false, TEX_ON>;
template <int WG> using VolpathRingInst = VolpathRing<false, WG, false, false, TEX_INST>;

} // inline namespace
} // namespace mtsamd
