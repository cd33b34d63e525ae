// volpathmis_flat.h -- volpathmis (integrators/volpathmis.cpp:86-445) on the regrouping machinery of volpath_flat.h and ring_driver.h.
//
// The spectral-MIS volumetric path tracer carries probability-ratio matrices instead of a throughput: p_over_f / p_over_f_nee along
// the path (volpathmis.cpp:117-118), and two more, started from p_over_f, along every emitter-sampling walk (sample_emitter,
// :330-445).  As in volpath_flat.h the three nested loops become one state machine -- a path is (mode, state) and advances one block
// at a time: INTERSECT, MEDIUM step of the path, MEDIUM step of a walk, SCATTER (emitter sampling at a medium interaction), walk
// SURFACE, path SURFACE + BSDF, PHASE, NEW sample -- and the workgroup regroups its paths by the block they wait for through the LDS
// rings of ring_driver.h, the driver it shares with volpath (VolpathMisRing at the end of this file).
// Hot state (round 4): TWO matrix slots per path, not four.  The path's pair (p_over_f, p_over_f_nee) is only read and written
// outside a walk, the walk's pair (p_over_f_uni, p_over_f_nee of sample_emitter) only inside one, and a walk starts from a copy of
// p_over_f (:345-346): start_walk PARKS the path's pair in a second 128-byte cold record (PathEnvT::park, HBM), the two slots then
// hold the walk's pair, and end_nee fetches the path's pair back.  49 hot dwords per path with the 3 x 3 matrices (67 before), 69 with
// the 4 x 4 matrices of the spectral build (MTS_SPEC_N = 4, volpathmis.cpp:66-69; 101 before): two 256-path workgroups per CU
// instead of one, i.e. twice the paths behind the same eight waves.
// The draws happen in the order of the nested formulation (integrator_dev.h, volpathmis_sample) -- results are bit-identical to it
// and to the CPU restatement.  Citations are relative to /root/reference.
#pragma once
#include "volpath_flat.h"

namespace mtsamd {
inline namespace MTS_VARIANT_NS {

// cold record: (delta ? 0 : phase / bsdf pdf) of the pending emitter sample; C_CW holds the phase / bsdf value.  The spectral build's
// record is full (C_COUNT = 32); a walk parks either the scattering position (C_SO) or the surface hit (C_SHIT), never both, so the
// pdf takes the first slot of the one that is free.
#if MTS_SPEC_N == 3
DEV int c_pdfv(bool) { return 30; }
#else
DEV int c_pdfv(bool from_medium) { return from_medium ? C_SHIT : C_SO; }
#endif

template <bool SPEC>
struct MisPathState {
    Pcg32 rng;
    DRay ray; Hit si; int medium;
    MisWeights<SPEC> pf, pn;       // path: p_over_f, p_over_f_nee (volpathmis.cpp:117-118)
    MisWeights<SPEC> wn, wu;       // walk: p_over_f_nee / p_over_f_uni of sample_emitter (:345-346)
    Spec res; F3 lsp;              // result; last_scatter_event.p (:131-132: only the position is read)
#if MTS_SPEC_N != 3
    Spec wl;                       // the sample's wavelengths (integrator.cpp:252)
#endif
    float eta, wa, wb;             // walk: wa = total_dist, wb = ds.dist
    uint32_t depth, channel, st, mode, flags;
};

template <bool COUNT, bool SPEC, bool MOMENT_ = false>
struct VolpathMisMachine : RingMachine<VolpathMisMachine<COUNT, SPEC, MOMENT_>, MisPathState<SPEC>, false> {
    static constexpr bool MOMENT = MOMENT_;                    // RingMachine::blk_new: the `moment` wrapper's eleven-channel tail
    static constexpr bool GEOM_TABLE = false;                  // RingMachine::intersect: the primitive list is walked from the scene records
    static constexpr bool INST = false;                        // instanced scenes render `volpathmis` in the nested kernel
    typedef MisPathState<SPEC> P;
    typedef MisWeights<SPEC> W;
    typedef RingMachine<VolpathMisMachine<COUNT, SPEC, MOMENT_>, P, false> Base;
    using Base::sc; using Base::cnt; using Base::ctx; using Base::queue_intersection;
    DEV VolpathMisMachine(const DScene &sc_, Counters &cnt_) : Base(sc_, cnt_) {}
    // the parked pair: one 128-byte record per path behind the cold records, written and read by one lane as whole lines
    template <class E> DEV static void park_put(const E &e, const W &a, const W &b) {
        constexpr int NR = SPEC ? MTS_SPEC_N : 1;
        for (int i = 0; i < NR; ++i) {
            MTS_GLOBAL_AS float *pa = e.park + MTS_SPEC_N * i, *pb = e.park + MTS_SPEC_N * (NR + i);
            pa[0] = a.r[i].x; pa[1] = a.r[i].y; pa[2] = a.r[i].z; pb[0] = b.r[i].x; pb[1] = b.r[i].y; pb[2] = b.r[i].z;
#if MTS_SPEC_N != 3
            pa[3] = a.r[i].w; pb[3] = b.r[i].w;
#endif
        }
    }
    template <class E> DEV static void park_get(const E &e, W &a, W &b) {
        constexpr int NR = SPEC ? MTS_SPEC_N : 1;
        for (int i = 0; i < NR; ++i) {
            const MTS_GLOBAL_AS float *pa = e.park + MTS_SPEC_N * i, *pb = e.park + MTS_SPEC_N * (NR + i);
            a.r[i].x = pa[0]; a.r[i].y = pa[1]; a.r[i].z = pa[2]; b.r[i].x = pb[0]; b.r[i].y = pb[1]; b.r[i].z = pb[2];
#if MTS_SPEC_N != 3
            a.r[i].w = pa[3]; b.r[i].w = pb[3];
#endif
        }
    }
    DEV bool walk_goes_on(const P &p) const {                  // volpathmis.cpp:438-441
        if (SPEC) return any_nonzero(mis_weight_w(p.wu));
        return any_nonzero(p.wu.r[0]) || any_nonzero(p.wn.r[0]);
    }
    template <class E> DEV void begin_sample(P &p, const E &e) const {      // integrator.cpp:242-264, volpathmis.cpp:98-132
        const DSensor &se = sc.sensor;
        const float px = (float) (e.lx + (uint32_t) e.blk.ox), py = (float) (e.ly + (uint32_t) e.blk.oy);
        if (se.wavefront) seed_wavefront_sample(p.rng, se, e.blk, e.lx, e.ly, __float_as_uint(e.cold.f(C_SAMPLE)));   // gpu_* streams (volpath_flat.h)
        F2 u = p.rng.next_2d();
        F2 position_sample; position_sample.x = px + u.x; position_sample.y = py + u.y;
        F2 aperture_sample; aperture_sample.x = .5f; aperture_sample.y = .5f;
        if (se.needs_aperture_sample) aperture_sample = p.rng.next_2d();
        if (se.shutter_open_time > 0.f) (void) p.rng.next_1d();
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
        e.cold.f(C_POS) = position_sample.x; e.cold.f(C_POS + 1) = position_sample.y; e.cold.f(C_RAYW) = rw.x;
        p.medium = se.medium;
        p.res = spec_s(0.f); p.lsp = f3s(0.f); p.eta = 1.f; p.depth = 0;
        p.pf = mw_full<SPEC>(1.f); p.pn = mw_full<SPEC>(1.f); p.wn = mw_full<SPEC>(1.f); p.wu = mw_full<SPEC>(1.f);
#if MTS_SPEC_N == 3
        p.channel = sc.integrator.monochrome ? 0u : (uint32_t) pm_min(p.rng.next_1d() * 3.f, 2.f);     // volpathmis.cpp:120-124
#else
        p.channel = 0u;                                        // :120-124: a draw in the rgb variants only
#endif
        p.si.p = f3s(0.f); p.si.uv.x = p.si.uv.y = 0.f; p.si.prim = 0; p.si.shape = -1;
        const bool hide_emitters = sc.integrator.hide_emitters != 0;
        p.flags = FL_ALIVE | ((!hide_emitters && sc.environment >= 0) ? FL_VALID_RAY : 0u) | (!hide_emitters ? FL_SPEC_CHAIN : 0u);
        p.wa = p.wb = 0.f;
        queue_intersection(p);
        p.mode = M_MAIN; p.st = S_TOP;
    }
    // emitter-sampling walk finished (volpathmis.cpp:443-444 + :233-236 / :297-299): MIS-weighted contribution, resume the path
    template <class E> DEV void end_nee(P &p, const E &e) const {
        const Spec fval = e.cold.get_spec(C_CW), emitted = e.cold.get_spec(C_EMIT);
        const float pdfv = e.cold.f(c_pdfv((p.flags & FL_FROM_MEDIUM) != 0));
        update_weights(p.wn, 1.0f, fval, p.channel, true);
        update_weights(p.wu, pdfv, fval, p.channel, true);
        p.res = p.res + mis_weight_w(p.wn, p.wu) * emitted;
        park_get(e, p.pf, p.pn);                               // ... and comes back
        this->resume_main(p, e);
    }
    // A block that runs on a partial state (MisClassFields) leaves the end of a walk to finish(), which runs on the full state
    template <bool DEFER, class E> DEV void nee_done(P &p, const E &e) const { if (DEFER) p.st = S_ENDNEE; else end_nee(p, e); }
    template <class E> DEV void finish(P &p, const E &e) const { if (p.st == S_ENDNEE) end_nee(p, e); }
    // loop heads: volpathmis.cpp:134-151 (path), :358-362 (walk)
    template <bool DEFER = false, class E> DEV void top(P &p, const E &e) const {
        if (p.st != S_TOP) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth, rr_depth = (uint32_t) sc.integrator.rr_depth;
        if (p.mode == M_MAIN) {
            bool active = (p.flags & FL_ALIVE) != 0;
            Spec mis_throughput = mis_weight_w(p.pf);
            float q = pm_min(hmax(mis_throughput) * (p.eta * p.eta), .95f);
            bool perform_rr = active && (p.depth > rr_depth);                          // last_event_was_null is never set (:146)
            active = active && !(p.rng.next_1d() >= q && perform_rr);
            update_weights(p.pf, q, 1.0f, p.channel, perform_rr);
            active = active && !(p.depth >= max_depth);
            active = active && any_nonzero(mis_weight_w(p.pf));
            if (!active) p.st = S_NEW;
            else { if (COUNT) cnt.n_iter++; p.st = p.medium >= 0 ? S_MED : S_SURF; }
        } else {
            float remaining_dist = p.wb * (1.f - MTS_SHADOW_EPSILON) - p.wa;
            p.ray.maxt = remaining_dist;
            if (!(remaining_dist > 0.f)) nee_done<DEFER>(p, e);
            else { if (COUNT) cnt.n_nee_step++; p.st = p.medium >= 0 ? S_MED : S_SURF; }
        }
    }
    // ================================================================= INTERSECT
    template <class E> DEV void blk_int(P &p, const E &) const { this->intersect(p); }
    // ================================================================= MEDIUM step of the path (volpathmis.cpp:165-245)
    template <class E> DEV void blk_med(P &p, const E &) const {
        if (p.st != S_MED || p.mode != M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth, channel = p.channel;
        const float u = p.rng.next_1d();
        MedStep mi;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(p.medium, mu)
            mi = medium_step<COUNT>(sc, cload(sc.media + mu), p.ray, u, channel, true, cnt MTS_CX);
        WATERFALL_END
        if (p.si.t < mi.t) mi.t = pm_inf();
        const MediumKind mk = { mi.info };
        const bool spectral = mk.spectral(), homogeneous = mk.homogeneous(), grey = mk.grey();
        const Spec sigma_n = homogeneous ? spec_s(0.f) : mi.combined - mi.sigma_t;
        if (spectral) {
            float t = pm_min(mi.t, p.si.t) - mi.mint;                                  // medium.cpp:77-89
            // a heterogeneous medium's combined extinction is its scalar majorant (heterogeneous.cpp:29): one exponential for every channel
            if (homogeneous) {
                Spec tr = transmittance_exp(t, mi.combined);
                Spec free_flight_pdf = p.si.t < mi.t ? tr : tr * mi.combined;
                update_weights(p.pf, free_flight_pdf, tr, channel, true);
                update_weights(p.pn, free_flight_pdf, tr, channel, true);
            } else {
                const float tr = pm_exp(-t * mi.combined.x), free_flight_pdf = p.si.t < mi.t ? tr : tr * mi.combined.x;
                update_weights_uniform(p.pf, free_flight_pdf, tr);
                update_weights_uniform(p.pn, free_flight_pdf, tr);
            }
        }
        if (mi.t == pm_inf()) { p.st = S_SURF; return; }                               // escaped_medium: the surface part of this iteration
        const bool null_scatter = p.rng.next_1d() >= div_by_invariant(pick(mi.sigma_t, channel), pick(mi.combined, channel), mi.inv_combined);
        if (null_scatter) {
            if (spectral && grey) {
                update_weights_uniform(p.pf, div_by_invariant(sigma_n.x, mi.combined.x, mi.inv_combined), sigma_n.x);
                update_weights_uniform(p.pn, 1.0f, sigma_n.x);
            } else if (spectral) {
                update_weights(p.pf, div_by_invariant(sigma_n, mi.combined, mi.inv_combined), sigma_n, channel, true);
                update_weights(p.pn, 1.0f, sigma_n, channel, true);
            } else {
                update_weights(p.pf, sigma_n, sigma_n, channel, true);
                update_weights(p.pn, 1.0f, div_by_invariant(sigma_n, mi.combined, mi.inv_combined), channel, true);
            }
            p.ray.o = mi.p; p.ray.mint = 0.f; p.si.t = p.si.t - mi.t;
            p.st = S_TOP;
            return;
        }
        p.depth += 1; p.lsp = mi.p;
        const bool sample_emitters = (mi.info & MI_SAMPLE_EMITTERS) != 0;
        if (!(p.depth < max_depth)) { p.flags &= ~FL_ALIVE; p.st = S_TOP; return; }    // :197-198: the path ends at the next loop head
        if (sample_emitters) p.flags &= ~FL_SPEC_CHAIN;                                // :199
        if (spectral && grey) update_weights_uniform(p.pf, div_by_invariant(mi.sigma_t.x, mi.combined.x, mi.inv_combined), mi.sigma_s.x);
        else if (spectral) update_weights(p.pf, div_by_invariant(mi.sigma_t, mi.combined, mi.inv_combined), mi.sigma_s, channel, true);
        else update_weights(p.pf, mi.sigma_t, mi.sigma_s, channel, true);
        p.flags |= FL_VALID_RAY;
        p.ray.o = mi.p;                                                                // scattering position; ray.d stays the incident direction
        p.st = sample_emitters ? S_SCATTER : S_PHASE;
    }
    // ================================================================= SCATTER: emitter sampling at a medium interaction (:228-237 -> :330-356)
    template <bool DEFER, class E> DEV void start_walk(P &p, const E &e, F3 ref_p, const DirSample &ds, Spec emitter_sample_weight, Spec fval, float pdfv, bool from_medium) const {
        park_put(e, p.pf, p.pn);                               // the path's pair leaves the hot state for the duration of the walk
        p.wn = p.pf; p.wu = p.pf;
        Spec emitter_val = emitter_sample_weight * ds.pdf;
        if (ds.pdf == 0.f) emitter_val = spec_s(0.f);
        const bool active = ds.pdf != 0.f;
        update_weights(p.wn, ds.pdf, 1.0f, p.channel, active);
        e.cold.put_spec(C_CW, fval); e.cold.put_spec(C_EMIT, emitter_val);
        e.cold.put3(C_SD, p.ray.d); e.cold.f(C_SMED) = __int_as_float(p.medium);
        if (from_medium) { e.cold.put3(C_SO, p.ray.o); p.flags |= FL_FROM_MEDIUM; }
        else { e.cold.put_hit(p.si); p.flags &= ~FL_FROM_MEDIUM; }
        e.cold.f(c_pdfv(from_medium)) = pdfv;
        p.mode = M_NEE;
        if (!active) { nee_done<DEFER>(p, e); return; }
        p.wa = 0.f; p.wb = ds.dist;
        p.ray = spawn_ray(ref_p, ds.d);
        if (from_medium) p.ray.mint = 0.f;
        queue_intersection(p);
        p.st = S_TOP;
    }
    template <bool DEFER = false, class E> DEV void blk_scatter(P &p, const E &e) const {
        if (p.st != S_SCATTER) return;
        Spec esw;
        const SpecCtx cx = ctx(p); (void) cx;
        DirSample ds = sample_emitter_direction(sc, p.ray.o, p.rng.next_2d(), false, esw MTS_CX);
        float phase_val = 0.f;
        WATERFALL_BEGIN(p.medium, mu)
            phase_val = phase_eval<true>(sc, cload(sc.media + mu).phase, -p.ray.d, p.ray.o, ds.d MTS_CX);
        WATERFALL_END
        start_walk<DEFER>(p, e, p.ray.o, ds, esw, spec_s(phase_val), ds.delta ? 0.f : phase_val, true);
    }
    // ================================================================= MEDIUM step of a walk (volpathmis.cpp:364-411)
    template <bool DEFER = false, class E> DEV void blk_medw(P &p, const E &e) const {
        if (p.st != S_MED || p.mode == M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const uint32_t channel = p.channel;
        const float u = p.rng.next_1d();
        MedStep mi;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(p.medium, mu)
            mi = medium_step<COUNT>(sc, cload(sc.media + mu), p.ray, u, channel, false, cnt MTS_CX);
        WATERFALL_END
        if (p.si.t < mi.t) mi.t = pm_inf();
        const MediumKind mk = { mi.info };
        const bool spectral = mk.spectral(), homogeneous = mk.homogeneous(), grey = mk.grey();
        const Spec sigma_n = homogeneous ? spec_s(0.f) : mi.combined - mi.sigma_t;
        const float remaining_dist = p.ray.maxt;
        if (spectral) {
            float t = pm_min(remaining_dist, pm_min(mi.t, p.si.t)) - mi.mint;
            // a heterogeneous medium's combined extinction is its scalar majorant (heterogeneous.cpp:29): one exponential for every channel
            const bool no_event = p.si.t < mi.t || mi.t > remaining_dist;
            if (homogeneous) {
                Spec tr = transmittance_exp(t, mi.combined);
                Spec free_flight_pdf = no_event ? tr : tr * mi.combined;
                update_weights(p.wn, free_flight_pdf, tr, channel, true);
                update_weights(p.wu, free_flight_pdf, tr, channel, true);
            } else {
                const float tr = pm_exp(-t * mi.combined.x), free_flight_pdf = no_event ? tr : tr * mi.combined.x;
                update_weights_uniform(p.wn, free_flight_pdf, tr);
                update_weights_uniform(p.wu, free_flight_pdf, tr);
            }
        }
        if (mi.t > remaining_dist && mi.t != pm_inf()) p.wa = p.wb;
        if (mi.t > remaining_dist) mi.t = pm_inf();
        if (mi.t == pm_inf()) { p.st = S_SURF; return; }                               // escaped_medium
        p.wa += mi.t;
        p.ray.o = mi.p; p.ray.mint = 0.f; p.si.t = p.si.t - mi.t;
        if (spectral && grey) {
            update_weights_uniform(p.wn, 1.f, sigma_n.x);
            update_weights_uniform(p.wu, div_by_invariant(sigma_n.x, mi.combined.x, mi.inv_combined), sigma_n.x);
        } else if (spectral) {
            update_weights(p.wn, 1.f, sigma_n, channel, true);
            update_weights(p.wu, div_by_invariant(sigma_n, mi.combined, mi.inv_combined), sigma_n, channel, true);
        } else {
            update_weights(p.wn, 1.f, div_by_invariant(sigma_n, mi.combined, mi.inv_combined), channel, true);
            update_weights(p.wu, sigma_n, sigma_n, channel, true);
        }
        if (walk_goes_on(p)) p.st = S_TOP; else nee_done<DEFER>(p, e);
    }
    // ================================================================= SURFACE step of a walk (volpathmis.cpp:413-441)
    template <class E> DEV void blk_wsurf(P &p, const E &e) const {
        if (p.st != S_SURF || p.mode == M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const bool hit = hit_valid(p.si);
        p.wa += p.si.t;
        if (!hit) { end_nee(p, e); return; }
        Spec nt = spec_s(0.f); F3 n = f3s(0.f); int is_tr = 0, ext = -1, inte = -1;
        WATERFALL_BEGIN(hit_shape(p.si), su)
            const DShape s = cload(sc.shapes + su);
            nt = s.bsdf_type == MTS_BSDF_NULL ? spec_s(1.f) : spec_s(0.f);
            is_tr = s.is_medium_transition; ext = s.exterior; inte = s.interior;
            if (is_tr) n = hit_geo_normal(sc, s, p.si);
        WATERFALL_END
        update_weights(p.wn, 1.0f, nt, p.channel, true);
        update_weights(p.wu, 1.0f, nt, p.channel, true);
        p.ray = spawn_ray(p.si.p, p.ray.d);
        queue_intersection(p);
        const bool go_on = walk_goes_on(p);
        if (is_tr) p.medium = dot(p.ray.d, n) > 0 ? ext : inte;
        if (go_on) p.st = S_TOP; else end_nee(p, e);
    }
    // ================================================================= SURFACE interaction of the path (volpathmis.cpp:253-300)
    template <class E> DEV void blk_surf(P &p, const E &e) const {
        if (p.st != S_SURF || p.mode != M_MAIN || (p.flags & FL_NEEDS_INT)) return;
        const uint32_t max_depth = (uint32_t) sc.integrator.max_depth;
        const bool hide_emitters = sc.integrator.hide_emitters != 0;
        const bool hit = hit_valid(p.si);
        Surf sf; sf.wi = -p.ray.d; sf.n = f3s(0.f); sf.sh.s = sf.sh.t = sf.sh.n = f3s(0.f);
        int emitter = sc.environment, bsdf_id = 0;
        if (hit) {
            WATERFALL_BEGIN(hit_shape(p.si), su)
                const DShape s = cload(sc.shapes + su);
                emitter = s.emitter; bsdf_id = s.bsdf;
                complete_surface(sc, s, p.si, p.ray.d, sf);
            WATERFALL_END
        }
        const bool count_direct = p.depth == 0 || (p.flags & FL_SPEC_CHAIN);
        const SpecCtx cx = ctx(p); (void) cx;
        if (emitter >= 0 && !(p.depth == 0 && hide_emitters)) {
            if (!count_direct) {
                DirSample ds;                                                          // records.h:168-174
                ds.p = p.si.p; ds.n = sf.sh.n; ds.d = p.si.p - p.lsp; ds.dist = norm(ds.d); ds.d = ds.d / ds.dist;
                if (!hit) ds.d = -sf.wi;
                ds.emitter = emitter; ds.pdf = 0.f; ds.delta = false;
                float emitter_pdf = pdf_emitter_direction(sc, p.lsp, ds);
                update_weights(p.pn, emitter_pdf, 1.f, p.channel, true);
            }
            Spec emitted = emitter_eval(sc, emitter, sf.wi.z MTS_CX);
            p.res = p.res + (count_direct ? mis_weight_w(p.pf) * emitted : mis_weight_w(p.pf, p.pn) * emitted);
        }
        if (!hit) { p.flags &= ~FL_ALIVE; p.st = S_TOP; return; }
        p.st = S_BSDF;
        bool active_e = false;
        WATERFALL_BEGIN(bsdf_id, bu)
            active_e = (cload(sc.bsdfs + bu).flags & F_Smooth) != 0 && (p.depth + 1 < max_depth);
        WATERFALL_END
        if (!active_e) return;
        Spec esw;
        DirSample ds = sample_emitter_direction(sc, p.si.p, p.rng.next_2d(), false, esw MTS_CX);
        F3 wo = to_local(sf.sh, ds.d);
        Spec bsdf_val; float bpdf;
        WATERFALL_BEGIN(bsdf_id, bu)
            const DBsdf bsdf = cload(sc.bsdfs + bu);
            bsdf_val = bsdf_eval(bsdf, sf.wi, wo MTS_CXI(bu));
            bpdf = bsdf_pdf(bsdf, sf.wi, wo MTS_CXI(bu));
        WATERFALL_END
        start_walk<false>(p, e, p.si.p, ds, esw, bsdf_val, ds.delta ? 0.f : bpdf, false);
    }
    // ================================================================= BSDF sampling (volpathmis.cpp:302-328)
    template <class E> DEV void blk_bsdf(P &p, const E &) const {
        if (p.st != S_BSDF) return;
        Surf sf; int bsdf_id = 0, is_tr = 0, ext = -1, inte = -1;
        WATERFALL_BEGIN(hit_shape(p.si), su)
            const DShape s = cload(sc.shapes + su);
            complete_surface(sc, s, p.si, p.ray.d, sf);
            bsdf_id = s.bsdf; is_tr = s.is_medium_transition; ext = s.exterior; inte = s.interior;
        WATERFALL_END
        const float s1 = p.rng.next_1d(); const F2 s2 = p.rng.next_2d();
        BSDFSample bs; Spec bsdf_weight;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(bsdf_id, bu)
            const DBsdf bsdf = cload(sc.bsdfs + bu);
            bsdf_weight = bsdf_sample(bsdf, sf.wi, s1, s2, bs MTS_CXI(bu));
        WATERFALL_END
        const bool invalid_bsdf_sample = bs.pdf == 0.f;
        const bool active_surface = bs.pdf > 0.f;
        if (active_surface) p.eta *= bs.eta;
        if (active_surface) { p.ray = spawn_ray(p.si.p, to_world(sf.sh, bs.wo)); queue_intersection(p); }
        const bool non_null_bsdf = active_surface && !(bs.sampled_type & F_Null);
        if (non_null_bsdf || invalid_bsdf_sample) p.flags |= FL_VALID_RAY;
        if (non_null_bsdf && (bs.sampled_type & F_Delta)) p.flags |= FL_SPEC_CHAIN;
        if (active_surface && (bs.sampled_type & F_Smooth)) p.flags &= ~FL_SPEC_CHAIN;
        if (non_null_bsdf) { p.depth += 1; p.lsp = p.si.p; p.pn = p.pf; }
        update_weights(p.pf, bs.pdf, bsdf_weight * bs.pdf, p.channel, active_surface);
        update_weights(p.pn, 1.f, bsdf_weight * bs.pdf, p.channel, non_null_bsdf);
        if (active_surface && is_tr) p.medium = dot(p.ray.d, sf.n) > 0 ? ext : inte;
        if (!active_surface) p.flags &= ~FL_ALIVE;                                     // :327: active &= (active_surface | active_medium)
        p.st = S_TOP;
    }
    // ================================================================= PHASE sampling (volpathmis.cpp:239-251)
    template <class E> DEV void blk_phase(P &p, const E &) const {
        if (p.st != S_PHASE) return;
        p.pn = p.pf;                                                                   // :240: a real interaction resets p_over_f_nee
        const float s1 = p.rng.next_1d(); const F2 s2 = p.rng.next_2d();
        F3 wo; float phase_pdf = 0.f;
        const SpecCtx cx = ctx(p); (void) cx;
        WATERFALL_BEGIN(p.medium, mu)
            wo = phase_sample_pdf(sc, cload(sc.media + mu).phase, make_frame(p.ray.d), p.ray.o, s1, s2, phase_pdf MTS_CX);
        WATERFALL_END
        p.ray = spawn_ray(p.ray.o, wo); p.ray.mint = 0.0f;
        queue_intersection(p);
        update_weights(p.pf, phase_pdf, phase_pdf, p.channel, true);
        update_weights(p.pn, 1.f, phase_pdf, p.channel, true);
        p.st = S_TOP;
    }
    template <bool DEFER, class E> DEV void run(P &p, const E &e, int sel) const {
        switch (sel) {
            case B_NEW: this->blk_new(p, e); break;
            case B_INT: blk_int(p, e); break;
            case B_MED: blk_med(p, e); break;
            case B_MEDW: blk_medw<DEFER>(p, e); break;
            case B_SCATTER: blk_scatter<DEFER>(p, e); break;
            case B_WSURF: blk_wsurf(p, e); break;
            case B_SURF: blk_surf(p, e); blk_bsdf(p, e); break;
            case B_PHASE: blk_phase(p, e); break;
            default: break;
        }
    }
};

// Hot state in LDS, struct of arrays over the workgroup's paths (as HotStore of volpath_flat.h).  A block loads / stores only the field
// groups its class can read / write (MisClassFields); at two waves per SIMD the register budget of 256 VGPRs holds the whole state.
enum : uint32_t { K_RNG = G_RNG, K_O = G_O, K_D = G_D, K_MINT = G_MINT, K_MAXT = G_MAXT, K_SIT = G_SIT, K_SIX = G_SIX, K_MED = G_MED,   // HotFront's groups
                  K_PF = 256, K_PN = 512, K_WN = 1024, K_WU = 2048, K_RES = 4096, K_LSP = 8192, K_ETA = 16384, K_WA = 32768, K_WB = 65536,
#if MTS_SPEC_N == 3
                  K_WL = 0, K_ALL = 131071 };
#else
                  K_WL = 131072 /* the sample's wavelengths: read by every block that evaluates a spectrum, written by NEW */, K_ALL = 262143 };
#endif
// What block class C (followed by top()) may read (`load`, a superset of `store`) and write (`store`); `defer`: the end of a walk,
// which touches almost everything, runs afterwards on the full state (VolpathMisMachine::finish).
template <int C> struct MisClassFields { static constexpr uint32_t load = K_ALL, store = K_ALL; static constexpr bool defer = false; };
template <> struct MisClassFields<B_INT> {
    static constexpr uint32_t load = K_O | K_D | K_MINT | K_MAXT, store = K_SIT | K_SIX; static constexpr bool defer = true; };
template <> struct MisClassFields<B_MED> {       // the path: p_over_f, p_over_f_nee; the loop head reads eta
    static constexpr uint32_t load = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_MED | K_PF | K_PN | K_ETA | K_LSP | K_WL,
                              store = K_RNG | K_O | K_MINT | K_SIT | K_PF | K_PN | K_LSP;
    static constexpr bool defer = true; };
template <> struct MisClassFields<B_MEDW> {      // a walk: its two matrices and its distance budget
    static constexpr uint32_t load = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_MED | K_WN | K_WU | K_WA | K_WB | K_WL,
                              store = K_RNG | K_O | K_MINT | K_MAXT | K_SIT | K_WN | K_WU | K_WA;
    static constexpr bool defer = true; };
template <> struct MisClassFields<B_SCATTER> {
    static constexpr uint32_t load = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_MED | K_PF | K_PN /* parked by start_walk */ | K_WA | K_WB | K_WL,
                              store = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_WN | K_WU | K_WA | K_WB;
    static constexpr bool defer = true; };
template <> struct MisClassFields<B_PHASE> {
    static constexpr uint32_t load = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_MED | K_PF | K_ETA | K_WL,
                              store = K_RNG | K_O | K_D | K_MINT | K_MAXT | K_SIT | K_PF | K_PN;
    static constexpr bool defer = true; };

// MisHotStore's own dwords, behind HotFront's (H_RNG .. H_PACKED: H_FRONT = 16 dwords, 13 in the units that do not store 1 / d)
enum { MH_WA = H_FRONT, MH_WB = MH_WA + 1, MH_ETA = MH_WB + 1, MH_RES = MH_ETA + 1, MH_LSP = MH_RES + MTS_SPEC_DW, MH_SIX = MH_LSP + 3,
#if MTS_SPEC_N == 3
       MH_W = MH_SIX + 7 };                                         // 32 (29)
#else
       MH_WL = MH_SIX + 7, MH_W = MH_WL + 4 };                      // 37
#endif
template <int WG, bool SPEC>
struct MisHotStore : HotFront<WG, MH_SIX> {
    typedef HotFront<WG, MH_SIX> Front;
    using Front::u; using Front::f; using Front::putf; using Front::put3; using Front::get3; using Front::put_spec; using Front::get_spec;
    static constexpr int NW = SPEC ? MTS_SPEC_N * MTS_SPEC_N : MTS_SPEC_N;      // floats per weight matrix
    enum { MH_COUNT = MH_W + 2 * NW };            // two matrix slots: A = p_over_f or the walk's p_over_f_uni, B = p_over_f_nee of the path or of the walk
    DEV void putw(int k, const MisWeights<SPEC> &w) const { for (int i = 0; i < NW / MTS_SPEC_N; ++i) put_spec(k + MTS_SPEC_N * i, w.r[i]); }
    DEV MisWeights<SPEC> getw(int k) const { MisWeights<SPEC> w; for (int i = 0; i < NW / MTS_SPEC_N; ++i) w.r[i] = get_spec(k + MTS_SPEC_N * i); return w; }
    template <uint32_t M> DEV void store_m(const MisPathState<SPEC> &p, int cls) const {
        this->template store_front<M>(p);
        u(H_PACKED) = Front::pack(p, cls);
        if (M & K_WA) putf(MH_WA, p.wa);
        if (M & K_WB) putf(MH_WB, p.wb);
        if (M & K_ETA) putf(MH_ETA, p.eta);
        if (M & K_RES) put_spec(MH_RES, p.res);
        if (M & K_LSP) put3(MH_LSP, p.lsp);
#if MTS_SPEC_N != 3
        if (M & K_WL) put_spec(MH_WL, p.wl);
#endif
        // slot A / slot B: the path's pair outside a walk, the walk's pair inside one (a block that can hold either -- K_ALL -- picks by mode)
        constexpr bool path_a = (M & K_PF) != 0, walk_a = (M & K_WU) != 0, path_b = (M & K_PN) != 0, walk_b = (M & K_WN) != 0;
        if (path_a && walk_a) putw(MH_W, p.mode == M_MAIN ? p.pf : p.wu); else if (path_a) putw(MH_W, p.pf); else if (walk_a) putw(MH_W, p.wu);
        if (path_b && walk_b) putw(MH_W + NW, p.mode == M_MAIN ? p.pn : p.wn); else if (path_b) putw(MH_W + NW, p.pn); else if (walk_b) putw(MH_W + NW, p.wn);
    }
    template <uint32_t M> DEV void load_m(MisPathState<SPEC> &p) const {
        this->template load_front<M>(p);
        Front::unpack(u(H_PACKED), p);
        p.wa = (M & K_WA) ? f(MH_WA) : 0.f; p.wb = (M & K_WB) ? f(MH_WB) : 0.f; p.eta = (M & K_ETA) ? f(MH_ETA) : 1.f;
        p.res = (M & K_RES) ? get_spec(MH_RES) : spec_s(0.f); p.lsp = (M & K_LSP) ? get3(MH_LSP) : f3s(0.f);
#if MTS_SPEC_N != 3
        p.wl = (M & K_WL) ? get_spec(MH_WL) : spec_s(0.f);
#endif
        // a block that may meet either pair (K_ALL) reads the two slots once; which pair they are follows from the mode, the other is never read
        const MisWeights<SPEC> slot_a = (M & (K_PF | K_WU)) ? getw(MH_W) : mw_full<SPEC>(1.f), slot_b = (M & (K_PN | K_WN)) ? getw(MH_W + NW) : mw_full<SPEC>(1.f);
        p.pf = slot_a; p.wu = slot_a; p.pn = slot_b; p.wn = slot_b;
    }
    DEV void store(const MisPathState<SPEC> &p, int cls) const { store_m<K_ALL>(p, cls); }
    DEV void load(MisPathState<SPEC> &p) const { load_m<K_ALL>(p); }
};

// One block of class C for the path `pid` (the class is wave-uniform, the blocks are inlined as in volpath_flat.h)
template <bool COUNT, bool SPEC, int WG, int C, bool MOMENT = false>
static __device__ __forceinline__ int mis_block(const MTS_CONST_AS void *kernarg_, uint32_t *hot_lds, uint32_t wg_base_, uint32_t pid, Counters *cnt) {
    uint32_t wg_base;
    const MTS_CONST_AS void *kernarg = block_uniforms(kernarg_, wg_base_, wg_base);
    const WgArgs a = cload_k<WgArgs>(kernarg);
    VolpathMisMachine<COUNT, SPEC, MOMENT> vm(a.sc, *cnt);
    PathEnvT<ColdStoreHbm> e; wg_env<WG>(a, wg_base, pid, e);
    MisHotStore<WG, SPEC> hs; hs.base = hot_lds + pid;
    typedef MisClassFields<C> CF;
    MisPathState<SPEC> p;
    hs.template load_m<CF::load>(p);
    int cls;
#pragma nounroll
    for (int rounds = 0;; ++rounds) {                           // tracking steps repeat in place while half the wave stays (volpath_flat.h, wg_block)
        vm.template run<CF::defer>(p, e, C);
        vm.template top<CF::defer>(p, e);
        cls = vm.classify(p);
        if (C == B_WSURF) {                                     // a walk that left the scene's box ends in the same visit (volpath_flat.h, wg_block)
            if (cls != C || rounds >= 1) break;
            continue;
        }
        if (!(C == B_MED || C == B_MEDW) || cls != C || rounds >= 16) break;
        if (__popcll(__ballot(true)) < MTS_REPEAT_MIN) break;
    }
    hs.template store_m<CF::store>(p, cls);
    if (CF::defer && p.st == S_ENDNEE) {                        // the end of a walk, on the full state
        MisPathState<SPEC> q;
        hs.template load_m<K_ALL>(q);
        vm.finish(q, e);
        vm.top(q, e);
        cls = vm.classify(q);
        hs.template store_m<K_ALL>(q, cls);
    }
    return cls;
}

// What the ring driver (ring_driver.h) needs to know of `volpathmis`
template <bool COUNT_, bool SPEC, int WG_, bool MOMENT = false>
struct VolpathMisRing {
    static constexpr bool COUNT = COUNT_;
    static constexpr int WG = WG_, HOT_DWORDS = MisHotStore<WG_, SPEC>::MH_COUNT, PACKED = H_PACKED;
    typedef MisPathState<SPEC> State;
    typedef MisHotStore<WG_, SPEC> Hot;
    typedef VolpathMisMachine<COUNT_, SPEC, MOMENT> Machine;
    static constexpr bool GEOM_TABLE = false;                  // no geometry table: the driver fills none for this machine
    static constexpr bool OPAQUE_INIT = MTS_OPAQUE_INIT;        // unit_config.h: travels with MTS_HOT_DRCP
    static constexpr bool CROSS = false;                       // ... and no ring of B_CROSS: the machine never names the class
    template <int NT> DEV static void check_shape() { static_assert(NT <= 2 * WG_, "up to two threads per path (768 on 512: a third wave per SIMD)"); }
    DEV static void init_idle(State &p) {
        p.medium = -1; p.res = spec_s(0.f); p.lsp = f3s(0.f); p.eta = 1.f; p.depth = 0; p.channel = 0; p.mode = M_MAIN; p.flags = 0; p.wa = p.wb = 0.f;
#if MTS_SPEC_N != 3
        p.wl = spec_s(0.f);
#endif
        p.pf = p.pn = p.wn = p.wu = mw_full<SPEC>(1.f);
    }
    template <int C> static constexpr auto block = &mis_block<COUNT_, SPEC, WG_, C, MOMENT>;
};
template <bool SPEC, int WG> using VolpathMisRingMoment = VolpathMisRing<false, SPEC, WG, true>;      // the machine of render_kernel_wga_mis_moment: no counters

} // inline namespace
} // namespace mtsamd
