// render_plan.cpp -- see render_plan.h.  Compiled inside capi.cpp's translation unit (and alone by tests/test_render_plan.py).
#include "render_plan.h"
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mtsamd {

// the index of the switch's value in `values`; `unset` without one
static int one_of(const char *name, std::initializer_list<const char *> values, int unset) {
    const char *v = getenv(name);
    if (!v) return unset;
    std::string all;
    int k = 0;
    for (const char *a : values) { if (!strcmp(v, a)) return k; all += (k++ ? ", " : "") + std::string(a); }
    throw std::runtime_error(std::string(name) + " must be one of " + all);
}

RenderSwitches read_render_switches() {
    RenderSwitches sw;
    static const int KERNELS[] = { kv::NESTED, kv::FLAT, kv::ring(256), kv::ring(1024) };
    const int kernel = one_of("MTSAMD_KERNEL", { "nested", "flat", "wga256", "wga1024" }, -1);
    sw.kernel = kernel < 0 ? -1 : KERNELS[kernel];
    sw.lean = one_of("MTSAMD_LEAN", { "0", "1", "2" }, 1);
    sw.lpt = one_of("MTSAMD_LPT", { "0", "1", "2", "3" }, -1);
    sw.pass_slots = one_of("MTSAMD_PASS_SLOTS", { "0", "1" }, 1) != 0;
    sw.lpt_debug = getenv("MTSAMD_LPT_DEBUG") != nullptr;
    if (const char *sv = getenv("MTSAMD_WAVEFRONT_SPLIT")) {
        char *end = nullptr; const long v = strtol(sv, &end, 10);
        if (end == sv || *end != '\0' || v < 1) throw std::runtime_error("MTSAMD_WAVEFRONT_SPLIT must be a positive integer");
        sw.wavefront_split = (size_t) v;
    }
    if (const char *iv = getenv("MTSAMD_TEST_INJECT_LOST_PATH")) {
        char *end = nullptr; errno = 0; const unsigned long long v = strtoull(iv, &end, 10);
        if (!isdigit((unsigned char) *iv) || *end != '\0' || errno == ERANGE) throw std::runtime_error("MTSAMD_TEST_INJECT_LOST_PATH must be a non-negative integer");
        sw.inject_lost_path = v;
    }
    return sw;
}

// ---- The kernel table (render_plan.h).  The rows are read off the launchers of kernels.hip, unit by unit.
const KernelRow KERNEL_ROWS[] = {
    // unit, variant, integrator, spectral MIS, wavefront streams, spectral build
    // the general kernels of the rgb / mono build (kernels.hip)
    { UNIT_GENERAL, kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_GENERAL, kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_YES,    false },     // the instantiation that recomputes the generator's increment (WF)
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_GENERAL, kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },
    { UNIT_GENERAL, kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_NO,     false },
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_NO,     false },
    { UNIT_GENERAL, kv::FLAT,       MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_EITHER, false },     // the flat state machine per lane
    { UNIT_GENERAL, kv::FLAT,       MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, false },     // one flat loop with regeneration (path_pixel_flat)
    { UNIT_GENERAL, kv::FLAT,       MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_EITHER, false },     // `volpathmis` has no flat kernel per lane: the launcher runs
    { UNIT_GENERAL, kv::FLAT,       MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_EITHER, false },     // the nested one (blocks below 256 pixels, MTSAMD_KERNEL=flat)
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, false },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_EITHER, false },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_EITHER, false },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_EITHER, false },
    // the general kernels of the spectral build (kernels_spectral.hip): four-wide state, 256-path workgroups
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     true },
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     true },
    { UNIT_GENERAL, kv::ring(256),  MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_NO,     true },
    { UNIT_GENERAL, kv::FLAT,       MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, true },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, true },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_EITHER, true },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_EITHER, true },
    { UNIT_GENERAL, kv::NESTED,     MTS_INTEGRATOR_VOLPATHMIS, ROW_NO,     ROW_EITHER, true },
#if !defined(MTSAMD_BLOCKSTATS)                                 // the diagnostic build compiles no lean unit
    // a / b / c / h: the regrouping machines of rgb / mono `volpath` and of `volpathmis` with spectral MIS
    { UNIT_A,       kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_A,       kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },     // its 512 paths served by 768 threads
    { UNIT_B,       kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_B,       kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },
    { UNIT_C,       kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_C,       kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },
    { UNIT_H,       kv::ring(1024), MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     false },
    { UNIT_H,       kv::ring(512),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     false },
    // s: the same machines of the spectral build
    { UNIT_S,       kv::ring(256),  MTS_INTEGRATOR_VOLPATH,    ROW_EITHER, ROW_NO,     true },
    { UNIT_S,       kv::ring(256),  MTS_INTEGRATOR_VOLPATHMIS, ROW_YES,    ROW_NO,     true },
    // p / ps: `path` as the flat loop
    { UNIT_P,       kv::FLAT,       MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, false },
    { UNIT_PS,      kv::FLAT,       MTS_INTEGRATOR_PATH,       ROW_EITHER, ROW_EITHER, true },
#endif
};
// In order of preference: the first unit whose promises a scene keeps and which has a row for it renders it.
const UnitRecord KERNEL_UNITS[] = {
#if !defined(MTSAMD_BLOCKSTATS)
    { UNIT_A,  MT_UNIT_A },                                     // every promise: no call left
    { UNIT_B,  MT_UNIT_B },                                     // rpv and grids behind volume_eval() allowed
    { UNIT_C,  MT_UNIT_C },                                     // ... and a BVH
    { UNIT_H,  MT_UNIT_H },                                     // homogeneous media
    { UNIT_S,  MT_UNIT_B },
    { UNIT_P,  MT_UNIT_P_NEEDS },                               // compiled with MT_UNIT_P, of which `path` can reach these: a walked
    { UNIT_PS, MT_UNIT_P_NEEDS },                               // primitive list, no spheres, no rpv
#endif
    { UNIT_GENERAL, 0 },
};
const size_t KERNEL_ROW_COUNT = sizeof(KERNEL_ROWS) / sizeof(KERNEL_ROWS[0]), KERNEL_UNIT_COUNT = sizeof(KERNEL_UNITS) / sizeof(KERNEL_UNITS[0]);

// The render kernel of a scene, the one place that uses MTSAMD_KERNEL and MTSAMD_LEAN: the variant by the rules below, then the first
// unit in order of preference whose promises the scene keeps and whose rows carry that variant for the scene.
KernelChoice choose_kernel(const KernelFacts &f, uint32_t block_size, const RenderSwitches &sw) {
    const bool path = f.integrator == MTS_INTEGRATOR_PATH, vol = f.integrator == MTS_INTEGRATOR_VOLPATH, mis = f.integrator == MTS_INTEGRATOR_VOLPATHMIS, spectral = f.spectral;
    // MTSAMD_KERNEL = nested | flat | wga256 | wga1024 (default: asynchronous regrouping, 1024 paths served by 1024 threads)
    int variant = sw.kernel >= 0 ? sw.kernel : kv::ring(1024);
    // without media there are no tracking walks to regroup: the per-lane kernels win (cornell box 512 x 512 x 256, volpath: rings 992,
    // per lane 1242 Msamples/s; `path` per lane: 2342, as one flat loop with regeneration 2910)
    if (sw.kernel < 0 && !f.has_media && !path) variant = kv::NESTED;
    if (path) variant = variant != kv::NESTED ? kv::FLAT : kv::NESTED;      // per lane: flat loop with regeneration (every variant), or nested (MTSAMD_KERNEL=nested)
    if (kv::is_ring(variant)) {
        uint32_t wg = (uint32_t) kv::ring_paths(variant);
        if (mis) wg = std::min(wg, 512u);                       // four weight matrices per path: 512 paths fill the LDS
        if (spectral) wg = std::min(wg, 256u);                  // four-wide spectra: 42 hot dwords per path; three 256-path workgroups per CU (12 waves) beat one of 512 (8 waves) by 10 %
        // a workgroup of the regrouping kernels sits in ONE spiral block: blocks smaller than its path count get the largest
        // workgroup that divides them (16 x 16 -> 256 paths); only blocks below 256 pixels fall back to the per-lane kernel
        while (wg > 256 && (block_size * block_size) % wg != 0) wg /= 2;
        variant = (block_size * block_size) % wg != 0 ? kv::FLAT : kv::ring((int) wg);
    }
    if (spectral && variant == kv::FLAT && !path) variant = kv::NESTED;     // the spectral build's per-lane flat kernel is `path`'s
    // AOV channels (nbins / bins) and a sensor response function: `volpath` and (round 4) `volpathmis` carry them on the regrouping
    // machines (their NEW blocks) and `path` in its flat loop (kernels.hip: path_pixel_flat); a discrete response function with repeated
    // wavelengths keeps the volumetric integrators per lane
    if ((f.has_bins || f.has_srf) && !(variant == kv::FLAT && path) && !(kv::is_ring(variant) && !path && f.srf_lookup_by_wavelength)) variant = kv::NESTED;
    // Wavefront (gpu_*) streams carry their own PCG32 increment per (pixel, sample).  The regrouping machine of rgb / mono `volpath` keeps
    // only the generator's 64-bit state in LDS and recomputes the increment on every load (round 4: wg_block's WF instantiation, 1024-path
    // workgroups); everything else runs per lane, where the generator lives in registers: `volpath` as the flat state machine, the
    // others nested
    if (f.wavefront && kv::is_ring(variant) && !(variant == kv::ring(1024) && vol && !spectral)) variant = vol && !spectral ? kv::FLAT : kv::NESTED;
    auto serves = [&](const KernelRow &r) {
        auto admits = [](Tri t, bool v) { return t == ROW_EITHER || (t == ROW_YES) == v; };
        return r.variant == variant && r.integrator == f.integrator && r.spectral == spectral && admits(r.spectral_mis, f.use_spectral_mis) && admits(r.wavefront, f.wavefront);
    };
    for (size_t u = 0; u < KERNEL_UNIT_COUNT; ++u) {
        const UnitRecord &unit = KERNEL_UNITS[u];
        // MTSAMD_LEAN = 0: never a lean unit; 2: unit a is skipped (a scene that qualifies for it runs on b)
        if (unit.unit != UNIT_GENERAL && (sw.lean == 0 || (sw.lean == 2 && unit.unit == UNIT_A))) continue;
        if ((f.traits & unit.promises) != unit.promises) continue;
        for (size_t r = 0; r < KERNEL_ROW_COUNT; ++r)
            if (KERNEL_ROWS[r].unit == unit.unit && serves(KERNEL_ROWS[r])) return { variant, unit.unit };
    }
    throw std::runtime_error("no render kernel for variant " + std::to_string(variant) + " of integrator " + std::to_string(f.integrator));
}

uint32_t plan_block_size(int32_t block_size_) {
    // integrator.cpp:26-32,89-97: the reference's heuristic depends on the host thread count; this
    // backend pins MTS_BLOCK_SIZE = 32 when the scene leaves block_size at 0
    uint32_t block_size = block_size_ > 0 ? (uint32_t) block_size_ : 32u;
    { uint32_t q = 1; while (q < block_size) q <<= 1; block_size = q; }
    if (block_size > 1024) throw std::runtime_error("block_size too large");
    return block_size;
}

RenderPlan plan_render(const DSensor &se, int32_t samples_per_pass_, int32_t block_size_, int32_t film_channels, int shard_index, int shard_count,
                       int cus, const RenderSwitches &sw) {
    RenderPlan p;
    // integrator.cpp:58-65
    const size_t total_spp = (size_t) se.sample_count;
    const size_t samples_per_pass = samples_per_pass_ < 0 ? total_spp : std::min((size_t) samples_per_pass_, total_spp);
    if (samples_per_pass == 0 || (total_spp % samples_per_pass) != 0)
        throw std::runtime_error("sample_count (" + std::to_string(total_spp) + ") must be a multiple of samples_per_pass (" + std::to_string(samples_per_pass) + ").");
    p.n_passes = (total_spp + samples_per_pass - 1) / samples_per_pass;
    const uint32_t block_size = p.block_size = plan_block_size(block_size_);
    // spiral.cpp: enumerate every (pass, block) pair in the reference's order; keep this shard's blocks
    Spiral spiral; spiral.init(se.crop_w, se.crop_h, se.crop_x, se.crop_y, (int) block_size, p.n_passes);
    // Passes are independent jobs (each block id seeds its own streams), so the (pass, block) pairs of this shard are launched together,
    // MAX_BLOCKS_PER_LAUNCH at a time: the workspace (128 bytes per path in flight) stays below 1 GiB and thread indices far below 2^32.
    const size_t MAX_BLOCKS_PER_LAUNCH = std::max<size_t>(1, ((size_t) 8 << 20) / ((size_t) block_size * block_size));
    // Wavefront (gpu_*) streams: one stream per (pixel, sample), so a film with fewer pixels than the GPU has lanes is spread over
    // `split` entries per spiral block, each rendering sample_count / split samples of every pixel (DBlock::sample_base) into a slot of its own.
    p.split = 1;
    if (se.wavefront) {
        const size_t pixels = (size_t) se.crop_w * se.crop_h, target = (size_t) std::max(cus, 1) * 4096;      // four 1024-path workgroups' worth per CU
        if (sw.wavefront_split) p.split = sw.wavefront_split;
        else while (pixels * p.split < target && p.split * 2 <= total_spp && total_spp % (p.split * 2) == 0) p.split *= 2;
        if (total_spp % p.split != 0) throw std::runtime_error("MTSAMD_WAVEFRONT_SPLIT must divide the sample count");
    }
    p.launch_spp = samples_per_pass / p.split;                   // samples per pixel one entry of a launch renders
    p.film_floats = (size_t) se.crop_w * se.crop_h * (size_t) film_channels;     // X, Y, Z, A, W (+ two AOV channels per spectral bin)
    // The reference adds pass after pass to the film (integrator.cpp:98-107, imageblock.cpp:59-77): film = ((pass 1 + pass 2) + pass 3) + ...
    // Here the passes (and `split` entries) run concurrently, so each adds into a film-sized SLOT of its own (DBlock::film_off_*), summed in
    // order at the end (launch_film_sum_slots): the same additions in the same order, AOV channels included, the same film run after run.
    // Slots beyond 2 GiB are not allocated: the passes then meet in the one film in launch order.
    p.n_slots = p.n_passes * p.split;
    p.pass_slots = sw.pass_slots && p.n_slots > 1 && (uint64_t) p.n_slots * p.film_floats * sizeof(float) <= ((uint64_t) 2 << 30);
    p.chunks.resize(1);
    p.samples = 0;
    for (size_t pass = 0; pass < p.n_passes; ++pass)
        for (size_t k = 0; k < spiral.block_count; ++k) {
            DBlock b; size_t id;
            if (!spiral.next_block(b, id)) throw std::runtime_error("spiral exhausted early");
            if ((int) (id % (size_t) shard_count) != shard_index) continue;
            if (id >= ((uint64_t) 1 << 32)) throw std::runtime_error("block id overflow");
            b.id = (uint32_t) id; b.sample_base = 0;
            for (size_t sub = 0; sub < p.split; ++sub) {             // wavefront streams: `split` entries share a block's samples
                b.sample_base = (uint32_t) (sub * p.launch_spp);
                { const uint64_t off = p.pass_slots ? (uint64_t) (pass * p.split + sub) * p.film_floats : 0; b.film_off_lo = (uint32_t) off; b.film_off_hi = (uint32_t) (off >> 32); }
                if (p.chunks.back().size() >= MAX_BLOCKS_PER_LAUNCH) p.chunks.emplace_back();
                p.chunks.back().push_back(b);
            }
            p.samples += (uint64_t) b.sx * b.sy * samples_per_pass;
        }
    return p;
}

// ---- Workgroups of equal-cost pixels, expensive ones first.
// (a) A launch with more workgroups than the GPU holds runs them in rounds, in array order, and blocks differ in cost (the horizon of
//     an atmosphere costs a multiple of its zenith): in spiral order the launch waited for the expensive block that started last
//     (round 3: C4 278 -> 412 Msamples/s by starting expensive blocks first).
// (b) INSIDE a block the costs differ as well, and a path renders ONE pixel (the streams of scalar_rgb): the cheap pixels of a workgroup
//     finish early and its 16 waves then share a fraction of its paths (C4: waves idle 21 % of their time -- profiles/r04_ab_experiments.log).
// So the regrouping kernels first render a few samples per pixel, every path adding its finishing time to the cost of its TILE (16
// Morton-consecutive pixels: a 4 x 4 square; < 0.5 % of the job, the film is cleared again); the tiles of every launch are then sorted
// by descending cost and cut into workgroups of equal-cost pixels, the expensive ones first.  Which pixel receives which samples does
// not depend on where its path runs (streams are seeded by block id and Morton index): same film.
// Tiles pay on the kernels with few waves per CU -- the spectral variant and volpathmis (C5S +7 %, C5SM +47 %); the rgb volpath kernel
// (16 waves) keeps whole blocks (C4 -1.4 % with tiles).  MTSAMD_LPT: 0 none, 1 whole blocks by cost, 3 tiles by cost, 2 the default
// policy; 2 and 3 calibrate whatever the block count (tests, diagnostics with MTSAMD_LPT_DEBUG).
LptPolicy lpt_policy(int lpt, int variant, bool few_waves, const RenderPlan &plan, int cus, bool stop_requested) {
    const bool force = lpt == 2 || lpt == 3;
    uint32_t cal_spp = (uint32_t) std::max<size_t>(std::min<size_t>(4, plan.launch_spp / 128), force && plan.launch_spp >= 2 ? 1 : 0);
    if (!(kv::is_ring(variant) && plan.block_size <= 256 && lpt != 0 && (force || plan.chunks[0].size() > (size_t) std::max(cus, 1)) && !stop_requested)) cal_spp = 0;
    return { cal_spp, lpt == 3 || (lpt != 1 && few_waves) };
}

static uint64_t pos(const DBlock &b) { return ((uint64_t) (uint32_t) b.ox << 32) | (uint32_t) b.oy; }

// the distinct block positions of a chunk, sorted by position; the calibration samples land in the first slot
std::vector<DBlock> calibration_blocks(const std::vector<DBlock> &chunk) {
    std::vector<DBlock> cal(chunk);
    std::sort(cal.begin(), cal.end(), [](const DBlock &x, const DBlock &y) { return pos(x) < pos(y); });
    cal.erase(std::unique(cal.begin(), cal.end(), [](const DBlock &x, const DBlock &y) { return pos(x) == pos(y); }), cal.end());
    for (DBlock &c : cal) c.film_off_lo = c.film_off_hi = 0;
    return cal;
}

// A tile's measurement is 16 pixels x 1-4 samples of a heavy-tailed quantity: too noisy to sort by (a workgroup of tiles
// with "equal" measurements would still spread by tens of per cent).  The cost of a pixel varies smoothly over the film, so
// every tile takes the mean over the 7 x 7 tiles around it (28 x 28 pixels), on the film-wide grid of 4 x 4-pixel tiles.
CostIndex smooth_tile_costs(std::vector<uint64_t> &tile_cost, const std::vector<DBlock> &cal, uint32_t block_size, const DSensor &se) {
    const uint32_t tiles_per_block = block_size * block_size / 16u;
    CostIndex cost_index;
    for (size_t k = 0; k < cal.size(); ++k) cost_index.emplace_back(pos(cal[k]), (uint32_t) (k * tiles_per_block));
    const int gw = (se.crop_w + 3) / 4, gh = (se.crop_h + 3) / 4;
    std::vector<double> grid((size_t) gw * gh, -1.0);
    std::vector<uint32_t> where(tile_cost.size(), 0xFFFFFFFFu);      // tile slot -> grid cell
    for (size_t k = 0; k < cal.size(); ++k)
        for (uint32_t t = 0; t < tiles_per_block; ++t) {
            const auto o = tile_origin(t);
            if ((int) o.first >= cal[k].sx || (int) o.second >= cal[k].sy) continue;
            const int gx = (cal[k].ox - se.crop_x + (int) o.first) / 4, gy = (cal[k].oy - se.crop_y + (int) o.second) / 4;
            if (gx < 0 || gy < 0 || gx >= gw || gy >= gh) continue;
            grid[(size_t) gy * gw + gx] = (double) tile_cost[k * tiles_per_block + t];
            where[k * tiles_per_block + t] = (uint32_t) ((size_t) gy * gw + gx);
        }
    // summed-area table over the cells that hold a measurement
    std::vector<double> sat((size_t) (gw + 1) * (gh + 1), 0.0), cnt((size_t) (gw + 1) * (gh + 1), 0.0);
    for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
            const double v = grid[(size_t) y * gw + x];
            const size_t i = (size_t) (y + 1) * (gw + 1) + (x + 1);
            sat[i] = (v >= 0.0 ? v : 0.0) + sat[i - 1] + sat[i - (gw + 1)] - sat[i - (gw + 1) - 1];
            cnt[i] = (v >= 0.0 ? 1.0 : 0.0) + cnt[i - 1] + cnt[i - (gw + 1)] - cnt[i - (gw + 1) - 1];
        }
    const int R = 3;
    for (size_t sl = 0; sl < tile_cost.size(); ++sl) {
        if (where[sl] == 0xFFFFFFFFu) continue;
        const int x = (int) (where[sl] % (uint32_t) gw), y = (int) (where[sl] / (uint32_t) gw);
        const int x0 = std::max(0, x - R), x1 = std::min(gw, x + R + 1), y0 = std::max(0, y - R), y1 = std::min(gh, y + R + 1);
        auto box = [&](const std::vector<double> &a) { return a[(size_t) y1 * (gw + 1) + x1] - a[(size_t) y0 * (gw + 1) + x1] - a[(size_t) y1 * (gw + 1) + x0] + a[(size_t) y0 * (gw + 1) + x0]; };
        const double n = box(cnt);
        if (n > 0.0) tile_cost[sl] = (uint64_t) (box(sat) / n);
    }
    return cost_index;
}

// MTSAMD_LPT_DEBUG: the spread of the costs, between blocks and between the tiles of a block
void report_tile_costs(const std::vector<uint64_t> &tile_cost, size_t n_blocks, uint32_t tiles_per_block, uint32_t cal_spp) {
    double sum = 0.0, worst_ratio = 1.0; uint64_t lo = ~0ull, hi = 0;
    for (size_t k = 0; k < n_blocks; ++k) {
        uint64_t bsum = 0, tlo = ~0ull, thi = 0;
        for (uint32_t t = 0; t < tiles_per_block; ++t) { const uint64_t c = tile_cost[k * tiles_per_block + t]; bsum += c; if (c) { tlo = std::min(tlo, c); thi = std::max(thi, c); } }
        sum += (double) bsum; lo = std::min(lo, bsum); hi = std::max(hi, bsum);
        if (thi && tlo != ~0ull) worst_ratio = std::max(worst_ratio, (double) thi / (double) tlo);
    }
    size_t odd = 0;
    for (size_t k = 0; k < tile_cost.size(); ++k) if (tile_cost[k] >> 62) { if (odd < 8) fprintf(stderr, "[mtsamd] odd tile cost %llx at tile slot %zu\n", (unsigned long long) tile_cost[k], k); ++odd; }
    fprintf(stderr, "[mtsamd] %zu of %zu tile costs have their top bits set\n", odd, tile_cost.size());
    fprintf(stderr, "[mtsamd] tile costs over %zu blocks x %u tiles (%u spp): block sums min %.3g mean %.3g max %.3g, max / mean %.3f; largest max / min tile cost inside one block %.2f\n",
            n_blocks, tiles_per_block, cal_spp, (double) lo, sum / (double) n_blocks, (double) hi, (double) hi * (double) n_blocks / sum, worst_ratio);
}

// Every tile of the chunk that holds a pixel, by descending cost (ties: spiral order), cut into workgroups of `wg` paths: the tile
// table of the regrouping kernels (volpath_flat.h, WgArgs::tiles).  Otherwise -- or beyond the 20 bits of block index of a tile
// code -- the chunk is reordered in place, whole blocks by descending cost, and the table is empty.  Blocks not calibrated cost 0.
std::vector<uint32_t> schedule_chunk(std::vector<DBlock> &blocks, const CostIndex &cost_index, const std::vector<uint64_t> &tile_cost,
                                     uint32_t block_size, bool use_tiles, uint32_t wg) {
    const uint32_t tiles_per_block = block_size * block_size / 16u;
    std::vector<std::pair<uint64_t, uint32_t>> order;
    order.reserve(blocks.size() * tiles_per_block);
    std::vector<uint64_t> bsum(blocks.size(), 0);
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
        const DBlock &bk = blocks[bi];
        auto it = std::lower_bound(cost_index.begin(), cost_index.end(), std::make_pair(pos(bk), (uint32_t) 0));
        const bool known = it != cost_index.end() && it->first == pos(bk);
        for (uint32_t t = 0; t < tiles_per_block; ++t) {
            const auto o = tile_origin(t);
            if ((int) o.first >= bk.sx || (int) o.second >= bk.sy) continue;                  // a partial block at the image border
            const uint64_t c = known ? tile_cost[it->second + t] : 0ull;
            bsum[bi] += c;
            if (use_tiles) order.emplace_back(c, (uint32_t) ((bi << 12) | t));
        }
    }
    std::vector<uint32_t> tiles;
    if (use_tiles && blocks.size() < ((size_t) 1 << 20)) {
        std::stable_sort(order.begin(), order.end(), [](const auto &x, const auto &y) { return x.first > y.first; });
        const size_t wg_tiles = (size_t) wg / 16u;
        tiles.reserve((order.size() + wg_tiles - 1) / wg_tiles * wg_tiles);
        for (const auto &o : order) tiles.push_back(o.second);
        while (tiles.size() % wg_tiles) tiles.push_back(0xFFFFFFFFu);
    } else {
        std::vector<size_t> idx(blocks.size());
        for (size_t k = 0; k < idx.size(); ++k) idx[k] = k;
        std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return bsum[x] > bsum[y]; });
        std::vector<DBlock> sorted(blocks.size());
        for (size_t k = 0; k < idx.size(); ++k) sorted[k] = blocks[idx[k]];
        blocks.swap(sorted);
    }
    return tiles;
}

} // namespace mtsamd
