// render_plan_shim.cpp -- an extern "C" face of csrc/render_plan.cpp for tests/test_render_plan.py (built with g++ next to it; the
// product library exports none of this).  Every call returns 0, or -1 with the exception's message in `err`.  A DBlock crosses as
// eight 32-bit words.
#include <cstring>
#include <stdexcept>
#include "render_plan.h"

using namespace mtsamd;

#define SHIM_TRY try {
#define SHIM_CATCH } catch (const std::exception &e) { strncpy(err, e.what(), 511); err[511] = 0; return -1; } return 0;

extern "C" {

int rp_spiral(int sx, int sy, int ox, int oy, int bs, int passes, int max_blocks, int32_t *out /* 5 per block: ox, oy, sx, sy, id */) {
    Spiral sp; sp.init(sx, sy, ox, oy, bs, (size_t) passes);
    int n = 0; DBlock b; size_t id;
    for (; n < max_blocks && sp.next_block(b, id); ++n) { int32_t *o = out + 5 * n; o[0] = b.ox; o[1] = b.oy; o[2] = b.sx; o[3] = b.sy; o[4] = (int32_t) id; }
    return n;
}

// the switches of the environment: kernel, lean, lpt, lpt_debug, pass_slots, wavefront_split, inject_lost_path
int rp_switches(int64_t *out, char *err) {
    SHIM_TRY
    const RenderSwitches sw = read_render_switches();
    const int64_t v[7] = { sw.kernel, sw.lean, sw.lpt, sw.lpt_debug, sw.pass_slots, (int64_t) sw.wavefront_split, (int64_t) sw.inject_lost_path };
    memcpy(out, v, sizeof(v));
    SHIM_CATCH
}

// choose_kernel under the environment's switches for `n` scenes, nine facts each: integrator, spectral, use_spectral_mis, media, bins, srf,
// srf lookup by wavelength, wavefront, traits.  out: mts_stats.kernel_variant of each
int rp_choose_kernel(const int32_t *facts, int64_t n, uint32_t block_size, int32_t *out, char *err) {
    SHIM_TRY
    const RenderSwitches sw = read_render_switches();
    for (int64_t k = 0; k < n; ++k) {
        const int32_t *f = facts + 9 * k;
        const KernelChoice kc = choose_kernel({ f[0], f[1] != 0, f[2] != 0, f[3] != 0, f[4] != 0, f[5] != 0, f[6] != 0, f[7] != 0, f[8] }, block_size, sw);
        out[k] = kv::stat(kc.variant, kc.unit);
    }
    SHIM_CATCH
}

// the kernel table: six words per row (unit, variant, integrator, spectral MIS and wavefront streams as 0 no / 1 yes / 2 either, spectral
// build) and two per unit in order of preference (unit, promises); returns the number of rows, the number of units in *n_units
int rp_kernel_rows(int32_t *rows, int32_t *units, int32_t *n_units) {
    for (size_t r = 0; r < KERNEL_ROW_COUNT; ++r) {
        const KernelRow &k = KERNEL_ROWS[r];
        const int32_t v[6] = { k.unit, k.variant, k.integrator, k.spectral_mis, k.wavefront, k.spectral };
        memcpy(rows + 6 * r, v, sizeof(v));
    }
    for (size_t u = 0; u < KERNEL_UNIT_COUNT; ++u) { units[2 * u] = KERNEL_UNITS[u].unit; units[2 * u + 1] = KERNEL_UNITS[u].promises; }
    *n_units = (int32_t) KERNEL_UNIT_COUNT;
    return (int) KERNEL_ROW_COUNT;
}

// plan_render under the environment's switches.  head: block_size, n_passes, split, launch_spp, film_floats, n_slots, pass_slots, samples,
// number of chunks, number of entries; up to `cap` entries go to `blocks` and the size of each chunk (up to `cap`) to `chunk_sizes`.
int rp_plan(const int32_t *crop /* x, y, w, h */, int32_t sample_count, int32_t wavefront, int32_t samples_per_pass, int32_t block_size,
            int32_t film_channels, int shard_index, int shard_count, int cus, int64_t cap, int64_t *head, uint32_t *blocks, int64_t *chunk_sizes, char *err) {
    SHIM_TRY
    DSensor se; memset(&se, 0, sizeof(se));
    se.crop_x = crop[0]; se.crop_y = crop[1]; se.crop_w = crop[2]; se.crop_h = crop[3]; se.sample_count = sample_count; se.wavefront = wavefront;
    const RenderPlan p = plan_render(se, samples_per_pass, block_size, film_channels, shard_index, shard_count, cus, read_render_switches());
    int64_t n = 0;
    for (size_t c = 0; c < p.chunks.size(); ++c) {
        if ((int64_t) c < cap) chunk_sizes[c] = (int64_t) p.chunks[c].size();
        for (const DBlock &b : p.chunks[c]) { if (n < cap) memcpy(blocks + 8 * n, &b, sizeof(DBlock)); ++n; }
    }
    const int64_t h[10] = { p.block_size, (int64_t) p.n_passes, (int64_t) p.split, (int64_t) p.launch_spp, (int64_t) p.film_floats, (int64_t) p.n_slots,
                            p.pass_slots, (int64_t) p.samples, (int64_t) p.chunks.size(), n };
    memcpy(head, h, sizeof(h));
    SHIM_CATCH
}

// lpt_policy for a plan reduced to what it reads: out = cal_spp, use_tiles
int rp_lpt_policy(int lpt, int variant, int few_waves, uint32_t block_size, int64_t launch_spp, int64_t chunk0_blocks, int cus, int stop, int64_t *out, char *err) {
    SHIM_TRY
    RenderPlan p{}; p.block_size = block_size; p.launch_spp = (size_t) launch_spp; p.chunks.resize(1); p.chunks[0].resize((size_t) chunk0_blocks);
    const LptPolicy l = lpt_policy(lpt, variant, few_waves != 0, p, cus, stop != 0);
    out[0] = l.cal_spp; out[1] = l.use_tiles;
    SHIM_CATCH
}

// calibration_blocks: `n` blocks in, the count out (`out` holds n)
int rp_calibration_blocks(const uint32_t *blocks, int64_t n, uint32_t *out, int64_t *n_out, char *err) {
    SHIM_TRY
    std::vector<DBlock> chunk((size_t) n);
    memcpy(chunk.data(), blocks, (size_t) n * sizeof(DBlock));
    const std::vector<DBlock> cal = calibration_blocks(chunk);
    memcpy(out, cal.data(), cal.size() * sizeof(DBlock)); *n_out = (int64_t) cal.size();
    SHIM_CATCH
}

// smooth_tile_costs in place on `cost` (n_cal * block_size^2 / 16 slots); the cost index: n_cal (position, first slot) pairs
int rp_smooth(uint64_t *cost, const uint32_t *cal, int64_t n_cal, uint32_t block_size, const int32_t *crop, uint64_t *index_pos, uint32_t *index_slot,
              int debug_report, uint32_t cal_spp, char *err) {
    SHIM_TRY
    const size_t n_cost = (size_t) n_cal * (block_size * block_size / 16u);
    std::vector<uint64_t> tc(cost, cost + n_cost);
    std::vector<DBlock> cb((size_t) n_cal);
    memcpy(cb.data(), cal, cb.size() * sizeof(DBlock));
    DSensor se; memset(&se, 0, sizeof(se));
    se.crop_x = crop[0]; se.crop_y = crop[1]; se.crop_w = crop[2]; se.crop_h = crop[3];
    const CostIndex ci = smooth_tile_costs(tc, cb, block_size, se);
    if (debug_report) report_tile_costs(tc, cb.size(), block_size * block_size / 16u, cal_spp);
    memcpy(cost, tc.data(), n_cost * sizeof(uint64_t));
    for (size_t k = 0; k < ci.size(); ++k) { index_pos[k] = ci[k].first; index_slot[k] = ci[k].second; }
    SHIM_CATCH
}

// schedule_chunk: `blocks` (n) are reordered in place; the tile table (up to `cap` entries) goes to `tiles`, its length to n_tiles
int rp_schedule(uint32_t *blocks, int64_t n, const uint64_t *index_pos, const uint32_t *index_slot, int64_t n_index, const uint64_t *cost, int64_t n_cost,
                uint32_t block_size, int use_tiles, uint32_t wg, int64_t cap, uint32_t *tiles, int64_t *n_tiles, char *err) {
    SHIM_TRY
    std::vector<DBlock> chunk((size_t) n);
    memcpy(chunk.data(), blocks, (size_t) n * sizeof(DBlock));
    CostIndex ci;
    for (int64_t k = 0; k < n_index; ++k) ci.emplace_back(index_pos[k], index_slot[k]);
    const std::vector<uint64_t> tc(cost, cost + n_cost);
    const std::vector<uint32_t> t = schedule_chunk(chunk, ci, tc, block_size, use_tiles != 0, wg);
    memcpy(blocks, chunk.data(), (size_t) n * sizeof(DBlock));
    *n_tiles = (int64_t) t.size();
    if ((int64_t) t.size() <= cap) memcpy(tiles, t.data(), t.size() * sizeof(uint32_t));
    SHIM_CATCH
}

} // extern "C"
