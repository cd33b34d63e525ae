// render_plan.h -- the host arithmetic of mts_render (capi.cpp), apart from the device so that the CPU test-suite can pin it
// (tests/test_render_plan.py): the render switches, the kernel table and the choice of a scene's render kernel, the passes and blocks
// of a shard, and the cost-sorted schedule of each launch.
// Plain C++17: dscene.h, the C ABI's enums and the standard library only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>
#include "dscene.h"
#include "kernel_names.h"                               // kv (nested, flat, ring(P), stat()) and enum KernelUnit
#include "../../include/mtsamd.h"

namespace mtsamd {

// librender/spiral.cpp:11-72
struct Spiral {
    int size_x, size_y, off_x, off_y, block_size, blocks_x, blocks_y;
    size_t block_count, block_counter, remaining_passes;
    int dir, pos_x, pos_y, steps_left, steps;
    void init(int sx, int sy, int ox, int oy, int bs, size_t passes) {
        size_x = sx; size_y = sy; off_x = ox; off_y = oy; block_size = bs; remaining_passes = passes;
        blocks_x = (int) std::ceil((float) sx / bs); blocks_y = (int) std::ceil((float) sy / bs);
        block_count = (size_t) blocks_x * blocks_y;
        reset();
    }
    void reset() { block_counter = 0; dir = 0; pos_x = blocks_x / 2; pos_y = blocks_y / 2; steps_left = 1; steps = 1; }
    bool next_block(DBlock &b, size_t &block_id) {
        if (block_count == block_counter) {
            if (remaining_passes > 1) { --remaining_passes; reset(); }
            else return false;
        }
        block_id = block_counter + (remaining_passes - 1) * block_count;
        int offx = pos_x * block_size, offy = pos_y * block_size;
        b.sx = std::min(block_size, size_x - offx); b.sy = std::min(block_size, size_y - offy);
        b.ox = offx + off_x; b.oy = offy + off_y; b.film_off_lo = b.film_off_hi = 0;
        ++block_counter;
        if (block_counter != block_count) {
            do {
                switch (dir) { case 0: ++pos_x; break; case 1: ++pos_y; break; case 2: --pos_x; break; case 3: --pos_y; break; }
                if (--steps_left == 0) { dir = (dir + 1) % 4; if (dir == 2 || dir == 0) ++steps; steps_left = steps; }
            } while (pos_x < 0 || pos_y < 0 || pos_x >= blocks_x || pos_y >= blocks_y);
        }
        return true;
    }
};

// The switches of a render, read once, before anything else happens; a value outside the accepted ones is an error.
struct RenderSwitches {
    int kernel = -1;                  // MTSAMD_KERNEL: -1 unset, else the variant it names (nested, flat, wga256 = ring(256), wga1024 = ring(1024))
    int lean = 1;                     // MTSAMD_LEAN: 0 never a lean unit, 1 the leanest unit a scene qualifies for, 2 unit b where a would do
    int lpt = -1;                     // MTSAMD_LPT: -1 unset, 0 spiral order, 1 whole blocks by cost, 2 the default forced, 3 tiles by cost (lpt_policy)
    bool lpt_debug = false;           // MTSAMD_LPT_DEBUG: set
    bool pass_slots = true;           // MTSAMD_PASS_SLOTS=0: the passes meet in the one film
    size_t wavefront_split = 0;       // MTSAMD_WAVEFRONT_SPLIT; 0: chosen to fill the GPU
    uint64_t inject_lost_path = 0;    // MTSAMD_TEST_INJECT_LOST_PATH: idle bound in ticks
};
RenderSwitches read_render_switches();

// ---- The kernel table: every render kernel choose_kernel can select, as the launchers of kernels.hip carry them (which keep the thread
// counts and the instantiations).  A row serves a scene of its integrator and build whose spectral MIS and random streams it admits.
enum Tri : int { ROW_NO = 0, ROW_YES = 1, ROW_EITHER = 2 };
struct KernelRow {
    KernelUnit unit; int variant; int integrator;       // MTS_INTEGRATOR_*
    Tri spectral_mis;                                   // mts_integrator.use_spectral_mis (volpathmis)
    Tri wavefront;                                      // the wavefront (gpu_*) streams: one generator per (pixel, sample)
    bool spectral;                                      // the spectral build (MTS_SPEC_N = 4) or the rgb / mono one
};
// A unit and what a scene must keep of dscene.h's MT_* promises to run on it; KERNEL_UNITS lists them in order of preference.
struct UnitRecord { KernelUnit unit; int promises; };
extern const KernelRow KERNEL_ROWS[];
extern const UnitRecord KERNEL_UNITS[];
extern const size_t KERNEL_ROW_COUNT, KERNEL_UNIT_COUNT;

// What the choice reads of a scene (capi.cpp: facts_of)
struct KernelFacts {
    int integrator;                                     // MTS_INTEGRATOR_*
    bool spectral, use_spectral_mis, has_media, has_bins /* bin_count > 0 */, has_srf /* srf >= 0 */, srf_lookup_by_wavelength, wavefront;
    int traits;                                         // MT_* (scene_host.cpp: scene_traits)
};
struct KernelChoice { int variant; KernelUnit unit; };
KernelChoice choose_kernel(const KernelFacts &f, uint32_t block_size, const RenderSwitches &sw);

// Passes, blocks and film slots of one shard of a render (integrator.cpp:58-97; the comments of render_plan.cpp say why).
struct RenderPlan {
    uint32_t block_size;                        // a power of two
    size_t n_passes, split, launch_spp, film_floats, n_slots;
    bool pass_slots;
    std::vector<std::vector<DBlock>> chunks;    // this shard's (pass, block) entries in spiral order, cut into launches
    uint64_t samples;
};
uint32_t plan_block_size(int32_t block_size);          // the block size of a render: the scene's, or the default, as a power of two
RenderPlan plan_render(const DSensor &se, int32_t samples_per_pass, int32_t block_size, int32_t film_channels, int shard_index, int shard_count,
                       int cus, const RenderSwitches &sw);

// The first pixel of tile t of a block: Morton index 16 t -> (x, y) by de-interleaving the bits (the other fifteen lie right of / below it).
inline std::pair<uint32_t, uint32_t> tile_origin(uint32_t t) {
    uint32_t x0 = 0, y0 = 0;
    for (uint32_t bit = 0; bit < 16; ++bit) { x0 |= (((16u * t) >> (2 * bit)) & 1u) << bit; y0 |= (((16u * t) >> (2 * bit + 1)) & 1u) << bit; }
    return { x0, y0 };
}

// The cost-sorted schedule: samples per pixel of the calibration launch (0: none, spiral order) and tiles or whole blocks.
struct LptPolicy { uint32_t cal_spp; bool use_tiles; };
LptPolicy lpt_policy(int lpt, int variant, bool few_waves, const RenderPlan &plan, int cus, bool stop_requested);
std::vector<DBlock> calibration_blocks(const std::vector<DBlock> &chunk);
// (block position, index of its first tile in the tile costs), sorted by position
typedef std::vector<std::pair<uint64_t, uint32_t>> CostIndex;
CostIndex smooth_tile_costs(std::vector<uint64_t> &tile_cost, const std::vector<DBlock> &cal, uint32_t block_size, const DSensor &se);
void report_tile_costs(const std::vector<uint64_t> &tile_cost, size_t n_blocks, uint32_t tiles_per_block, uint32_t cal_spp);
std::vector<uint32_t> schedule_chunk(std::vector<DBlock> &blocks, const CostIndex &cost_index, const std::vector<uint64_t> &tile_cost,
                                     uint32_t block_size, bool use_tiles, uint32_t wg);

} // namespace mtsamd
