// ring_driver.h -- the asynchronous-regrouping driver: a workgroup's paths wait in LDS rings, one per block class, and its waves serve them.
//
// Written once for every state machine that cuts its work into the block classes B_INT .. B_CROSS of volpath_flat.h: `volpath`
// (VolpathRing, volpath_flat.h) and `volpathmis` (VolpathMisRing, volpathmis_flat.h).  A machine comes in as a policy M -- types,
// constants and static functions, nothing stored:
//   M::COUNT                  the counting kernel variant (loop counters, block statistics, the lost-path test hook)
//   M::State, M::Hot          a path's state in registers, and its struct-of-arrays store in LDS (hs.base, hs.store(p, cls))
//   M::HOT_DWORDS, M::PACKED  hot dwords per path; the one whose low four bits hold the path's S_* state (wg_flush_unfinished)
//   M::Machine                vm(sc, cnt) with begin_sample, top and classify
//   M::init_idle(p)           the fields of a path that owns no pixel, beyond the ray and the hit the driver sets
//   M::block<C>               the block function of class C (wg_block, mis_block), as a constant: block<C>(kernarg, hot_lds, wg_base,
//                             pid, &cnt) is one visit of path `pid` and returns the class it waits for next
//   M::check_shape<NT>()      static_assert on the threads that serve the policy's WG paths
//   M::OPAQUE_INIT            the init loop loads the kernel arguments inside its body (see there)
//   M::CROSS                  the machine names the class B_CROSS: nine rings; otherwise eight, and the class has neither slots nor a block
#pragma once
#include "volpath_flat.h"

namespace mtsamd {
inline namespace MTS_VARIANT_NS {

// No workgroup barriers and no sort: one LDS ring of path ids per block class.  A wave claims up to 64 ids from the fullest ring
// (compare-and-swap on its head), runs that block with every claimed lane active, and appends each path to
// the ring of the class it waits for next (one LDS atomic add on the tail per lane; the value returned is the slot).  Waves never wait for
// each other; a wave that finds every ring empty naps briefly.
//
// Ring protocol.  q_ctl[2c] / q_ctl[2c + 1] are head / tail of ring c: two 32-bit counters that only ever grow (slot = counter mod
// WG), each touched with 32-bit atomics only; "ring" B_DONE has no slots, its tail counts the finished paths; q_ctl[2 B_COUNT] is the
// workgroup's stop word.  The slots are 16 bit wide and touched with 16-bit loads / stores only; a slot holds (lap, id), lap = the
// ring index's lap number modulo 2^(16 - log2 WG) (RingSlot below; round 3 -- rounds 1 and 2 marked a slot empty / full instead):
//   producer: release fence (state in LDS / HBM is written), tail++ -> index, store (lap of index, id): no look at the slot, no wait;
//   consumer: head: h -> h + n by compare-and-swap (n <= tail - h of a snapshot: those indices are already handed out), the n slots
//             read together with it; a slot is accepted when it carries the lap of its index, acquire fence.  Nothing is written back.
// A consumer can be ahead of its producer (index handed out, id not stored yet): the slot then still carries the previous lap, and
// the lane waits in a wave-uniform loop (a divergent `while` would park the ready lanes behind the reconvergence point).  The wait is
// BOUNDED: after MTS_RING_SPIN_LIMIT polls it writes a diagnostic record (ring, index, head, tail) and stops the workgroup --
// mts_render reports an error instead of hanging.  A slot is overwritten one lap (WG pushes through this ring) after it was written,
// while its consumer reads it within a few instructions of its claim; a lane that ever sat between claim and read for a whole lap
// would find a newer lap, run into that bound and fail the render loudly.  A path that never comes back for any other reason leaves
// the finished count short: the idle wait is bounded too -- by ELAPSED TIME (round 4; a nap count measured the wave's own speed, and
// a debugger, a profiler or a throttled clock stretches another wave's long block visit but not the naps): MTS_IDLE_TICKS of the
// constant 100 MHz clock (s_memrealtime) in a row with every ring empty -> diagnostic code 3.
// Stopping (Integrator::cancel / timeout, or a stall) adds no exit to the claim loop (a second exit measured 4.5 % slower): the
// first lane to raise the stop word adds 2^31 to every head, which makes every ring look empty to every wave (a count above WG is no
// count, see the snapshot) and every pending claim fail; a wave that finds every ring empty looks at the stop word before it naps.
#define MTS_RING_SPIN_LIMIT (1u << 22)
#define MTS_IDLE_TICKS 1000000000u     // ten seconds of the 100 MHz constant clock with nothing waiting anywhere before a wave reports a lost path (never seen)
#define MTS_COST_FLAG 15           // counters[15] != 0: a calibration launch; counters[MTS_COST_BASE + slot]: summed finish times of the paths of tile `slot`
#define MTS_COST_BASE 16
#define MTS_INJECT_SLOT 14         // counters[14] != 0 (set by mts_render from MTSAMD_TEST_INJECT_LOST_PATH, counting kernel variants only):
                                   // the first wave of workgroup 0 drops one hand-over, and the idle bound is that many ticks -- the
                                   // test of the error path (tests/test_gpu_parity.py::test_lost_path_is_reported)
#define MTS_CROSS_SLOT 3           // counters[3] (counting kernel variants): lane-visits of the class B_CROSS -- mts_debug_cross_visits, tests/test_gpu_cross_class.py
#define MTS_DIAG_BASE 4            // counters[MTS_DIAG_BASE + 0..5]: code (1 consumer / 2 producer), ring, index, head, tail, workgroup
enum : uint32_t { STOP_NONE = 0, STOP_CANCEL = 1, STOP_STALL = 2 };

// One nap of an idle wave: true once the rings have looked empty for `limit` ticks in a row.  The clock is read on the first nap of
// an idle period and on every 1024th after it (32-bit differences: the checks are ~1 ms apart, the counter wraps after 43 s).
DEV bool wga_idle_expired(uint32_t &idle_naps, uint32_t &idle_t0, uint32_t limit) {
    if (idle_naps++ == 0u) { idle_t0 = (uint32_t) __builtin_amdgcn_s_memrealtime(); return false; }
    if ((idle_naps & 1023u) != 0u) return false;
    return (uint32_t) __builtin_amdgcn_s_memrealtime() - idle_t0 > limit;
}

template <int WG>
DEV bool wga_raise_stop(uint32_t *q_ctl, uint32_t why) {
    if (atomicCAS(&q_ctl[2 * B_COUNT], (uint32_t) STOP_NONE, why) != STOP_NONE) return false;          // already stopping
#pragma unroll 1
    for (int c = 0; c < B_DONE; ++c) atomicAdd(&q_ctl[2 * c], 0x80000000u);
    return true;
}
template <int WG>
DEV void wga_stall(uint32_t code, int ring, uint32_t index, uint32_t *q_ctl, unsigned long long *counters) {
    const uint32_t hd = __atomic_load_n(&q_ctl[2 * ring], __ATOMIC_RELAXED), tl = __atomic_load_n(&q_ctl[2 * ring + 1], __ATOMIC_RELAXED);
    if (wga_raise_stop<WG>(q_ctl, STOP_STALL)) {                                                       // first lane of the workgroup to give up
        if (atomicCAS(counters + MTS_DIAG_BASE, 0ull, (unsigned long long) code) == 0ull) {            // first workgroup of the launch
            counters[MTS_DIAG_BASE + 1] = (unsigned long long) ring; counters[MTS_DIAG_BASE + 2] = index;
            counters[MTS_DIAG_BASE + 3] = hd; counters[MTS_DIAG_BASE + 4] = tl; counters[MTS_DIAG_BASE + 5] = blockIdx.x;
        }
    }
}
// Tagged slots: (lap << log2(WG)) | id.  Against the empty / full marking of rounds 1 and 2 (load, store on both sides, and a producer
// that waits for the previous lap's consumer) this is two dependent LDS round trips less per block visit; measured C3 +-0, C4 +2 %
// (profiles/r03_ab_experiments.log).
template <int WG> struct RingSlot {
    static constexpr uint32_t IDBITS = WG == 1024 ? 10 : WG == 512 ? 9 : WG == 256 ? 8 : WG == 128 ? 7 : 6;
    static_assert((1u << IDBITS) == (uint32_t) WG, "paths per workgroup: 64 .. 1024, a power of two");
    static constexpr uint32_t TAGMASK = (1u << (16 - IDBITS)) - 1u;
    DEV static uint32_t tag_of(uint32_t index) { return (index >> IDBITS) & TAGMASK; }
    DEV static uint32_t make(uint32_t index, uint32_t pid) { return (tag_of(index) << IDBITS) | pid; }
    DEV static bool matches(uint32_t v, uint32_t index) { return (v >> IDBITS) == tag_of(index); }
    DEV static uint32_t id(uint32_t v) { return v & (uint32_t) (WG - 1); }
};
// a lane ahead of its producer: wait (wave-uniform loop, bounded) until the slot carries the lane's lap
template <int WG>
DEV uint32_t wga_tag_wait(bool pending, uint16_t *slot, uint32_t *q_ctl, unsigned long long *counters, int ring, uint32_t index) {
    uint32_t out = 0xFFFFu;
#pragma nounroll
    for (uint32_t spins = 0;; ++spins) {
        if (pending) {
            const uint32_t v = __atomic_load_n(slot, __ATOMIC_RELAXED);
            if (RingSlot<WG>::matches(v, index)) { out = RingSlot<WG>::id(v); pending = false; }
        }
        if (!__builtin_amdgcn_ballot_w64(pending)) break;
        if (spins > MTS_RING_SPIN_LIMIT) { if (pending) wga_stall<WG>(1u, ring, index, q_ctl, counters); break; }
        if (__atomic_load_n(&q_ctl[2 * B_COUNT], __ATOMIC_RELAXED) != STOP_NONE) break;
    }
    return out;
}

template <int WG>
DEV void wga_push(int cls, uint32_t pid, bool valid, uint16_t (*q_ids)[WG], uint32_t *q_ctl) {
    // One LDS atomic per lane: the tail value it returns IS the lane's ring index; the LDS unit serialises the lanes that share a ring.
    // (Ranking the lanes first -- nine ballots, per-class counts, one atomic per class -- took 45 to 100 VALU instructions per push
    // and measured 1 to 3 % slower; the order of the ids inside a ring is immaterial.)
    uint32_t ti = 0;
    if (valid) ti = atomicAdd(&q_ctl[2 * cls + 1], 1u);
    if (valid && cls != B_DONE) __atomic_store_n(&q_ids[cls][ti & (uint32_t) (WG - 1)], (uint16_t) RingSlot<WG>::make(ti, pid), __ATOMIC_RELAXED);
}

// A stopped workgroup (Integrator::cancel(), the integrator's timeout, a stall) adds the accumulators of its unfinished pixels to the
// film: the reference puts a partially rendered block on the film as well (integrator.cpp:120-130: render_block returns early on
// should_stop(), film->put(block) follows; :213-216).  The sample in flight is dropped, W counts the finished ones.  Runs behind a
// workgroup barrier, when no wave touches the path state any more; `packed_at` = the hot dword that holds a path's state (S_DONE:
// already on the film).
template <int WG, int NT, bool MOMENT = false>
DEV void wg_flush_unfinished(const MTS_CONST_AS void *kernarg, const uint32_t *hot_lds, int packed_at, uint32_t wg_base) {
    const WgArgs a = cload_k<WgArgs>(kernarg);
#pragma unroll 1
    for (uint32_t pid = threadIdx.x; pid < (uint32_t) WG; pid += NT) {
        if ((hot_lds[packed_at * WG + pid] & 15u) == S_DONE) continue;
        PathEnvT<ColdStoreHbm> e;
        if (!wg_env<WG>(a, wg_base, pid, e)) continue;
        float *own = film_entry_of<MOMENT>(a.sc, e.blk, e.lx, e.ly, e.film);       // a `moment` machine's AOV channels are on the film already
        for (int k = 0; k < 5; ++k) atomicAdd(own + k, e.cold.f(C_ACC + k));
    }
}

// The driver: M::WG paths served by NT threads (fewer threads than paths keeps the rings fuller).  Every instantiation, that is every
// kernel, owns its three LDS arrays.
template <class M, int NT>
DEV void ring_workgroup_async(const MTS_CONST_AS void *kernarg, Counters &cnt) {
    constexpr bool COUNT = M::COUNT;
    constexpr int WG = M::WG, NQ = M::CROSS ? B_DONE : B_CROSS;      // B_CROSS is the last class: a machine without it keeps the rings before it
    static_assert((WG & (WG - 1)) == 0 && WG <= 32768, "ring indices wrap with a mask and ids are 16 bit");
    static_assert(NT % 64 == 0 && WG % 64 == 0, "whole waves");
    M::template check_shape<NT>();
    __shared__ uint32_t hot_lds[M::HOT_DWORDS * WG];
    __shared__ uint16_t q_ids[NQ][WG];
    __shared__ __attribute__((aligned(8))) uint32_t q_ctl[2 * B_COUNT + 2];      // head / tail pairs, then the stop word
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wg_base = blockIdx.x * WG;
#pragma unroll 1
    for (int c = 0; c < NQ; ++c) {
#pragma unroll 1
        for (uint32_t i = tid; i < (uint32_t) WG; i += NT) q_ids[c][i] = 0xFFFFu;      // runs once: not worth 300 unrolled instructions
    }
    if (tid < 2u * B_COUNT + 2u) q_ctl[tid] = 0;
    pm_tables_to_lds(tid);
    // the kernel's LDS: the three arrays above, the two pmath tables (512 B) and, for a machine that has one, the geometry table
    static_assert(sizeof(hot_lds) + sizeof(q_ids) + sizeof(q_ctl) + 512 + (M::GEOM_TABLE ? MTS_GEOM_LDS_BYTES : 0) <= 160 * 1024, "a workgroup has 160 KiB of LDS");
    if constexpr (M::GEOM_TABLE) geom_table_to_lds(cload_k<WgArgs>(kernarg).sc, tid, (uint32_t) NT);      // read-only behind the barrier
    __syncthreads();
#pragma unroll 1
    for (uint32_t pid0 = tid; pid0 < (uint32_t) WG; pid0 += NT) {   // ---- initialise the paths (integrator.cpp:198) and queue them
        // M::OPAQUE_INIT: the loop reads the arguments through an opaque copy of their pointer, as a block does, so that the scene's scalars
        // are loaded where begin_sample reads them and not ahead of the loop.  Register allocation only -- the flagship kernel spills 177
        // SGPRs at its head without it and 153 with it -- but it moves whole kernels by up to a per cent either way, so the units choose
        // (unit_config.h: MTS_OPAQUE_INIT, with MTS_HOT_DRCP).
        uint32_t wg_base_u = 0;
        const MTS_CONST_AS void *ka = kernarg;
        if constexpr (M::OPAQUE_INIT) ka = block_uniforms(kernarg, wg_base, wg_base_u);
        const WgArgs a = cload_k<WgArgs>(ka);
        typename M::Machine vm(a.sc, cnt);
        PathEnvT<ColdStoreHbm> e; typename M::State p;
        typename M::Hot hs; hs.base = hot_lds + pid0;
        const bool ok = wg_env<WG>(a, wg_base, pid0, e);
        p.rng.state = 0; p.rng.inc = 0;
        p.ray = make_ray(f3s(0.f), f3(0.f, 0.f, 1.f), 0.f, 0.f); p.si.t = pm_inf(); p.si.p = f3s(0.f); p.si.uv.x = p.si.uv.y = 0.f; p.si.shape = -1; p.si.prim = 0;
        M::init_idle(p);
        p.st = S_DONE;
        if (ok) {
            const uint32_t ppb = a.block_size * a.block_size;
            p.rng.seed(a.sc.sensor.seed + (uint64_t) e.blk.id * ppb + e.index, PCG32_DEFAULT_STREAM);     // sampler.cpp:83-96
            for (int k = 0; k < 5; ++k) e.cold.f(C_ACC + k) = 0.f;
            e.cold.f(C_SAMPLE) = __uint_as_float(0u);
            vm.begin_sample(p, e);
            vm.top(p, e);
        }
        const int cls = vm.classify(p);
        hs.store(p, cls);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        wga_push<WG>(cls, pid0, true, q_ids, q_ctl);
    }
#if defined(MTSAMD_BLOCKSTATS)
    long long bs_t0 = clock64(); unsigned long long bs_loc[48] = {};                      // laid out like g_blockstats
#endif
    uint32_t poll_ticks = (tid >> 6) * 2048u, idle_naps = 0, idle_t0 = 0; // per wave, staggered: paces the polls of the host's stop word
    uint32_t idle_limit = MTS_IDLE_TICKS; bool drop_one = false;
    if (COUNT) {                                              // error-path test hook (MTS_INJECT_SLOT): never in the production instantiation
        const uint32_t inj = (uint32_t) __builtin_amdgcn_readfirstlane((int) (uint32_t) cload_k<WgArgs>(kernarg).counters[MTS_INJECT_SLOT]);
        if (inj != 0u) { idle_limit = inj; drop_one = blockIdx.x == 0u && tid < 64u; }
    }
    // calibration launch of mts_render (counters[MTS_COST_FLAG] != 0): every path adds the time at which it finished its pixel to its tile's cost
    const bool record_cost = __builtin_amdgcn_readfirstlane((int) (uint32_t) cload_k<WgArgs>(kernarg).counters[MTS_COST_FLAG]) != 0;
    const long long cost_t0 = record_cost ? clock64() : 0ll;
#pragma unroll 1
    for (;;) {
      uint32_t n = 0, h = 0, spec_slot = 0xFFFFu; int sel = 0; bool finished = false;
      // ---- the claim: an inner loop of its own (snapshot, vote, compare-and-swap), left with a claim or when the workgroup is done.
      // (As `continue`s of the outer loop the retries dragged eighteen register copies of dead path state through every round.)
#pragma unroll 1
      for (;;) {
        // ---- snapshot of the rings, pick the fullest
        uint32_t hd = 0, avail = 0;
        if (lane < (uint32_t) B_COUNT) {
            hd = __atomic_load_n(&q_ctl[2 * lane], __ATOMIC_RELAXED);
            const uint32_t tl = __atomic_load_n(&q_ctl[2 * lane + 1], __ATOMIC_RELAXED);
            // the two loads are not one atomic snapshot: a head newer than the tail gives a "negative" count, which is no count at all
            // (so does a stopped ring, wga_raise_stop).  Any tail that was ever read is a lower bound of the tail now, so tl - hd
            // entries exist whenever the claim finds head == hd.
            avail = tl - hd;
            if (avail > (uint32_t) WG) avail = 0;
        }
        // argmax over the NQ rings in three DPP steps: lanes 0..7 hold (avail << 4 | 15 - ring), the maximum of a row's first eight
        // lanes ends up in lane 7 (ties go to the lower ring, as a first-maximum scan would have it); one readlane instead of eight
        // and no scalar compare chain.  Nine rings: a fourth step, and the maximum of the row's sixteen lanes is in lane 15.
        uint32_t key = lane < (uint32_t) NQ ? ((avail << 4) | (15u - lane)) : 0u;
        key = max(key, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) key, 0x111 /* row_shr:1 */, 0xf, 0xf, true));
        key = max(key, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) key, 0x112 /* row_shr:2 */, 0xf, 0xf, true));
        key = max(key, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) key, 0x114 /* row_shr:4 */, 0xf, 0xf, true));
        if constexpr (NQ > 8) key = max(key, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) key, 0x118 /* row_shr:8 */, 0xf, 0xf, true));
        const uint32_t top_key = (uint32_t) __builtin_amdgcn_readlane((int) key, NQ > 8 ? 15 : 7);
        const uint32_t best = top_key >> 4; sel = 15 - (int) (top_key & 15u);
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) {      // population at snapshot time: finished paths [45], paths waiting in the rings [46], snapshots [47]
            uint32_t waiting = 0;
            for (int c = 0; c < NQ; ++c) waiting += (uint32_t) __builtin_amdgcn_readlane((int) avail, c);
            bs_loc[45] += (uint32_t) __builtin_amdgcn_readlane((int) avail, B_DONE); bs_loc[46] += waiting; bs_loc[47] += 1ull;
        }
#endif
        if (best == 0) {
            // every path of the workgroup has finished, or the workgroup was stopped (then every ring looks empty for good)
            if ((uint32_t) __builtin_amdgcn_readlane((int) avail, B_DONE) == (uint32_t) WG || __atomic_load_n(&q_ctl[2 * B_COUNT], __ATOMIC_RELAXED) != STOP_NONE) { finished = true; break; }
            // Integrator::should_stop() (integrator.h:143-146): waves look at the host's stop word (pinned host memory) now and then.  Reads
            // of host memory are a scarce resource -- the whole GPU sustains about 3 * 10^7 per second, and a poll on every nap made the
            // render 4.7 times longer -- so a wave earns a poll with 32768 ticks: one per nap, 256 per execution of the NEW block (below).
            // That is about 10^5 polls per second over all workgroups, and a few milliseconds until a workgroup notices.
            if ((poll_ticks += 1u) >= 32768u) {
                poll_ticks = 0;
                if (lane == 0 && __hip_atomic_load(cload_k<WgArgs>(kernarg).stop_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)
                    (void) wga_raise_stop<WG>(q_ctl, STOP_CANCEL);
            }
            // a path that never comes back (a lost hand-over, see the protocol notes) would leave the finished count short for ever:
            // after MTS_IDLE_TICKS with every ring empty the wave reports it (diagnostic code 3) instead
            if (wga_idle_expired(idle_naps, idle_t0, idle_limit)) wga_stall<WG>(3u, B_DONE, 0u, q_ctl, cload_k<WgArgs>(kernarg).counters);
            __builtin_amdgcn_s_sleep(2);
#if defined(MTSAMD_BLOCKSTATS)
            if (COUNT) { long long t = clock64(); bs_loc[42] += (unsigned long long) (t - bs_t0); bs_t0 = t; }
#endif
            continue;
        }
        idle_naps = 0;
        // ---- claim up to 64 ids
        n = best < 64u ? best : 64u;
        h = (uint32_t) __builtin_amdgcn_readlane((int) hd, sel);
        uint32_t won = 0;
        // the slots are read together with the compare-and-swap (both depend on the snapshot only); a lost claim discards them
        if (lane < n) spec_slot = __atomic_load_n(&q_ids[sel][(h + lane) & (uint32_t) (WG - 1)], __ATOMIC_RELAXED);
        if (lane == 0) won = atomicCAS(&q_ctl[2 * sel], h, h + n) == h ? 1u : 0u;
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) { bs_loc[10] += 1ull; if (!__builtin_amdgcn_readfirstlane((int) won)) bs_loc[11] += 1ull; }      // claim attempts / lost compare-and-swaps
#endif
        if (__builtin_amdgcn_readfirstlane((int) won)) break;
      }
      if (finished) break;
        uint32_t pid = 0xFFFFu;
        bool mine = lane < n;
        {
            uint16_t *slot = &q_ids[sel][(h + lane) & (uint32_t) (WG - 1)];
            const bool ready = mine && RingSlot<WG>::matches(spec_slot, h + lane);
            if (ready) pid = RingSlot<WG>::id(spec_slot);
            if (__builtin_amdgcn_ballot_w64(mine && !ready) != 0ull) {           // a lane ahead of its producer (rare)
                const uint32_t got = wga_tag_wait<WG>(mine && !ready, slot, q_ctl, cload_k<WgArgs>(kernarg).counters, sel, h + lane);
                if (mine && !ready) pid = got;
                mine = mine && pid != 0xFFFFu;                // 0xFFFF: the workgroup is stopping, the lane drops out
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) { bs_loc[sel] += 1ull; bs_loc[12 + sel] += (unsigned long long) n;
                     long long t = clock64(); bs_loc[44] += (unsigned long long) (t - bs_t0); bs_t0 = t; }
#endif
        int cls = B_DONE;
        if (mine) {
            switch (sel) {                                      // wave-uniform
                case B_INT: cls = M::template block<B_INT>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_MED: cls = M::template block<B_MED>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_MEDW: cls = M::template block<B_MEDW>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_SCATTER: cls = M::template block<B_SCATTER>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_WSURF: cls = M::template block<B_WSURF>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_SURF: cls = M::template block<B_SURF>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_PHASE: cls = M::template block<B_PHASE>(kernarg, hot_lds, wg_base, pid, &cnt); break;
                case B_CROSS:                                   // never claimed by a machine without the class
                    if constexpr (M::CROSS) {
                        cls = M::template block<B_CROSS>(kernarg, hot_lds, wg_base, pid, &cnt);
                        if (COUNT && lane == 0) atomicAdd(cload_k<WgArgs>(kernarg).counters + MTS_CROSS_SLOT, (unsigned long long) n);     // lane-visits of the class
                    }
                    break;
                default: cls = M::template block<B_NEW>(kernarg, hot_lds, wg_base, pid, &cnt); break;
            }
        }
        // should_stop() for a busy wave: see the nap above.  Here, in the wake of the NEW block's film atomics, the vector load is cheap; at
        // the head of the claim loop it measured 3.5 % however seldom it ran.
        if (sel == B_NEW && (poll_ticks += 256u) >= 32768u) {
            poll_ticks = 0;
            if (lane == 0 && __hip_atomic_load(cload_k<WgArgs>(kernarg).stop_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)
                (void) wga_raise_stop<WG>(q_ctl, STOP_CANCEL);
        }
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) { long long t = clock64(); bs_loc[24 + sel] += (unsigned long long) (t - bs_t0); bs_t0 = t; }
#endif
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        if (COUNT && drop_one && cls != B_DONE) { mine = mine && lane != 0u; drop_one = false; }      // the injected lost hand-over (test hook)
        if (record_cost && mine && cls == B_DONE)             // once per path: calibration launches only
            atomicAdd(cload_k<WgArgs>(kernarg).counters + MTS_COST_BASE + (wg_base + pid) / MTS_TILE_PIXELS, (unsigned long long) (clock64() - cost_t0));
        wga_push<WG>(cls, pid, mine, q_ids, q_ctl);
#if defined(MTSAMD_BLOCKSTATS)
        if (COUNT) { long long t = clock64(); bs_loc[43] += (unsigned long long) (t - bs_t0); bs_t0 = t; }
#endif
    }
#if defined(MTSAMD_BLOCKSTATS)
    if (COUNT) {
        long long t = clock64(); bs_loc[44] += (unsigned long long) (t - bs_t0);
        for (int k = 0; k < 6; ++k) bs_loc[36 + k] = cnt.seg[k];
        if (lane == 0) for (int k = 0; k < 48; ++k) atomicAdd(&g_blockstats[k], bs_loc[k]);
    }
#endif
    __syncthreads();                                          // every wave has left the loop: the path state is final
    if (__atomic_load_n(&q_ctl[2 * B_COUNT], __ATOMIC_RELAXED) != STOP_NONE) wg_flush_unfinished<WG, NT, M::Machine::MOMENT>(kernarg, hot_lds, M::PACKED, wg_base);
}

} // inline namespace
} // namespace mtsamd
