// capi.cpp -- the extern "C" entry points declared in include/mtsamd.h.
//
// -DMTSAMD_HOST_ONLY (tests/test_host_sanitizers.py: the host pass alone, built with AddressSanitizer + UndefinedBehaviorSanitizer):
// everything that validates and flattens caller-owned records runs as in the product -- mts_scene_create up to the upload, mts_render
// up to the first device call (options, passes, spiral, shard filter, film capacity, kernel choice) -- and every entry point that would touch the GPU
// reports "host-only build" instead.
//
// mts_render mirrors SamplingIntegrator::render (/root/reference/src/librender/integrator.cpp:51-179): the pass / block bookkeeping
// of render_plan.cpp on the host, then the launches.  No exception crosses the boundary: errors become a non-zero status + mts_last_error().
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <atomic>
#include <signal.h>
#include "scene_host.h"
#include "launch.h"
#include "render_plan.cpp"         // part of this translation unit: scene_host.cpp + capi.cpp are the whole host side (tests/test_render_plan.py builds it alone)

using namespace mtsamd;

static thread_local std::string g_error;

#define API_TRY try {
#define API_CATCH } catch (const std::exception &e) { g_error = e.what(); return 1; } catch (...) { g_error = "unknown error"; return 1; } return 0;
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// Device buffers and events a render needs besides the scene; they are kept with the handle and only grow, so that a sequence of
// renders of one scene (passes, sensors swept by the caller, benchmark steps) pays for hipMalloc / hipFree -- which synchronise
// the device -- once.  Guarded by render_mutex.
// BUF_FILM: the film of a host-film render; BUF_SLOTS: the film slots of the passes (RenderPlan::pass_slots)
enum RenderBuffer { BUF_FILM, BUF_COUNTERS, BUF_BLOCKS, BUF_WORKSPACE, BUF_TILES, BUF_SLOTS, BUF_COUNT };
struct RenderCache {
    void *ptr[BUF_COUNT] = {};
    size_t cap[BUF_COUNT] = {};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void *get(RenderBuffer k, size_t bytes) {
        bytes = std::max<size_t>(bytes, 16);
        if (cap[k] < bytes) {
            if (ptr[k]) { (void) hipFree(ptr[k]); ptr[k] = nullptr; cap[k] = 0; }
            hipError_t e = hipMalloc(&ptr[k], bytes);
            if (e != hipSuccess) throw std::runtime_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
            cap[k] = bytes;
        }
        return ptr[k];
    }
    void events() {
        if (!ev0) { if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) throw std::runtime_error("hipEventCreate failed"); }
    }
    void release() {
        for (int k = 0; k < BUF_COUNT; ++k) if (ptr[k]) { (void) hipFree(ptr[k]); ptr[k] = nullptr; cap[k] = 0; }
        if (ev0) { (void) hipEventDestroy(ev0); ev0 = nullptr; }
        if (ev1) { (void) hipEventDestroy(ev1); ev1 = nullptr; }
    }
};
// stop_word: one word of pinned, device-visible host memory per scene -- the m_stop of Integrator::cancel() (integrator.cpp:43-45)
// as the kernels see it (stop_requested(), the stop word of the ring driver).  mts_cancel stores to it from any thread.
struct mts_scene { HostScene *hs; std::mutex render_mutex; RenderCache cache; volatile uint32_t *stop_word = nullptr; };

namespace {
template <typename T> struct DeviceBuffer {
    T *p = nullptr;
    explicit DeviceBuffer(size_t n) { HIP_CHECK(hipMalloc((void **) &p, std::max<size_t>(n * sizeof(T), 16))); }
    ~DeviceBuffer() { if (p) (void) hipFree(p); }
    DeviceBuffer(const DeviceBuffer &) = delete;
};
} // namespace

extern "C" {

int mts_abi_version(void) { return MTS_ABI_VERSION; }
#ifndef MTSAMD_BUILD_ID
#define MTSAMD_BUILD_ID "unidentified...."
#endif
static const char g_build_id[] = "MTSAMD_BUILD_ID=" MTSAMD_BUILD_ID;   // also readable from the file without loading it (eradiate-kernel_amd/_buildid.py)
#ifndef MTSAMD_TOOLCHAIN_ID
#define MTSAMD_TOOLCHAIN_ID "unknown."
#endif
// the compiler that built it (hash of `hipcc --version`): build.py rebuilds when it changes; read from the file's bytes only
__attribute__((used)) static const char g_toolchain_id[] = "MTSAMD_TOOLCHAIN=" MTSAMD_TOOLCHAIN_ID;
const char *mts_build_id(void) { return g_build_id + 16; }
const char *mts_last_error(void) { return g_error.c_str(); }

int mts_abi_sizeof(const char *name) {
#define SZ(T) if (!strcmp(name, #T)) return (int) sizeof(T);
    SZ(mts_spectrum) SZ(mts_transform) SZ(mts_volume) SZ(mts_phase) SZ(mts_medium) SZ(mts_bsdf) SZ(mts_shape) SZ(mts_emitter)
    SZ(mts_sensor) SZ(mts_integrator) SZ(mts_scene_desc) SZ(mts_stats) SZ(mts_render_opts) SZ(mts_dirty) SZ(mts_texture)
#undef SZ
    return -1;
}

#if defined(MTSAMD_HOST_ONLY)
#define HOST_ONLY_STOP(what) throw std::runtime_error(std::string(what) + ": host-only build (validated, nothing launched)")
#endif

int mts_device_count(int *count) {
    API_TRY
#if defined(MTSAMD_HOST_ONLY)
    (void) count; HOST_ONLY_STOP("mts_device_count");
#else
    HIP_CHECK(hipGetDeviceCount(count));
#endif
    API_CATCH
}

int mts_scene_create(const mts_scene_desc *desc, int device, mts_scene **out) {
    API_TRY
    if (!out) throw std::runtime_error("mts_scene_create: out is NULL");
    HostScene *hs = build_host_scene(desc);
#if defined(MTSAMD_HOST_ONLY)
    (void) device;
    mts_scene *s = new mts_scene(); s->hs = hs;
    s->stop_word = new uint32_t(0);
#else
    try { upload_host_scene(*hs, device); } catch (...) { free_host_scene(hs); throw; }
    mts_scene *s = new mts_scene(); s->hs = hs;
    void *sw = nullptr;
    if (hipHostMalloc(&sw, 64, hipHostMallocDefault) != hipSuccess) { free_host_scene(hs); delete s; throw std::runtime_error("hipHostMalloc failed (stop word)"); }
    s->stop_word = (volatile uint32_t *) sw; *s->stop_word = 0;
#endif
    *out = s;
    API_CATCH
}

// Not part of the ABI (include/mtsamd.h does not declare it): which promises of integrator_dev.h's scene traits a description keeps
// (scene_host.cpp: scene_traits) -- what decides which lean translation unit mts_render launches.  Host only: no device is touched, so the
// CPU test-suite pins the decision (tests/test_abi.py::test_scene_traits).
int mts_debug_scene_traits(const mts_scene_desc *desc, int32_t *traits) {
    API_TRY
    if (!traits) throw std::runtime_error("mts_debug_scene_traits: traits is NULL");
    HostScene *hs = build_host_scene(desc);
    *traits = hs->traits;
    free_host_scene(hs);
    API_CATCH
}

// Not part of the ABI either: DScene::cross_mask of a description's host scene -- the shapes whose hits the ring machines sort into the
// class of null-boundary crossings (volpath_flat.h: B_CROSS).  Host only (tests/test_gpu_cross_class.py pins it on hand-built shape lists).
int mts_debug_cross_mask(const mts_scene_desc *desc, uint64_t *mask) {
    API_TRY
    if (!mask) throw std::runtime_error("mts_debug_cross_mask: mask is NULL");
    HostScene *hs = build_host_scene(desc);
    *mask = hs->scene.cross_mask;
    free_host_scene(hs);
    API_CATCH
}

// ... and how many lane-visits the class B_CROSS served in this process's last render with loop counters (0: the kernel has no such
// class, or met no crossing): the test that the lean units a and b do fill their ninth ring.  ONE value per process, not per scene:
// every mts_render of any scene on any thread overwrites it, so it means something only to a caller that renders one scene at a time
// and asks right after (tests/test_gpu_cross_class.py does).  mts_stats has no room for it without a change of the ABI.
static std::atomic<unsigned long long> g_last_cross_visits{0};
int mts_debug_cross_visits(uint64_t *visits) {
    API_TRY
    if (!visits) throw std::runtime_error("mts_debug_cross_visits: visits is NULL");
    *visits = g_last_cross_visits.load();
    API_CATCH
}

int mts_scene_destroy(mts_scene *scene) {
    if (scene) {
#if defined(MTSAMD_HOST_ONLY)
        delete (uint32_t *) scene->stop_word;
#else
        (void) hipSetDevice(scene->hs->device); scene->cache.release();
        if (scene->stop_word) (void) hipHostFree((void *) scene->stop_word);
#endif
        free_host_scene(scene->hs); delete scene;
    }
    return 0;
}

int mts_cancel(mts_scene *scene) {
    if (!scene) { g_error = "mts_cancel: scene is NULL"; return 1; }
    scene->hs->stop.store(1);
    if (scene->stop_word) *scene->stop_word = 1;          // seen by the running kernels within a few microseconds
    return 0;
}

// ---- the SIGINT scope (integrator_v.cpp:129-151).  The handler touches lock-free atomics, one word of pinned host memory,
// sigaction and raise: all async-signal-safe.
static std::atomic<mts_scene *> g_sigint_scene{nullptr};
static struct sigaction g_sigint_prev;
static_assert(std::atomic<int>::is_always_lock_free, "the stop flag is stored from a signal handler");
static void mts_sigint_handler(int) {
    mts_scene *s = g_sigint_scene.exchange(nullptr);
    if (!s) return;
    s->hs->stop.store(1);                                  // = mts_cancel
    if (s->stop_word) *s->stop_word = 1;
    (void) sigaction(SIGINT, &g_sigint_prev, nullptr);     // the previous handler sees the signal as well (Python: KeyboardInterrupt once
    (void) raise(SIGINT);                                  // the interpreter runs again, i.e. after the render has wound down)
}

int mts_sigint_scope_enter(mts_scene *scene) {
    if (!scene) { g_error = "mts_sigint_scope_enter: scene is NULL"; return 1; }
    mts_scene *expected = nullptr;
    if (!g_sigint_scene.compare_exchange_strong(expected, scene)) { g_error = "mts_sigint_scope_enter: another scope is open"; return 1; }
    struct sigaction sa; memset(&sa, 0, sizeof(sa));
    sa.sa_handler = mts_sigint_handler; sigemptyset(&sa.sa_mask);
    if (sigaction(SIGINT, &sa, &g_sigint_prev) != 0) { g_sigint_scene.store(nullptr); g_error = "mts_sigint_scope_enter: sigaction failed"; return 1; }
    return 0;
}

int mts_sigint_scope_exit(void) {
    // a handler that ran has already put the previous one back (and emptied the slot); otherwise do it here
    if (g_sigint_scene.exchange(nullptr)) (void) sigaction(SIGINT, &g_sigint_prev, nullptr);
    return 0;
}

// What choose_kernel (render_plan.cpp; DESIGN.md section 4, "kernel table") reads of a scene
// (a `moment` scene presents no traits: its kernels are in the general unit)
// Facts, traits and the choice are those of a (scene, sensor) pair: `sv` is the sensor that renders (scene_host.h: host_sensor)
static KernelFacts facts_of(const HostScene &hs, const SensorView &sv) { return { hs.integrator.type, hs.integrator.spectral != 0, hs.integrator.use_spectral_mis != 0, !hs.media.empty(), hs.scene.bin_count > 0, sv.srf >= 0, sv.srf_lookup_by_wavelength, sv.sensor->wavefront != 0, hs.integrator.moment ? 0 : sv.traits }; }
// The kernel that renders a scene: the table's choice, which the `moment` wrapper maps to its own instantiation of that row or to the
// nested moment kernel (kernel_names.h: kv::moment_variant)
static KernelChoice kernel_of(const HostScene &hs, const SensorView &sv, uint32_t block_size, const RenderSwitches &sw, bool counters) {
    KernelChoice kc = choose_kernel(facts_of(hs, sv), block_size, sw);
    if (hs.integrator.moment) kc.variant = kv::moment_variant(kc.variant, hs.integrator.type, sv.sensor->wavefront != 0, counters);
    return kc;
}

// Not part of the ABI either: mts_stats.kernel_variant as mts_render would report it for this description under the environment's
// switches.  Host only (tests/test_abi.py::test_kernel_choice).
int mts_debug_kernel_choice(const mts_scene_desc *desc, int32_t *kernel_variant) {
    API_TRY
    if (!kernel_variant) throw std::runtime_error("mts_debug_kernel_choice: kernel_variant is NULL");
    HostScene *hs = build_host_scene(desc);
    try {
        const KernelChoice kc = kernel_of(*hs, host_sensor(*hs, 0), plan_block_size(hs->integrator.block_size), read_render_switches(), false);
        *kernel_variant = kv::stat(kc.variant, kc.unit);
    } catch (...) { free_host_scene(hs); throw; }
    free_host_scene(hs);
    API_CATCH
}

// Not part of the ABI either: what sensor `sensor` of a scene would render on -- the scene of `desc` with the `n_extra` sensors of
// `extra` added in order (mts_scene_add_sensor's host half): the traits of that (scene, sensor) pair and mts_stats.kernel_variant
// as mts_render_sensor would report it.  Host only (tests/test_sensors.py compares with the single-sensor description's
// mts_debug_scene_traits / mts_debug_kernel_choice).
int mts_debug_sensor_choice(const mts_scene_desc *desc, const mts_sensor *extra, int32_t n_extra, int32_t sensor, int32_t *traits, int32_t *kernel_variant) {
    API_TRY
    if (!traits || !kernel_variant) throw std::runtime_error("mts_debug_sensor_choice: NULL output");
    if (n_extra < 0 || (n_extra > 0 && !extra)) throw std::runtime_error("mts_debug_sensor_choice: a negative count, or sensors missing");
    HostScene *hs = build_host_scene(desc);
    try {
        for (int32_t k = 0; k < n_extra; ++k) (void) add_host_sensor(*hs, extra + k);
        const SensorView sv = host_sensor(*hs, sensor);
        const KernelChoice kc = kernel_of(*hs, sv, plan_block_size(hs->integrator.block_size), read_render_switches(), false);
        *traits = sv.traits; *kernel_variant = kv::stat(kc.variant, kc.unit);
    } catch (...) { free_host_scene(hs); throw; }
    free_host_scene(hs);
    API_CATCH
}

// Further sensors of a scene: sensor 0's constructor against the scene as created (scene_host.cpp: add_host_sensor).  Like an update
// it is refused, not made to wait, while a render or another call holds the handle.
int mts_scene_add_sensor(mts_scene *scene, const mts_sensor *sensor, int32_t *index) {
    API_TRY
    if (!scene) throw std::runtime_error("mts_scene_add_sensor: scene is NULL");
    std::unique_lock<std::mutex> guard(scene->render_mutex, std::try_to_lock);
    if (!guard.owns_lock()) throw std::runtime_error("mts_scene_add_sensor: a render of this scene is in flight (or another call on this handle: a sample / intersection query, an update)");
    const int32_t i = add_host_sensor(*scene->hs, sensor);
    if (index) *index = i;
    API_CATCH
}

int mts_scene_sensor_count(mts_scene *scene, int32_t *count) {
    API_TRY
    if (!scene || !count) throw std::runtime_error("mts_scene_sensor_count: NULL argument");
    *count = scene->hs->sensor_count.load();
    API_CATCH
}

// traverse() + params.update() of the reference (src/python/python/util.py:14-190): the dirty records of `desc` and everything derived
// from them are rebuilt by the constructors' own functions and rewritten in place (scene_host.cpp: update_host_scene)
int mts_scene_update(mts_scene *scene, const mts_scene_desc *desc, const mts_dirty *dirty, int32_t n, void *stream) {
    API_TRY
    if (!scene) throw std::runtime_error("mts_scene_update: scene is NULL");
    // every entry that reads the device scene (mts_render for the whole render, mts_sample / _spectral, mts_ray_intersect, the digest) or
    // rewrites it (another update) holds the handle's mutex: an update never waits for them, it is refused
    std::unique_lock<std::mutex> guard(scene->render_mutex, std::try_to_lock);
    if (!guard.owns_lock()) throw std::runtime_error("mts_scene_update: a render of this scene is in flight (or another call on this handle: a sample / intersection query, another update)");
    update_host_scene(*scene->hs, desc, dirty, n, (hipStream_t) stream);
    API_CATCH
}

// Not part of the ABI: the host half of an update -- build_host_scene(before), then mts_scene_update's work with `after` through the
// host functions -- and what the next render would run on: the traits and mts_stats.kernel_variant.  No device is touched
// (tests/test_traverse.py compares with mts_debug_scene_traits / mts_debug_kernel_choice of `after`).
int mts_debug_update_plan(const mts_scene_desc *before, const mts_scene_desc *after, const mts_dirty *dirty, int32_t n, int32_t *traits, int32_t *kernel_variant) {
    API_TRY
    if (!traits || !kernel_variant) throw std::runtime_error("mts_debug_update_plan: NULL output");
    HostScene *hs = build_host_scene(before);
    try {
        update_host_scene(*hs, after, dirty, n, nullptr);
        const KernelChoice kc = kernel_of(*hs, host_sensor(*hs, 0), plan_block_size(hs->integrator.block_size), read_render_switches(), false);
        *traits = hs->traits; *kernel_variant = kv::stat(kc.variant, kc.unit);
    } catch (...) { free_host_scene(hs); throw; }
    free_host_scene(hs);
    API_CATCH
}

// Not part of the ABI: a hash of the device scene's contents (scene_host.cpp: digest_host_scene).  Two scenes with equal digests render equal films.
int mts_debug_scene_digest(mts_scene *scene, uint64_t *out8) {
    API_TRY
    if (!scene || !out8) throw std::runtime_error("mts_debug_scene_digest: NULL argument");
    std::lock_guard<std::mutex> guard(scene->render_mutex);
#if defined(MTSAMD_HOST_ONLY)
    digest_host_scene(*scene->hs, false, out8);           // a host-only handle has no device copy: the walk over the host's own arrays
#else
    digest_host_scene(*scene->hs, true, out8);
#endif
    API_CATCH
}

// Not part of the ABI: the same hash of the host scene a description builds, taken from the host's own arrays.  No device is touched, so
// the CPU test-suite can tell whether a change of the host side altered what the kernels receive (tests/test_host_digest.py).
int mts_debug_desc_digest(const mts_scene_desc *desc, uint64_t *out8) {
    API_TRY
    if (!out8) throw std::runtime_error("mts_debug_desc_digest: out8 is NULL");
    HostScene *hs = build_host_scene(desc);
    try { digest_host_scene(*hs, false, out8); } catch (...) { free_host_scene(hs); throw; }
    free_host_scene(hs);
    API_CATCH
}

// Not part of the ABI: how a description's geometry is laid out on the host.  counts[6]: the scene level's primitives (an instance is
// one), all primitives (the groups' members behind the scene's), instances, groups, the scene level's BVH nodes, all BVH nodes;
// bbox[6]: the scene's bounding box, min then max.  Host only (tests/test_instance.py: members are not scene geometry).
int mts_debug_scene_geometry(const mts_scene_desc *desc, int32_t *counts, float *bbox) {
    API_TRY
    if (!counts || !bbox) throw std::runtime_error("mts_debug_scene_geometry: NULL output");
    HostScene *hs = build_host_scene(desc);
    counts[0] = hs->scene.prim_count; counts[1] = (int32_t) hs->prims.size(); counts[2] = (int32_t) hs->instances.size(); counts[3] = (int32_t) hs->groups.size();
    counts[4] = hs->scene.bvh_node_count; counts[5] = (int32_t) (hs->bvh_nodes.size() / 8);
    for (int k = 0; k < 3; ++k) { bbox[k] = hs->scene.bbox.min[k]; bbox[3 + k] = hs->scene.bbox.max[k]; }
    free_host_scene(hs);
    API_CATCH
}

#if !defined(MTSAMD_HOST_ONLY)
// the launcher of each unit (UNIT_GENERAL: launch_render, or launch_render_spectral for a scene of the spectral variant)
#if defined(MTSAMD_BLOCKSTATS)
static const RenderLauncher RENDER_LAUNCHERS[] = { launch_render };
#else
static const RenderLauncher RENDER_LAUNCHERS[] = { launch_render, launch_render_lean_a, launch_render_lean_b, launch_render_lean_s,
                                                   launch_render_lean_p, launch_render_lean_ps, launch_render_lean_h, launch_render_lean_c };
static_assert(sizeof(RENDER_LAUNCHERS) / sizeof(RENDER_LAUNCHERS[0]) == UNIT_COUNT, "one launcher per KernelUnit, in the enum's order");
#endif
#endif

// Sensor `sensor` of the scene renders: plan, film size, kernel facts, traits and the kernel choice are that sensor's.  The kernels get
// a COPY of the scene's DScene with the sensor's record and srf in it (RenderArgs::sc): hs.scene, which mts_sample, mts_ray_intersect,
// the digest and mts_scene_update read, is never written -- whatever a render throws, nothing is left swapped.
int mts_render_sensor(mts_scene *scene, int32_t sensor, const mts_render_opts *opts_, float *film, mts_stats *stats) {
    API_TRY
    if (!scene || !film) throw std::runtime_error("mts_render: NULL argument");
    std::lock_guard<std::mutex> guard(scene->render_mutex);         // one render per handle at a time
    HostScene &hs = *scene->hs;
    SensorView sv;
    try { sv = host_sensor(hs, sensor); } catch (const std::runtime_error &e) { throw std::runtime_error(std::string("mts_render_sensor: ") + e.what()); }
    DScene sc = hs.scene;
    sc.sensor = *sv.sensor; sc.srf = sv.srf;
    mts_render_opts opts; memset(&opts, 0, sizeof(opts)); opts.shard_count = 1;
    if (opts_) opts = *opts_;
    if (opts.shard_count < 1 || opts.shard_index < 0 || opts.shard_index >= opts.shard_count) throw std::runtime_error("mts_render: invalid shard specification");
    const RenderSwitches sw = read_render_switches();
    auto t0 = std::chrono::steady_clock::now();
    hs.stop.store(0);                                               // integrator.cpp:53
    int cus = 256;
#if !defined(MTSAMD_HOST_ONLY)
    HIP_CHECK(hipSetDevice(hs.device));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hs.device));
#endif
    hipStream_t stream = (hipStream_t) opts.stream;
    const DSensor &se = sc.sensor;
    RenderPlan plan = plan_render(se, hs.integrator.samples_per_pass, hs.integrator.block_size, hs.scene.film_channels, opts.shard_index, opts.shard_count, cus, sw);
    const uint32_t block_size = plan.block_size; const size_t film_floats = plan.film_floats;
    if (opts.film_capacity > 0 && (uint64_t) opts.film_capacity < (uint64_t) film_floats)
        throw std::runtime_error("mts_render: the film buffer holds " + std::to_string(opts.film_capacity) + " floats, this scene writes " + std::to_string(film_floats) +
                                 " (crop_width x crop_height x " + std::to_string(hs.scene.film_channels) + " channels: " +
                                 (hs.integrator.moment ? "X, Y, Z, A, W + the moment integrator's m1.X, m1.Y, m1.Z, m2.X, m2.Y, m2.Z)" : "X, Y, Z, A, W + two per spectral bin)"));
    const KernelChoice kc = kernel_of(hs, sv, block_size, sw, opts.collect_counters != 0);
    // a textured scene: the TEX instantiation that renders the table's row (kernel_names.h); mts_stats.kernel_variant keeps naming the row
    const bool textured = !hs.bsdf_tex.empty();            // texture records, a blendbsdf, a twosided, a dielectric or a conductor (scene_host.cpp: build_textures); an instanced scene has the table too
    const bool instanced = !hs.instances.empty() || hs.has_cone;   // instances or a cone: the INST kernels (kernels.hip): the TEX instantiations over the two-level traversal, mapped from the row alike
    const int variant = textured ? kv::textured_variant(kc.variant, hs.integrator.type, se.wavefront != 0, opts.collect_counters != 0) : kc.variant;
#if defined(MTSAMD_HOST_ONLY)
    (void) stream; (void) t0; (void) stats; (void) variant; (void) instanced; (void) sc;
    HOST_ONLY_STOP("mts_render");
#else
    RenderCache &rc = scene->cache;
    float *d_film = film;
    if (!opts.film_on_device) d_film = (float *) rc.get(BUF_FILM, film_floats * sizeof(float));
    constexpr int N_COUNTERS = 16;                                   // [0..2] loop counters, [4..9] ring-stall record (ring_driver.h, MTS_DIAG_BASE), [15] cost-recording flag
    // [16 + s]: cost of tile slot s of a calibration launch (16 pixels per tile: block_size^2 / 16 slots per block of the first chunk)
    const uint32_t tiles_per_block = block_size * block_size / 16u;
    unsigned long long *d_counters = (unsigned long long *) rc.get(BUF_COUNTERS, (N_COUNTERS + std::max<size_t>(1, plan.chunks[0].size()) * (tiles_per_block + 1u)) * sizeof(unsigned long long));
    HIP_CHECK(hipMemsetAsync(d_film, 0, film_floats * sizeof(float), stream));               // hdrfilm.cpp:201-203 (storage cleared by prepare())
    float *d_target = d_film;                                        // what the kernels add to: the film, or the slots of the passes
    if (plan.pass_slots) {
        d_target = (float *) rc.get(BUF_SLOTS, plan.n_slots * film_floats * sizeof(float));
        HIP_CHECK(hipMemsetAsync(d_target, 0, plan.n_slots * film_floats * sizeof(float), stream));
    }
    HIP_CHECK(hipMemsetAsync(d_counters, 0, N_COUNTERS * sizeof(unsigned long long), stream));
    if (sw.inject_lost_path != 0 && opts.collect_counters)          // test hook of the ring drivers' error path (ring_driver.h, MTS_INJECT_SLOT): idle bound in ticks
        HIP_CHECK(hipMemcpyAsync(d_counters + 14, &sw.inject_lost_path, sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    rc.events();
    double kernel_ms = 0.0, calibration_ms = 0.0; int launches = 0, calibration_launches = 0, last_variant = 0; bool timed_out = false;
    const float timeout = hs.integrator.timeout;
    *scene->stop_word = 0;
    if (hs.stop.load()) *scene->stop_word = 1;                      // cancel() raced the start of the render
    auto should_stop = [&]() {                                      // integrator.h:143-146
        if (hs.stop.load()) return true;
        if (timeout > 0.f && std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count() > timeout) { timed_out = true; return true; }
        return false;
    };
    auto throw_on_ring_stall = [](const unsigned long long *c) {    // counters[4..9]: a bounded ring wait gave up (ring_driver.h): an error, never a hang
        if (c[4] != 0)
            throw std::runtime_error("render kernel: " + std::string(c[4] == 3 ? "lost path (nothing waiting, finished paths = tail" : c[4] == 1 ? "ring stall (consumer" : "ring stall (producer") + ", ring " + std::to_string(c[5]) +
                                     ", index " + std::to_string(c[6]) + ", head " + std::to_string(c[7]) + ", tail " + std::to_string(c[8]) +
                                     ", workgroup " + std::to_string(c[9]) + ")");
    };
    try {
        last_variant = kv::stat(kc.variant, kc.unit);
        if (instanced && (kc.unit != UNIT_GENERAL || hs.integrator.spectral || !textured)) throw std::runtime_error("mts_render: an instanced scene outside the general rgb / mono unit");
        const RenderLauncher launcher = kc.unit == UNIT_GENERAL && hs.integrator.spectral ? launch_render_spectral : RENDER_LAUNCHERS[kc.unit];

        // one launch over `blocks` with `spp` samples per pixel, watched for cancel() / the timeout (which reach the kernel through the stop word).
        // `tiles`: the cost-sorted tile table of the regrouping kernels (volpath_flat.h, WgArgs::tiles), or empty: one workgroup per
        // run of a block's Morton order.
        auto launch = [&](const std::vector<DBlock> &blocks, uint32_t spp, const std::vector<uint32_t> &tiles) {
            DBlock *d_blocks = (DBlock *) rc.get(BUF_BLOCKS, blocks.size() * sizeof(DBlock));
            HIP_CHECK(hipMemcpyAsync(d_blocks, blocks.data(), blocks.size() * sizeof(DBlock), hipMemcpyHostToDevice, stream));
            uint32_t *d_tiles = nullptr;
            if (!tiles.empty()) {
                d_tiles = (uint32_t *) rc.get(BUF_TILES, tiles.size() * sizeof(uint32_t));
                HIP_CHECK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            }
            const uint64_t paths = tiles.empty() ? (uint64_t) blocks.size() * block_size * block_size : (uint64_t) tiles.size() * 16u;
            HIP_CHECK(hipEventRecord(rc.ev0, stream));
            // one 128-byte cold record per path in flight; volpathmis parks the path's two weight matrices in a second one (volpathmis_flat.h)
            const size_t ws_records = hs.integrator.type == MTS_INTEGRATOR_VOLPATHMIS ? 2 : 1;
            float *d_ws = (float *) rc.get(BUF_WORKSPACE, render_workspace_floats(paths, variant) * ws_records * sizeof(float));
            const RenderArgs args = { &sc, d_blocks, (uint32_t) blocks.size(), block_size, spp, d_target, d_counters, opts.collect_counters != 0, variant,
                                      d_ws, (const uint32_t *) scene->stop_word, d_tiles, (uint32_t) tiles.size(), stream, hs.integrator.moment != 0, textured, instanced };
            HIP_CHECK(launcher(args));
            HIP_CHECK(hipEventRecord(rc.ev1, stream));
            for (;;) {
                hipError_t q = hipEventQuery(rc.ev1);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) HIP_CHECK(q);
                if (should_stop()) *scene->stop_word = 1;
                std::this_thread::sleep_for(std::chrono::microseconds(50));
            }
            float ms = 0.f; HIP_CHECK(hipEventElapsedTime(&ms, rc.ev0, rc.ev1));
            kernel_ms += ms; ++launches;
        };

        // calibration (render_plan.cpp: lpt_policy): a few samples per pixel, every path adding its finishing time to the cost of its tile
        const LptPolicy lpt = lpt_policy(sw.lpt, variant, hs.integrator.spectral || hs.integrator.type == MTS_INTEGRATOR_VOLPATHMIS, plan, cus, should_stop());
        CostIndex cost_index;
        std::vector<uint64_t> tile_cost;
        if (lpt.cal_spp > 0) {
            const std::vector<DBlock> cal = calibration_blocks(plan.chunks[0]);
            const size_t n_cost = cal.size() * tiles_per_block;
            HIP_CHECK(hipMemsetAsync(d_counters + N_COUNTERS, 0, n_cost * sizeof(unsigned long long), stream));
            const unsigned long long flag = 1ull;
            HIP_CHECK(hipMemcpyAsync(d_counters + 15, &flag, sizeof(flag), hipMemcpyHostToDevice, stream));
            launch(cal, lpt.cal_spp, {});                          // identity tiles: tile slot = block index * tiles_per_block + tile
            calibration_ms = kernel_ms; calibration_launches = launches; kernel_ms = 0.0; launches = 0;      // timed apart from the render (mts_stats)
            tile_cost.resize(n_cost);
            HIP_CHECK(hipMemcpyAsync(tile_cost.data(), d_counters + N_COUNTERS, n_cost * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            unsigned long long diag[N_COUNTERS] = {};
            HIP_CHECK(hipMemcpyAsync(diag, d_counters, sizeof(diag), hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            throw_on_ring_stall(diag);                             // a bounded wait that gave up during calibration is an error like any other
            cost_index = smooth_tile_costs(tile_cost, cal, block_size, se);
            if (sw.lpt_debug) report_tile_costs(tile_cost, cal.size(), tiles_per_block, lpt.cal_spp);
            // A cancel or the timeout that landed during calibration: the samples it rendered are the first of every pixel's stream --
            // they stay as the (partial) film, as a stopped render keeps its finished samples; otherwise they are not part of the image
            if (!should_stop()) {
                HIP_CHECK(hipMemsetAsync(d_target, 0, film_floats * sizeof(float), stream));
                HIP_CHECK(hipMemsetAsync(d_counters, 0, N_COUNTERS * sizeof(unsigned long long), stream));
            }
        }
        for (std::vector<DBlock> &blocks : plan.chunks) {
            if (should_stop()) break;
            if (blocks.empty()) continue;
            const std::vector<uint32_t> tiles = cost_index.empty() ? std::vector<uint32_t>() : schedule_chunk(blocks, cost_index, tile_cost, block_size, lpt.use_tiles, (uint32_t) kv::ring_paths(variant));
            launch(blocks, (uint32_t) plan.launch_spp, tiles);
        }
        if (plan.pass_slots) HIP_CHECK(launch_film_sum_slots(d_film, d_target, film_floats, (uint32_t) plan.n_slots, stream));
        if (!opts.film_on_device) HIP_CHECK(hipMemcpyAsync(film, d_film, film_floats * sizeof(float), hipMemcpyDeviceToHost, stream));
        unsigned long long h_counters[N_COUNTERS] = {};
        HIP_CHECK(hipMemcpyAsync(h_counters, d_counters, sizeof(h_counters), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        throw_on_ring_stall(h_counters);
        g_last_cross_visits.store(h_counters[3]);                    // ring_driver.h: MTS_CROSS_SLOT (zero unless the counting variant of a ring kernel ran)
        const bool cancelled = hs.stop.load() != 0;                  // render() returns !m_stop (integrator.cpp:178): a timeout alone is not a cancellation
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->samples = plan.samples; stats->n_iter = h_counters[0]; stats->n_lookup = h_counters[1]; stats->n_nee_step = h_counters[2];
            stats->kernel_ms = kernel_ms; stats->kernel_launches = launches; stats->cancelled = cancelled ? 1 : 0; stats->timed_out = timed_out ? 1 : 0; stats->kernel_variant = last_variant;
            stats->calibration_ms = calibration_ms; stats->calibration_launches = calibration_launches; stats->textured = instanced ? 2 : textured ? 1 : 0;
            stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    } catch (...) { (void) hipStreamSynchronize(stream); throw; }     // nothing of this render may still be using the cached buffers
#endif
    API_CATCH
}

int mts_render(mts_scene *scene, const mts_render_opts *opts, float *film, mts_stats *stats) { return mts_render_sensor(scene, 0, opts, film, stats); }

// mts_sample, mts_sample_spectral and mts_ray_intersect read hs.scene as it is: sensor 0's seed and medium, whatever sensors were added
int mts_sample(mts_scene *scene, int32_t n, uint64_t seed_offset, const float *ox, const float *oy, const float *oz,
               const float *dx, const float *dy, const float *dz, float *out_rgb, uint8_t *out_valid) {
    API_TRY
    if (!scene || n < 0) throw std::runtime_error("mts_sample: invalid argument");
    if (n == 0) return 0;
    HostScene &hs = *scene->hs;
    std::lock_guard<std::mutex> guard(scene->render_mutex);         // not while an update rewrites the scene
    if (hs.integrator.spectral) throw std::runtime_error("mts_sample: the scene was built for the spectral variant (use mts_sample_spectral: the rays carry wavelengths)");
#if defined(MTSAMD_HOST_ONLY)
    HOST_ONLY_STOP("mts_sample");
#else
    HIP_CHECK(hipSetDevice(hs.device));
    DeviceBuffer<float> d_rays((size_t) 6 * n), d_rgb((size_t) 3 * n);
    DeviceBuffer<uint8_t> d_valid((size_t) n);
    const float *rows[6] = { ox, oy, oz, dx, dy, dz };
    for (int r = 0; r < 6; ++r) HIP_CHECK(hipMemcpy(d_rays.p + (size_t) r * n, rows[r], (size_t) n * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(launch_sample(hs.scene, n, seed_offset, d_rays.p, d_rgb.p, d_valid.p, nullptr));
    HIP_CHECK(hipMemcpy(out_rgb, d_rgb.p, (size_t) 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_valid, d_valid.p, (size_t) n, hipMemcpyDeviceToHost));
#endif
    API_CATCH
}

int mts_sample_spectral(mts_scene *scene, int32_t n, uint64_t seed_offset, const float *ox, const float *oy, const float *oz,
                        const float *dx, const float *dy, const float *dz, const float *wavelengths, float *out_spec, uint8_t *out_valid) {
    API_TRY
    if (!scene || n < 0) throw std::runtime_error("mts_sample_spectral: invalid argument");
    if (n == 0) return 0;
    if (!ox || !oy || !oz || !dx || !dy || !dz || !wavelengths || !out_spec || !out_valid) throw std::runtime_error("mts_sample_spectral: null array");
    HostScene &hs = *scene->hs;
    std::lock_guard<std::mutex> guard(scene->render_mutex);         // not while an update rewrites the scene
    if (!hs.integrator.spectral) throw std::runtime_error("mts_sample_spectral: the scene was built for an rgb / mono variant (use mts_sample)");
#if defined(MTSAMD_HOST_ONLY)
    HOST_ONLY_STOP("mts_sample_spectral");
#else
    HIP_CHECK(hipSetDevice(hs.device));
    DeviceBuffer<float> d_rays((size_t) 6 * n), d_wl((size_t) 4 * n), d_spec((size_t) 4 * n);
    DeviceBuffer<uint8_t> d_valid((size_t) n);
    const float *rows[6] = { ox, oy, oz, dx, dy, dz };
    for (int r = 0; r < 6; ++r) HIP_CHECK(hipMemcpy(d_rays.p + (size_t) r * n, rows[r], (size_t) n * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_wl.p, wavelengths, (size_t) 4 * n * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(launch_sample_spectral(hs.scene, n, seed_offset, d_rays.p, d_wl.p, d_spec.p, d_valid.p, nullptr));
    HIP_CHECK(hipMemcpy(out_spec, d_spec.p, (size_t) 4 * n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_valid, d_valid.p, (size_t) n, hipMemcpyDeviceToHost));
#endif
    API_CATCH
}

int mts_sample_tea(int device, int32_t n, const uint32_t *v0, const uint32_t *v1, int32_t rounds, uint32_t *out32, uint64_t *out64, float *out_float32) {
    API_TRY
    if (n < 0 || !v0 || !v1 || !out32 || !out64 || !out_float32) throw std::runtime_error("mts_sample_tea: invalid argument");
    if (n == 0) return 0;
#if defined(MTSAMD_HOST_ONLY)
    HOST_ONLY_STOP("mts_sample_tea");
#else
    HIP_CHECK(hipSetDevice(device));
    DeviceBuffer<uint32_t> d0(n), d1(n), o32(n); DeviceBuffer<uint64_t> o64(n); DeviceBuffer<float> of(n);
    HIP_CHECK(hipMemcpy(d0.p, v0, (size_t) n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d1.p, v1, (size_t) n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(launch_tea(n, d0.p, d1.p, rounds, o32.p, o64.p, of.p, nullptr));
    HIP_CHECK(hipMemcpy(out32, o32.p, (size_t) n * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(out64, o64.p, (size_t) n * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_float32, of.p, (size_t) n * 4, hipMemcpyDeviceToHost));
#endif
    API_CATCH
}

int mts_wavefront_sampler(int device, int32_t lanes, uint64_t seed_value, int32_t count, float *out) {
    API_TRY
    if (lanes < 0 || count < 0 || !out) throw std::runtime_error("mts_wavefront_sampler: invalid argument");
    if (lanes == 0 || count == 0) return 0;
#if defined(MTSAMD_HOST_ONLY)
    HOST_ONLY_STOP("mts_wavefront_sampler");
#else
    HIP_CHECK(hipSetDevice(device));
    DeviceBuffer<float> d((size_t) lanes * count);
    HIP_CHECK(launch_wavefront_sampler(lanes, seed_value, count, d.p, nullptr));
    HIP_CHECK(hipMemcpy(out, d.p, (size_t) lanes * count * 4, hipMemcpyDeviceToHost));
#endif
    API_CATCH
}

int mts_ray_intersect(mts_scene *scene, int32_t n, const float *o, const float *d, const float *mint, const float *maxt,
                      float *out_t, int32_t *out_shape, int32_t *out_prim, float *out_p, float *out_n) {
    API_TRY
    if (!scene || n < 0) throw std::runtime_error("mts_ray_intersect: invalid argument");
    if (n == 0) return 0;
    HostScene &hs = *scene->hs; (void) hs;
    std::lock_guard<std::mutex> guard(scene->render_mutex);         // not while an update rewrites the scene
#if defined(MTSAMD_HOST_ONLY)
    HOST_ONLY_STOP("mts_ray_intersect");
#else
    HIP_CHECK(hipSetDevice(hs.device));
    DeviceBuffer<float> d_o((size_t) 3 * n), d_d((size_t) 3 * n), d_mint(n), d_maxt(n), d_t(n), d_p((size_t) 3 * n), d_n((size_t) 3 * n);
    DeviceBuffer<int32_t> d_shape(n), d_prim(n);
    HIP_CHECK(hipMemcpy(d_o.p, o, (size_t) 3 * n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d_d.p, d, (size_t) 3 * n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_mint.p, mint, (size_t) n * 4, hipMemcpyHostToDevice)); HIP_CHECK(hipMemcpy(d_maxt.p, maxt, (size_t) n * 4, hipMemcpyHostToDevice));
    HIP_CHECK(launch_intersect(hs.scene, n, d_o.p, d_d.p, d_mint.p, d_maxt.p, d_t.p, d_shape.p, d_prim.p, d_p.p, d_n.p, nullptr));
    HIP_CHECK(hipMemcpy(out_t, d_t.p, (size_t) n * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(out_shape, d_shape.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_prim, d_prim.p, (size_t) n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out_p, d_p.p, (size_t) 3 * n * 4, hipMemcpyDeviceToHost)); HIP_CHECK(hipMemcpy(out_n, d_n.p, (size_t) 3 * n * 4, hipMemcpyDeviceToHost));
#endif
    API_CATCH
}

} // extern "C"
