// sensors_host_asan.cpp -- stand-alone driver for the host side of mts_scene_add_sensor / mts_scene_sensor_count / mts_render_sensor
// under AddressSanitizer / UBSan (tests/test_sensors.py::test_host_side_under_sanitizers builds it together with csrc/scene_host.cpp
// and csrc/capi.cpp in host-only mode, -DMTSAMD_HOST_ONLY: no device code, no upload).  It creates a scene, adds three sensors -- one
// of them an mdistant whose matrix array is freed right after the call --, tries every add the library refuses and checks that the
// count stays, runs one mts_scene_update, takes the handle's digest and destroys the scene.  Exit status 0 and the last line say
// that all passed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mtsamd.h"

extern "C" int mts_debug_scene_digest(mts_scene *scene, uint64_t out[8]);
extern "C" int mts_debug_desc_digest(const mts_scene_desc *desc, uint64_t out[8]);
extern "C" int mts_debug_sensor_choice(const mts_scene_desc *desc, const mts_sensor *extra, int32_t n_extra, int32_t sensor, int32_t *traits, int32_t *kernel_variant);

static mts_transform translate(float x, float y, float z, float sx = 1.f) {
    mts_transform t; memset(&t, 0, sizeof(t));
    for (int i = 0; i < 3; ++i) { t.matrix[i * 5] = sx; t.inverse_transpose[i * 5] = 1.f / sx; }
    t.matrix[15] = t.inverse_transpose[15] = 1.f;
    t.matrix[3] = x; t.matrix[7] = y; t.matrix[11] = z;
    t.inverse_transpose[12] = -x / sx; t.inverse_transpose[13] = -y / sx; t.inverse_transpose[14] = -z / sx;
    return t;
}

static mts_sensor perspective(int w, int h) {
    mts_sensor s; memset(&s, 0, sizeof(s));
    s.type = MTS_SENSOR_PERSPECTIVE; s.to_world = translate(0, 0, 3.f);
    s.fov_x = 40.f; s.near_clip = 1e-2f; s.far_clip = 1e4f;
    s.film_width = s.crop_size[0] = w; s.film_height = s.crop_size[1] = h;
    s.rfilter_type = MTS_RFILTER_BOX; s.rfilter_radius = .5f; s.sample_count = 2; s.medium = -1;
    return s;
}

// a rectangle, a homogeneous medium the sensors may sit in, one emitter
struct Scene {
    mts_shape shape; mts_bsdf bsdf; mts_medium medium; mts_volume volume; mts_phase phase; mts_emitter emitter;
    mts_scene_desc desc;
    Scene() {
        memset(&shape, 0, sizeof(shape)); shape.type = MTS_SHAPE_RECTANGLE; shape.to_world = translate(0, 0, 0, 4.f); shape.radius = 1.f;
        shape.bsdf = 0; shape.interior_medium = shape.exterior_medium = shape.emitter = -1;
        memset(&bsdf, 0, sizeof(bsdf)); bsdf.type = MTS_BSDF_DIFFUSE; bsdf.reflectance[0] = bsdf.reflectance[1] = bsdf.reflectance[2] = .4f;
        for (int k = 0; k < 6; ++k) bsdf.spectrum[k] = -1;
        memset(&volume, 0, sizeof(volume)); volume.type = MTS_VOLUME_CONST; volume.value[0] = volume.value[1] = volume.value[2] = 1.f; volume.to_world = translate(0, 0, 0); volume.value_spectrum = -1;
        memset(&medium, 0, sizeof(medium)); medium.type = MTS_MEDIUM_HOMOGENEOUS; medium.sigma_t_volume = medium.albedo_volume = 0; medium.scale = 1.f; medium.phase = 0;
        medium.sample_emitters = 1; medium.has_spectral_extinction = 1;
        memset(&phase, 0, sizeof(phase)); phase.type = MTS_PHASE_ISOTROPIC; phase.child[0] = phase.child[1] = phase.weight_volume = -1;
        memset(&emitter, 0, sizeof(emitter));
        emitter.type = MTS_EMITTER_DIRECTIONAL; emitter.to_world = translate(0, 0, 0); emitter.shape = -1; emitter.radiance_spectrum = -1;
        emitter.radiance[0] = emitter.radiance[1] = emitter.radiance[2] = 1.f;
        memset(&desc, 0, sizeof(desc));
        desc.abi_version = MTS_ABI_VERSION;
        desc.sensor = perspective(4, 4);
        desc.integrator.type = MTS_INTEGRATOR_VOLPATH; desc.integrator.max_depth = -1; desc.integrator.rr_depth = 5;
        desc.integrator.samples_per_pass = 1; desc.integrator.timeout = -1.f;
        desc.volumes = &volume; desc.volume_count = 1; desc.phases = &phase; desc.phase_count = 1; desc.media = &medium; desc.medium_count = 1;
        desc.bsdfs = &bsdf; desc.bsdf_count = 1; desc.shapes = &shape; desc.shape_count = 1; desc.emitters = &emitter; desc.emitter_count = 1;
    }
};

static int failures = 0, cases = 0;
static void check(const char *name, bool ok) {
    ++cases;
    if (!ok) { ++failures; printf("FAILED %s: \"%s\"\n", name, mts_last_error()); }
}
static int32_t count_of(mts_scene *h) { int32_t n = -1; return mts_scene_sensor_count(h, &n) == 0 ? n : -1; }
static bool says(const char *message) { return std::string(mts_last_error()).find(message) != std::string::npos; }
// an add the library must refuse: non-zero status, the message, the index untouched, the count as it was
static void refused(mts_scene *h, const char *name, const mts_sensor *s, const char *message) {
    const int32_t before = count_of(h);
    int32_t index = -7;
    const int rc = mts_scene_add_sensor(h, s, &index);
    const std::string err = rc ? mts_last_error() : "";
    ++cases;
    if (!(rc != 0 && err.find(message) != std::string::npos && index == -7 && count_of(h) == before)) {
        ++failures; printf("FAILED refusal %s: rc %d, message \"%s\", index %d, count %d -> %d\n", name, rc, err.c_str(), index, before, count_of(h));
    }
}

int main() {
    Scene sc;
    mts_scene *h = nullptr;
    check("create", mts_scene_create(&sc.desc, 0, &h) == 0 && h != nullptr);
    if (!h) { printf("sensors host sanitizer: no scene\n"); return 1; }
    check("one sensor to begin with", count_of(h) == 1);
    uint64_t fresh[8], lone[8];
    check("digest of the handle", mts_debug_scene_digest(h, fresh) == 0);
    check("digest of the description", mts_debug_desc_digest(&sc.desc, lone) == 0 && memcmp(fresh, lone, sizeof(fresh)) == 0);

    int32_t index = -1;
    {   // 1: a perspective of another film size, in the scene's medium
        mts_sensor s = perspective(9, 5); s.crop_offset[0] = 2; s.crop_offset[1] = 1; s.crop_size[0] = 5; s.crop_size[1] = 3; s.medium = 0;
        s.rfilter_type = MTS_RFILTER_GAUSSIAN; s.rfilter_stddev = .5f;
        check("add perspective", mts_scene_add_sensor(h, &s, &index) == 0 && index == 1 && count_of(h) == 2);
    }
    {   // 2: an mdistant whose matrices live on the heap and are gone right after the call
        const int n = 5;
        float *mats = new float[16 * n];
        for (int i = 0; i < n; ++i) { const mts_transform t = translate(.1f * (float) i, 0, 0); memcpy(mats + 16 * i, t.matrix, 64); }
        mts_sensor s = perspective(n, 1); s.type = MTS_SENSOR_MDISTANT; s.to_world = translate(0, 0, 0);
        s.multi_transforms = mats; s.multi_count = n; s.distant_target_type = MTS_DISTANT_TARGET_POINT; s.distant_target_point[2] = .5f;
        const int rc = mts_scene_add_sensor(h, &s, &index);
        memset(mats, 0xff, 16 * n * sizeof(float)); delete[] mats;
        check("add mdistant", rc == 0 && index == 2 && count_of(h) == 3);
    }
    {   // 3: a distant sensor that aims at a sphere (no index asked for)
        mts_sensor s = perspective(6, 1); s.type = MTS_SENSOR_DISTANT; s.distant_target_type = MTS_DISTANT_TARGET_SHAPE;
        mts_shape &t = s.distant_target_shape; t.type = MTS_SHAPE_SPHERE; t.to_world = translate(0, 0, 0); t.radius = .75f; t.center[2] = 1.f;
        t.bsdf = t.interior_medium = t.exterior_medium = t.emitter = -1;
        check("add distant", mts_scene_add_sensor(h, &s, nullptr) == 0 && count_of(h) == 4);
    }
    uint64_t four[8];          // the added sensors enter the header slot [5] and the table slot [7], nothing else
    check("digest with four sensors", mts_debug_scene_digest(h, four) == 0 && four[5] != fresh[5] && four[7] != fresh[7] && memcmp(four, fresh, 5 * sizeof(uint64_t)) == 0 && four[6] == fresh[6]);

    // ---- every add the library refuses; the count stays at four
    refused(h, "NULL sensor", nullptr, "sensor is NULL");
    { mts_sensor s = perspective(4, 4); s.medium = 1; refused(h, "medium past the end", &s, "index out of range: sensor medium"); }
    { mts_sensor s = perspective(4, 4); s.medium = 0x7fffffff; refused(h, "medium INT_MAX", &s, "index out of range: sensor medium"); }
    { mts_sensor s = perspective(4, 4); s.crop_size[0] = 5; refused(h, "crop window", &s, "film: invalid size / crop window"); }
    { mts_sensor s = perspective(4, 4); s.sample_count = 0; refused(h, "sample_count 0", &s, "sample_count must be positive"); }
    { mts_sensor s = perspective(4, 4); s.type = 9; refused(h, "type 9", &s, "unknown sensor type"); }
    { mts_sensor s = perspective(4, 4); s.rfilter_type = 5; refused(h, "filter 5", &s, "unknown reconstruction filter"); }
    {   // mradiancemeter: the film must be [count, 1]
        std::vector<float> mats(32, 0.f);
        mts_sensor s = perspective(3, 1); s.type = MTS_SENSOR_MRADIANCEMETER; s.multi_transforms = mats.data(); s.multi_count = 2;
        refused(h, "mradiancemeter film", &s, "Film size must be [sensor_count, 1].");
        s.multi_transforms = nullptr; s.film_width = s.crop_size[0] = 2;
        refused(h, "mradiancemeter without matrices", &s, "no sub-sensors given");
    }
    { mts_sensor s = perspective(4, 4); s.sampler_wavefront = 1; refused(h, "wavefront under samples_per_pass 1", &s, "samples_per_pass must cover the whole sample_count"); }
    {   // a target shape the backend has not got
        mts_sensor s = perspective(6, 1); s.type = MTS_SENSOR_DISTANT; s.distant_target_type = MTS_DISTANT_TARGET_SHAPE; s.distant_target_shape.type = MTS_SHAPE_CUBE;
        refused(h, "cube target", &s, "must be a rectangle, a disk or a sphere");
    }
    check("still four", count_of(h) == 4);
    check("count: NULL arguments", mts_scene_sensor_count(h, nullptr) != 0 && mts_scene_sensor_count(nullptr, &index) != 0);
    check("add: NULL scene", mts_scene_add_sensor(nullptr, &sc.desc.sensor, &index) != 0);

    {   // rendering: an index outside [0, count) is refused by name; inside, the host-only build validates and stops before the device
        float film[9 * 5 * 5];
        mts_render_opts o; memset(&o, 0, sizeof(o)); o.shard_count = 1;
        check("render sensor 4", mts_render_sensor(h, 4, &o, film, nullptr) != 0 && says("sensor index 4 is out of range (the scene has 4 sensors)"));
        check("render sensor -1", mts_render_sensor(h, -1, &o, film, nullptr) != 0 && says("out of range"));
        for (int32_t k = 0; k < 4; ++k) check("render stops at the device", mts_render_sensor(h, k, &o, film, nullptr) != 0 && says("host-only build"));
        o.film_capacity = 5 * 3 * 5 - 1;                  // sensor 1's film is 5 x 3 x 5 floats, sensor 0's 4 x 4 x 5
        check("capacity of sensor 1", mts_render_sensor(h, 1, &o, film, nullptr) != 0 && says("this scene writes 75"));
        check("mts_render is sensor 0", mts_render(h, &o, film, nullptr) != 0 && says("this scene writes 80"));
    }
    {   // one update: the BSDF's reflectance; the sensors stay, the record slot of the digest moves
        sc.bsdf.reflectance[0] = .9f;
        mts_dirty dirty[1] = { { MTS_OBJ_BSDF, 0, nullptr } };
        uint64_t after[8];
        check("update", mts_scene_update(h, &sc.desc, dirty, 1, nullptr) == 0);
        check("digest after the update", mts_debug_scene_digest(h, after) == 0 && after[0] != four[0] && after[5] == four[5] && after[7] == four[7] && count_of(h) == 4);
    }
    {   // the debug entry runs the same adds on a description
        mts_sensor extra[2] = { perspective(8, 8), perspective(6, 1) };
        extra[1].type = MTS_SENSOR_DISTANT; extra[1].distant_target_type = MTS_DISTANT_TARGET_SHAPE;
        mts_shape &t = extra[1].distant_target_shape; t.type = MTS_SHAPE_SPHERE; t.to_world = translate(0, 0, 0); t.radius = .75f;
        int32_t traits[3] = { -1, -1, -1 }, variant = -1;
        bool ok = true;
        for (int32_t k = 0; k < 3; ++k) ok = ok && mts_debug_sensor_choice(&sc.desc, extra, 2, k, &traits[k], &variant) == 0;
        check("sensor choice", ok && traits[0] == traits[1] && traits[2] != traits[1]);          // the sphere target breaks the no-sphere promise
        check("sensor choice out of range", mts_debug_sensor_choice(&sc.desc, extra, 2, 3, &traits[0], &variant) != 0);
    }
    check("destroy", mts_scene_destroy(h) == 0);
    printf("sensors host sanitizer: %d cases, %d failed\n", cases, failures);
    return failures ? 1 : 0;
}
