// twosided_host_asan.cpp -- stand-alone driver for the host side of MTS_BSDF_TWOSIDED under AddressSanitizer / UBSan
// (tests/test_twosided.py::test_host_side_under_sanitizers builds it together with csrc/scene_host.cpp and csrc/capi.cpp in
// host-only mode, -DMTSAMD_HOST_ONLY: no device code, no upload).  It hands mts_scene_create a valid description and each corrupted
// one, checks status and message, and runs the update plan.  Exit status 0 and the last line say that all passed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mtsamd.h"

extern "C" int mts_debug_desc_digest(const mts_scene_desc *desc, uint64_t out[8]);
extern "C" int mts_debug_update_plan(const mts_scene_desc *before, const mts_scene_desc *after, const mts_dirty *dirty, int32_t n, int32_t *traits, int32_t *kernel_variant);

static mts_transform identity() {
    mts_transform t; memset(&t, 0, sizeof(t));
    for (int i = 0; i < 4; ++i) t.matrix[i * 5] = t.inverse_transpose[i * 5] = 1.f;
    return t;
}

struct Scene {
    std::vector<mts_bsdf> bsdfs;
    mts_shape shape; mts_emitter emitter;
    mts_scene_desc desc;

    static mts_bsdf bsdf(int type, float v) {
        mts_bsdf b; memset(&b, 0, sizeof(b)); b.type = type;
        for (int c = 0; c < 3; ++c) { b.reflectance[c] = v; b.rho_0[c] = v; b.k[c] = .6f; b.g[c] = -.2f; b.rho_c[c] = v; b.transmittance[c] = .25f; }
        for (int k = 0; k < 6; ++k) b.spectrum[k] = -1;
        return b;
    }
    // bsdfs: 0 a twosided of 1 and 2 (children behind it), 1 diffuse, 2 rpv, 3 a blend of 1 and 2, 4 a twosided of 3 alone (its child
    // before it), 5 null, 6 bilambertian, 7 a second blend of 1 and 2 that no record uses (behind every adapter)
    Scene() {
        bsdfs = { bsdf(MTS_BSDF_TWOSIDED, 0.f), bsdf(MTS_BSDF_DIFFUSE, .5f), bsdf(MTS_BSDF_RPV, .2f), bsdf(MTS_BSDF_BLEND, .3f), bsdf(MTS_BSDF_TWOSIDED, 0.f),
                  bsdf(MTS_BSDF_NULL, 0.f), bsdf(MTS_BSDF_BILAMBERTIAN, .4f), bsdf(MTS_BSDF_BLEND, .5f) };
        bsdfs[0].spectrum[0] = 1; bsdfs[0].spectrum[1] = 2;
        bsdfs[3].spectrum[0] = 1; bsdfs[3].spectrum[1] = 2;
        bsdfs[4].spectrum[0] = 3; bsdfs[4].spectrum[1] = 3;
        bsdfs[7].spectrum[0] = 1; bsdfs[7].spectrum[1] = 2;
        memset(&shape, 0, sizeof(shape));
        shape.type = MTS_SHAPE_RECTANGLE; shape.to_world = identity(); shape.bsdf = 0;
        shape.interior_medium = shape.exterior_medium = shape.emitter = -1;
        memset(&emitter, 0, sizeof(emitter));
        emitter.type = MTS_EMITTER_DIRECTIONAL; emitter.to_world = identity(); emitter.shape = -1; emitter.radiance_spectrum = -1;
        emitter.radiance[0] = emitter.radiance[1] = emitter.radiance[2] = 1.f;
        memset(&desc, 0, sizeof(desc));
        desc.abi_version = MTS_ABI_VERSION;
        mts_sensor &s = desc.sensor;
        s.type = MTS_SENSOR_PERSPECTIVE; s.to_world = identity(); s.to_world.matrix[11] = 3.f; s.to_world.inverse_transpose[14] = -3.f;
        s.fov_x = 40.f; s.near_clip = 1e-2f; s.far_clip = 1e4f;
        s.film_width = s.film_height = s.crop_size[0] = s.crop_size[1] = 4;
        s.rfilter_type = MTS_RFILTER_BOX; s.rfilter_radius = .5f; s.sample_count = 2; s.medium = -1;
        desc.integrator.type = MTS_INTEGRATOR_PATH; desc.integrator.max_depth = -1; desc.integrator.rr_depth = 5;
        desc.integrator.samples_per_pass = -1; desc.integrator.timeout = -1.f;
        desc.bsdfs = bsdfs.data(); desc.bsdf_count = (int32_t) bsdfs.size();
        desc.shapes = &shape; desc.shape_count = 1; desc.emitters = &emitter; desc.emitter_count = 1;
    }
};

static int failures = 0, cases = 0;
static void expect(const char *name, const mts_scene_desc &d, const char *message) {
    mts_scene *h = nullptr;
    const int rc = mts_scene_create(&d, 0, &h);
    const std::string err = rc ? mts_last_error() : "";
    ++cases;
    const bool ok = message ? (rc != 0 && err.find(message) != std::string::npos && (err.find("bsdf") != std::string::npos || err.find("BSDF") != std::string::npos)) : rc == 0;
    if (!ok) { ++failures; printf("FAILED %s: rc %d, message \"%s\"\n", name, rc, err.c_str()); }
    if (h) mts_scene_destroy(h);
}

int main() {
    const char *transmission = "twosided: Only materials without a transmission component can be nested!";
    { Scene s; expect("valid", s.desc, nullptr); }
    { Scene s; s.shape.bsdf = 4; expect("valid, one blend child before the adapter", s.desc, nullptr); }
    { Scene s; s.bsdfs[0].spectrum[1] = 1; expect("valid, one child under both names", s.desc, nullptr); }
    { Scene s; s.bsdfs[0].spectrum[0] = -1; expect("child -1", s.desc, "index out of range"); }
    { Scene s; s.bsdfs[0].spectrum[1] = 8; expect("child past the end", s.desc, "index out of range"); }
    { Scene s; s.bsdfs[0].spectrum[1] = 0x7fffffff; expect("child INT_MAX", s.desc, "index out of range"); }
    { Scene s; s.bsdfs[0].spectrum[0] = (int32_t) 0x80000000u; expect("child INT_MIN", s.desc, "index out of range"); }
    { Scene s; s.bsdfs[0].spectrum[0] = 0; expect("child is the adapter", s.desc, "is the twosided itself"); }
    { Scene s; s.bsdfs[0].spectrum[1] = 4; expect("nested adapter", s.desc, "nested twosided adapters are not supported by this backend"); }
    { Scene s; s.bsdfs[3].spectrum[0] = 0; expect("adapter inside a blend", s.desc, "a twosided inside a blend is not supported by this backend"); }
    { Scene s; s.bsdfs[0].spectrum[1] = 5; expect("null child", s.desc, transmission); }
    { Scene s; s.bsdfs[0].spectrum[0] = 6; expect("bilambertian child", s.desc, transmission); }
    { Scene s; s.bsdfs[7].spectrum[1] = 6; s.bsdfs[0].spectrum[1] = 7; expect("transmissive blend behind the adapter", s.desc, transmission); }
    { Scene s; s.bsdfs[3].spectrum[1] = 6; expect("transmissive blend before the adapter", s.desc, transmission); }
    { Scene s; s.desc.integrator.moment = 1; expect("moment", s.desc, "twosided is not supported inside a moment integrator's scene"); }
    { Scene s; s.desc.integrator.spectral = 1; expect("spectral", s.desc, "twosided is not supported in the spectral variant"); }
    { Scene s; s.bsdfs[0].type = 5; expect("type 5", s.desc, "unknown BSDF type"); }
    { Scene s; s.bsdfs[0].type = 7; expect("type 7", s.desc, "unknown BSDF type"); }
    {   // update plan: a child's colour is accepted, a new child index refused by the field's name, the digest tells the children
        Scene a, b;
        b.bsdfs[1].reflectance[0] = .9f;
        mts_dirty dirty[2] = { { MTS_OBJ_BSDF, 1, nullptr }, { MTS_OBJ_BSDF, 0, nullptr } };
        int32_t traits = -1, variant = -1;
        ++cases;
        if (mts_debug_update_plan(&a.desc, &b.desc, dirty, 2, &traits, &variant) != 0 || traits != 0) { ++failures; printf("FAILED update of a child's colour: %s\n", mts_last_error()); }
        b.bsdfs[0].spectrum[1] = 1;
        ++cases;
        if (mts_debug_update_plan(&a.desc, &b.desc, dirty, 2, &traits, &variant) == 0 || !strstr(mts_last_error(), "spectrum[1] (brdf_1)")) { ++failures; printf("FAILED update of a child index: %s\n", mts_last_error()); }
        uint64_t da[8], db[8];
        ++cases;
        if (mts_debug_desc_digest(&a.desc, da) != 0 || mts_debug_desc_digest(&b.desc, db) != 0 || da[0] == db[0]) { ++failures; printf("FAILED digest\n"); }
    }
    printf("twosided host sanitizer: %d cases, %d failed\n", cases, failures);
    return failures ? 1 : 0;
}
