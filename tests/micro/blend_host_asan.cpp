// blend_host_asan.cpp -- stand-alone driver for the host side of MTS_BSDF_BLEND under AddressSanitizer / UBSan
// (tests/test_blendbsdf.py::test_host_side_under_sanitizers builds it together with csrc/scene_host.cpp and csrc/capi.cpp in
// host-only mode, -DMTSAMD_HOST_ONLY: no device code, no upload).  It hands mts_scene_create a valid blend description and each
// corrupted one, checks status and message, and runs one update on the host scene.  Exit status 0 and the last line say that all passed.
#include <cmath>
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
    std::vector<mts_texture> textures;
    std::vector<int32_t> bsdf_textures;
    mts_shape shape; mts_emitter emitter;
    mts_scene_desc desc;
    float texels[4] = { 0.f, 1.f, .5f, .5f };

    static mts_bsdf bsdf(int type, float v) {
        mts_bsdf b; memset(&b, 0, sizeof(b)); b.type = type;
        for (int c = 0; c < 3; ++c) { b.reflectance[c] = v; b.rho_0[c] = v; b.k[c] = .6f; b.g[c] = -.2f; b.rho_c[c] = v; b.transmittance[c] = .25f; }
        for (int k = 0; k < 6; ++k) b.spectrum[k] = -1;
        return b;
    }
    // bsdfs: 0 diffuse, 1 rpv, 2 the blend of the two (weight 0.3), 3 null, 4 a second blend (of 0 and 1)
    explicit Scene(bool textured) {
        bsdfs = { bsdf(MTS_BSDF_DIFFUSE, .5f), bsdf(MTS_BSDF_RPV, .2f), bsdf(MTS_BSDF_BLEND, .3f), bsdf(MTS_BSDF_NULL, 0.f), bsdf(MTS_BSDF_BLEND, .6f) };
        bsdfs[2].spectrum[0] = 0; bsdfs[2].spectrum[1] = 1;
        bsdfs[4].spectrum[0] = 1; bsdfs[4].spectrum[1] = 0;
        memset(&shape, 0, sizeof(shape));
        shape.type = MTS_SHAPE_RECTANGLE; shape.to_world = identity(); shape.bsdf = 2;
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
        if (textured) {
            mts_texture t; memset(&t, 0, sizeof(t));
            t.type = MTS_TEXTURE_BITMAP; t.to_uv[0] = t.to_uv[4] = t.to_uv[8] = 1.f;
            t.data = texels; t.width = t.height = 2; t.channels = 1; t.filter_type = MTS_FILTER_NEAREST; t.wrap_mode = MTS_WRAP_REPEAT;
            textures.push_back(t);
            bsdf_textures.assign(6 * bsdfs.size(), -1);
            bsdf_textures[6 * 2] = 0;
        }
        link();
    }
    void link() {
        desc.bsdfs = bsdfs.data(); desc.bsdf_count = (int32_t) bsdfs.size();
        desc.shapes = &shape; desc.shape_count = 1; desc.emitters = &emitter; desc.emitter_count = 1;
        desc.textures = textures.empty() ? nullptr : textures.data(); desc.texture_count = (int32_t) textures.size();
        desc.bsdf_textures = bsdf_textures.empty() ? nullptr : bsdf_textures.data();
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
    for (int textured = 0; textured < 2; ++textured) {
        { Scene s(textured != 0); expect("valid", s.desc, nullptr); }
        { Scene s(textured != 0); s.shape.bsdf = 4; expect("valid, children behind and before", s.desc, nullptr); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[0] = -1; expect("child -1", s.desc, "index out of range"); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[1] = 5; expect("child past the end", s.desc, "index out of range"); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[1] = 0x7fffffff; expect("child INT_MAX", s.desc, "index out of range"); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[0] = 2; expect("child is the blend", s.desc, "the blend itself"); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[1] = 3; expect("null child", s.desc, "not supported by this backend"); }
        { Scene s(textured != 0); s.bsdfs[2].spectrum[0] = 4; expect("nested blend", s.desc, "nested blends are not supported by this backend"); }
        { Scene s(textured != 0); s.bsdfs[2].reflectance[0] = NAN; expect("NaN weight", s.desc, "not finite"); }
        { Scene s(textured != 0); s.bsdfs[2].reflectance[0] = INFINITY; expect("infinite weight", s.desc, "not finite"); }
        { Scene s(textured != 0); s.desc.integrator.moment = 1; expect("moment", s.desc, "moment"); }
        { Scene s(textured != 0); s.desc.integrator.spectral = 1; expect("spectral", s.desc, "spectral"); }
        { Scene s(textured != 0); s.bsdfs[2].type = 5; expect("type 5", s.desc, "unknown BSDF type"); }
    }
    {   // the weight's texture slot out of range
        Scene s(true); s.bsdf_textures[6 * 2] = 1; expect("texture slot", s.desc, "index out of range");
    }
    {   // update plan: a new weight is accepted, a new child refused by the field's name
        Scene a(true), b(true);
        b.bsdfs[2].reflectance[0] = .4f;
        mts_dirty dirty = { MTS_OBJ_BSDF, 2, nullptr };
        int32_t traits = -1, variant = -1;
        ++cases;
        if (mts_debug_update_plan(&a.desc, &b.desc, &dirty, 1, &traits, &variant) != 0) { ++failures; printf("FAILED update of the weight: %s\n", mts_last_error()); }
        b.bsdfs[2].spectrum[1] = 0;
        ++cases;
        if (mts_debug_update_plan(&a.desc, &b.desc, &dirty, 1, &traits, &variant) == 0 || !strstr(mts_last_error(), "spectrum[1]")) { ++failures; printf("FAILED update of a child: %s\n", mts_last_error()); }
        uint64_t da[8], db[8];
        ++cases;
        if (mts_debug_desc_digest(&a.desc, da) != 0 || mts_debug_desc_digest(&b.desc, db) != 0 || da[0] == db[0]) { ++failures; printf("FAILED digest\n"); }
    }
    printf("blend host sanitizer: %d cases, %d failed\n", cases, failures);
    return failures ? 1 : 0;
}
