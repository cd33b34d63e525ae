// instance_host_asan.cpp -- stand-alone driver for the host side of MTS_SHAPE_SHAPEGROUP / MTS_SHAPE_INSTANCE under AddressSanitizer /
// UBSan (tests/test_instance.py::test_host_side_under_sanitizers builds it together with csrc/scene_host.cpp and csrc/capi.cpp in
// host-only mode, -DMTSAMD_HOST_ONLY: no device code, no upload).  It hands mts_scene_create a valid instanced description -- host
// validation, scene construction, the two levels' BVHs under whatever MTSAMD_BVH_THRESHOLD the test sets -- and each corrupted one,
// checks status and message, and runs digest, geometry query and update plan.  Exit status 0 and the last line say that all passed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/mtsamd.h"

extern "C" int mts_debug_desc_digest(const mts_scene_desc *desc, uint64_t out[8]);
extern "C" int mts_debug_scene_geometry(const mts_scene_desc *desc, int32_t *counts, float *bbox);
extern "C" int mts_debug_update_plan(const mts_scene_desc *before, const mts_scene_desc *after, const mts_dirty *dirty, int32_t n, int32_t *traits, int32_t *kernel_variant);

static mts_transform translate(float x, float y, float z, float sx = 1.f) {
    mts_transform t; memset(&t, 0, sizeof(t));
    for (int i = 0; i < 3; ++i) { t.matrix[i * 5] = sx; t.inverse_transpose[i * 5] = 1.f / sx; }
    t.matrix[15] = t.inverse_transpose[15] = 1.f;
    t.matrix[3] = x; t.matrix[7] = y; t.matrix[11] = z;
    t.inverse_transpose[12] = -x / sx; t.inverse_transpose[13] = -y / sx; t.inverse_transpose[14] = -z / sx;
    return t;
}

// shapes: 0 a rectangle of the scene, 1 a group of 2, 3, 4 (a 3 x 3 grid mesh of 18 triangles, a sphere, a disk), 5 .. 10 six instances of
// it (one standing BEFORE nothing: the group precedes them all), 11 an empty group, 12 an instance of the empty group, 13 a rectangle
struct Scene {
    std::vector<float> positions, texcoords; std::vector<uint32_t> faces;
    std::vector<mts_shape> shapes; mts_bsdf bsdf; mts_medium medium; mts_volume volume; mts_phase phase; mts_emitter emitter;
    mts_scene_desc desc;

    static mts_shape shape(int type, mts_transform t) {
        mts_shape s; memset(&s, 0, sizeof(s)); s.type = type; s.to_world = t; s.radius = 1.f;
        s.bsdf = s.interior_medium = s.exterior_medium = s.emitter = -1;
        return s;
    }
    Scene() {
        for (int j = 0; j < 4; ++j) for (int i = 0; i < 4; ++i) { positions.insert(positions.end(), { i / 3.f - .5f, j / 3.f - .5f, .1f * (float) ((i + j) & 1) }); texcoords.insert(texcoords.end(), { i / 3.f, j / 3.f }); }
        for (uint32_t j = 0; j < 3; ++j) for (uint32_t i = 0; i < 3; ++i) { const uint32_t a = j * 4 + i; faces.insert(faces.end(), { a, a + 1, a + 5, a, a + 5, a + 4 }); }
        shapes.push_back(shape(MTS_SHAPE_RECTANGLE, translate(0, 0, 0, 8.f)));
        mts_shape g = shape(MTS_SHAPE_SHAPEGROUP, translate(0, 0, 0)); g.face_count = 3; shapes.push_back(g);
        mts_shape m = shape(MTS_SHAPE_MESH, translate(0, 0, .5f));
        m.vertex_positions = positions.data(); m.vertex_texcoords = texcoords.data(); m.faces = faces.data(); m.vertex_count = 16; m.face_count = 18; m.bsdf = 0;
        shapes.push_back(m);
        mts_shape sp = shape(MTS_SHAPE_SPHERE, translate(0, 0, 1.f)); sp.radius = .25f; shapes.push_back(sp);
        shapes.push_back(shape(MTS_SHAPE_DISK, translate(0, 0, .2f, .5f)));
        for (int k = 0; k < 6; ++k) { mts_shape in = shape(MTS_SHAPE_INSTANCE, translate((float) k - 2.5f, .3f * (float) k, 1.f + .2f * (float) k, 1.f + .25f * (float) k)); in.vertex_count = 1; shapes.push_back(in); }
        mts_shape e = shape(MTS_SHAPE_SHAPEGROUP, translate(0, 0, 0)); e.face_count = 0; shapes.push_back(e);
        mts_shape ie = shape(MTS_SHAPE_INSTANCE, translate(1, 1, 1)); ie.vertex_count = 11; shapes.push_back(ie);
        shapes.push_back(shape(MTS_SHAPE_RECTANGLE, translate(0, 0, 6.f, 2.f)));
        memset(&bsdf, 0, sizeof(bsdf)); bsdf.type = MTS_BSDF_DIFFUSE; bsdf.reflectance[0] = bsdf.reflectance[1] = bsdf.reflectance[2] = .4f;
        for (int k = 0; k < 6; ++k) bsdf.spectrum[k] = -1;
        memset(&volume, 0, sizeof(volume)); volume.type = MTS_VOLUME_CONST; volume.value[0] = volume.value[1] = volume.value[2] = 1.f; volume.to_world = translate(0, 0, 0); volume.value_spectrum = -1;
        memset(&medium, 0, sizeof(medium)); medium.type = MTS_MEDIUM_HOMOGENEOUS; medium.sigma_t_volume = medium.albedo_volume = 0; medium.scale = 1.f; medium.phase = 0;
        memset(&phase, 0, sizeof(phase)); phase.type = MTS_PHASE_ISOTROPIC; phase.child[0] = phase.child[1] = phase.weight_volume = -1;
        medium.sample_emitters = 1; medium.has_spectral_extinction = 1;
        memset(&emitter, 0, sizeof(emitter));
        emitter.type = MTS_EMITTER_DIRECTIONAL; emitter.to_world = translate(0, 0, 0); emitter.shape = -1; emitter.radiance_spectrum = -1;
        emitter.radiance[0] = emitter.radiance[1] = emitter.radiance[2] = 1.f;
        memset(&desc, 0, sizeof(desc));
        desc.abi_version = MTS_ABI_VERSION;
        mts_sensor &s = desc.sensor;
        s.type = MTS_SENSOR_PERSPECTIVE; s.to_world = translate(0, 0, 3.f);
        s.fov_x = 40.f; s.near_clip = 1e-2f; s.far_clip = 1e4f;
        s.film_width = s.film_height = s.crop_size[0] = s.crop_size[1] = 4;
        s.rfilter_type = MTS_RFILTER_BOX; s.rfilter_radius = .5f; s.sample_count = 2; s.medium = -1;
        desc.integrator.type = MTS_INTEGRATOR_PATH; desc.integrator.max_depth = -1; desc.integrator.rr_depth = 5;
        desc.integrator.samples_per_pass = -1; desc.integrator.timeout = -1.f;
        desc.bsdfs = &bsdf; desc.bsdf_count = 1;
        desc.shapes = shapes.data(); desc.shape_count = (int32_t) shapes.size(); desc.emitters = &emitter; desc.emitter_count = 1;
    }
    void with_medium() { desc.volumes = &volume; desc.volume_count = 1; desc.phases = &phase; desc.phase_count = 1; desc.media = &medium; desc.medium_count = 1; }
};

static int failures = 0, cases = 0;
static void expect(const char *name, const mts_scene_desc &d, const char *message) {
    mts_scene *h = nullptr;
    const int rc = mts_scene_create(&d, 0, &h);
    const std::string err = rc ? mts_last_error() : "";
    ++cases;
    const bool ok = message ? (rc != 0 && err.find(message) != std::string::npos) : rc == 0;
    if (!ok) { ++failures; printf("FAILED %s: rc %d, message \"%s\"\n", name, rc, err.c_str()); }
    if (h) mts_scene_destroy(h);
}

int main() {
    { Scene s; expect("valid", s.desc, nullptr); }
    { Scene s; s.shapes[5].vertex_count = 11; expect("valid, an instance of the empty group", s.desc, nullptr); }
    { Scene s; s.shapes[5].vertex_count = 0; expect("instance of a rectangle", s.desc, "is not a shapegroup"); }
    { Scene s; s.shapes[5].vertex_count = -1; expect("group index -1", s.desc, "is out of range"); }
    { Scene s; s.shapes[5].vertex_count = 14; expect("group index past the end", s.desc, "is out of range"); }
    { Scene s; s.shapes[5].vertex_count = 0x7fffffff; expect("group index INT_MAX", s.desc, "is out of range"); }
    { Scene s; s.shapes[1].face_count = 13; expect("members past the end", s.desc, "run past the end of the shape array"); }
    { Scene s; s.shapes[1].face_count = 0x7fffffff; expect("member count INT_MAX", s.desc, "run past the end of the shape array"); }
    { Scene s; s.shapes[1].face_count = -1; expect("member count -1", s.desc, "run past the end of the shape array"); }
    { Scene s; s.shapes[11].face_count = 2; expect("an instance among the members", s.desc, "Nested instancing is not permitted"); }
    { Scene s; s.shapes[3].type = MTS_SHAPE_SHAPEGROUP; s.shapes[3].face_count = 0; expect("a group among the members", s.desc, "Nested ShapeGroup is not permitted"); }
    { Scene s; s.shapes[3].emitter = 0; expect("an emitter on a member", s.desc, "Instancing of emitters is not supported"); }
    { Scene s; s.with_medium(); s.shapes[4].interior_medium = 0; expect("a medium on a member", s.desc, "\"interior\" medium"); }
    { Scene s; s.shapes[6].bsdf = 0; expect("a bsdf on an instance", s.desc, "must be -1"); }
    { Scene s; s.desc.integrator.moment = 1; expect("moment", s.desc, "not supported inside a moment integrator's scene"); }
    { Scene s; s.shapes[7].type = 7; expect("type 7", s.desc, "unknown shape type"); }
    {   // the geometry query: fourteen records, three primitives of the scene's own, seven instances, the group's twenty behind them
        Scene s; int32_t counts[6]; float box[6];
        ++cases;
        if (mts_debug_scene_geometry(&s.desc, counts, box) != 0 || counts[0] != 9 || counts[1] != 29 || counts[2] != 7 || counts[3] != 2 || !(box[0] <= -8.f && box[3] >= 8.f))
            { ++failures; printf("FAILED geometry: %s (%d %d %d %d)\n", mts_last_error(), counts[0], counts[1], counts[2], counts[3]); }
    }
    {   // the digest tells an instance's transform and a member's vertex
        Scene a, b, c; uint64_t da[8], db[8], dc[8];
        b.shapes[7].to_world = translate(0.f, 0.f, 2.5f);
        c.positions[5] += .01f;
        ++cases;
        if (mts_debug_desc_digest(&a.desc, da) != 0 || mts_debug_desc_digest(&b.desc, db) != 0 || mts_debug_desc_digest(&c.desc, dc) != 0 || da[6] == db[6] || da[6] == dc[6])
            { ++failures; printf("FAILED digest: %s\n", mts_last_error()); }
    }
    {   // update plan: the material of a member is rewritten; an instanced scene keeps no traits
        Scene a, b;
        b.bsdf.reflectance[0] = .9f;
        mts_dirty dirty[1] = { { MTS_OBJ_BSDF, 0, nullptr } };
        int32_t traits = -1, variant = -1;
        ++cases;
        if (mts_debug_update_plan(&a.desc, &b.desc, dirty, 1, &traits, &variant) != 0 || traits != 0) { ++failures; printf("FAILED update of a member's material: %s\n", mts_last_error()); }
    }
    printf("instance host sanitizer: %d cases, %d failed\n", cases, failures);
    return failures ? 1 : 0;
}
