// scene_host.cpp -- host side of libmtsamd.so: the "plugin constructors" that turn the C-ABI scene
// description into the flattened device scene (dscene.h), and its upload to HBM.
//
// Each block follows the constructor of the reference plugin it stands for (citations relative to
// /root/reference) with the same float arithmetic (explicit fma where the reference uses fmadd), so the
// constants the kernels read are the ones a scalar_rgb build would hold.
#include <cmath>
#include <cstddef>
#include <cstring>
#include <algorithm>
#include <map>
#include <set>
#include "scene_host.h"
#include "launch.h"
#include "cie_tables.h"

namespace mtsamd {

static void mat_transpose(const float *a, float *o) { for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) o[r * 4 + c] = a[c * 4 + r]; }
// enoki matrix product: result(r, j) = fma chain over k of a(r, k) * b(k, j)
static void mat_mul(const float *a, const float *b, float *o) {
    for (int j = 0; j < 4; ++j)
        for (int r = 0; r < 4; ++r) {
            float acc = a[r * 4 + 0] * b[0 * 4 + j];
            for (int k = 1; k < 4; ++k) acc = pm_fma(a[r * 4 + k], b[k * 4 + j], acc);
            o[r * 4 + j] = acc;
        }
}
static DXf xf_from_abi(const mts_transform &t) { DXf x; memcpy(x.m, t.matrix, 64); memcpy(x.it, t.inverse_transpose, 64); return x; }
static DXf xf_identity() { DXf x; memset(&x, 0, sizeof(x)); for (int i = 0; i < 4; ++i) x.m[i * 5] = x.it[i * 5] = 1.f; return x; }
static DXf xf_inverse(const DXf &x) { DXf r; mat_transpose(x.it, r.m); mat_transpose(x.m, r.it); return r; }          // transform.h:59-61
static DXf xf_mul(const DXf &a, const DXf &b) { DXf r; mat_mul(a.m, b.m, r.m); mat_mul(a.it, b.it, r.it); return r; }  // transform.h:53-56
static DXf xf_scale(F3 s) { DXf x = xf_identity(); x.m[0] = s.x; x.m[5] = s.y; x.m[10] = s.z; x.it[0] = 1.f / s.x; x.it[5] = 1.f / s.y; x.it[10] = 1.f / s.z; return x; }
static DXf xf_translate(F3 t) { DXf x = xf_identity(); x.m[3] = t.x; x.m[7] = t.y; x.m[11] = t.z; x.it[12] = -t.x; x.it[13] = -t.y; x.it[14] = -t.z; return x; }

static void bbox_reset(DBBox &b) { for (int i = 0; i < 3; ++i) { b.min[i] = INFINITY; b.max[i] = -INFINITY; } }
static void bbox_expand(DBBox &b, F3 p) {
    float v[3] = { p.x, p.y, p.z };
    for (int i = 0; i < 3; ++i) { b.min[i] = pm_min(b.min[i], v[i]); b.max[i] = pm_max(b.max[i], v[i]); }
}
static void bbox_expand(DBBox &b, const DBBox &o) { bbox_expand(b, f3(o.min)); bbox_expand(b, f3(o.max)); }
static void store3(float *d, F3 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }

static void check_index(int i, int n, const char *what, bool allow_none) {
    if (i < 0 && allow_none) return;
    if (i < 0 || i >= n) throw std::runtime_error(std::string("index out of range: ") + what);
}

// cube.cpp:43-67
static const float CUBE_VERTICES[24][3] = {
    { 1, -1, -1 }, { 1, -1, 1 }, { -1, -1, 1 }, { -1, -1, -1 }, { 1, 1, -1 }, { -1, 1, -1 }, { -1, 1, 1 }, { 1, 1, 1 },
    { 1, -1, -1 }, { 1, 1, -1 }, { 1, 1, 1 }, { 1, -1, 1 }, { 1, -1, 1 }, { 1, 1, 1 }, { -1, 1, 1 }, { -1, -1, 1 },
    { -1, -1, 1 }, { -1, 1, 1 }, { -1, 1, -1 }, { -1, -1, -1 }, { 1, 1, -1 }, { 1, -1, -1 }, { -1, -1, -1 }, { -1, 1, -1 } };
static const float CUBE_NORMALS[24][3] = {
    { 0, -1, 0 }, { 0, -1, 0 }, { 0, -1, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 1, 0 }, { 0, 1, 0 }, { 0, 1, 0 },
    { 1, 0, 0 }, { 1, 0, 0 }, { 1, 0, 0 }, { 1, 0, 0 }, { 0, 0, 1 }, { 0, 0, 1 }, { 0, 0, 1 }, { 0, 0, 1 },
    { -1, 0, 0 }, { -1, 0, 0 }, { -1, 0, 0 }, { -1, 0, 0 }, { 0, 0, -1 }, { 0, 0, -1 }, { 0, 0, -1 }, { 0, 0, -1 } };
static const float CUBE_TEXCOORDS[24][2] = {
    { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 }, { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 }, { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 },
    { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 }, { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 }, { 0, 1 }, { 1, 1 }, { 1, 0 }, { 0, 0 } };
static const uint32_t CUBE_TRIANGLES[12][3] = {
    { 0, 1, 2 }, { 3, 0, 2 }, { 4, 5, 6 }, { 7, 4, 6 }, { 8, 9, 10 }, { 11, 8, 10 },
    { 12, 13, 14 }, { 15, 12, 14 }, { 16, 17, 18 }, { 19, 16, 18 }, { 20, 21, 22 }, { 23, 20, 22 } };

static uint32_t bsdf_flags(int type) {
    if (type == MTS_BSDF_DIFFUSE) return F_DiffuseReflection | F_FrontSide;                // diffuse.cpp:55
    if (type == MTS_BSDF_NULL) return F_Null | F_FrontSide | F_BackSide;                   // null.cpp:26
    if (type == MTS_BSDF_BILAMBERTIAN) return F_DiffuseReflection | F_DiffuseTransmission | F_FrontSide | F_BackSide;   // bilambertian.cpp:55-60
    if (type == MTS_BSDF_DIELECTRIC) return F_DeltaReflection | F_DeltaTransmission | F_FrontSide | F_BackSide | F_NonSymmetric;   // dielectric.cpp:193-198
    if (type == MTS_BSDF_CONDUCTOR) return F_DeltaReflection | F_FrontSide;               // conductor.cpp:201
    return F_GlossyReflection | F_FrontSide;                                               // rpv.cpp:66
}

// cone.cpp:113-124: the box of the two end circles of radius r -- at the tip as well, where the cone has none: restated, not tightened
static DBBox cone_bbox(const DShape &s) {
    const F3 x1 = mat_vector(s.to_world.m, f3(s.radius, 0.f, 0.f)), x2 = mat_vector(s.to_world.m, f3(0.f, s.radius, 0.f));
    const F3 x = f3(pm_sqrt(x1.x * x1.x + x2.x * x2.x), pm_sqrt(x1.y * x1.y + x2.y * x2.y), pm_sqrt(x1.z * x1.z + x2.z * x2.z));
    const F3 p0 = mat_point_affine(s.to_world.m, f3s(0.f)), p1 = mat_point_affine(s.to_world.m, f3(s.center));
    DBBox b; bbox_reset(b);
    bbox_expand(b, p0 - x); bbox_expand(b, p1 - x); bbox_expand(b, p0 + x); bbox_expand(b, p1 + x);
    return b;
}

// Shape constructors: rectangle.cpp:59-74, cube.cpp:70-112 (+ mesh.cpp), sphere.cpp:80-105, cone.cpp:79-124
static DShape build_shape(const mts_shape &d, HostScene &hs, DBBox &shape_bbox, int &prim_count) {
    DShape s; memset(&s, 0, sizeof(s));
    s.type = d.type;
    s.to_world = xf_from_abi(d.to_world);
    s.bsdf = d.bsdf; s.interior = d.interior_medium; s.exterior = d.exterior_medium; s.emitter = d.emitter;
    s.is_medium_transition = (d.interior_medium >= 0 || d.exterior_medium >= 0) ? 1 : 0;   // shape.h:341
    s.flip_normals = d.flip_normals != 0;
    bbox_reset(shape_bbox);
    if (d.type == MTS_SHAPE_RECTANGLE) {
        if (d.flip_normals) s.to_world = xf_mul(s.to_world, xf_scale(f3(1.f, 1.f, -1.f)));
        s.to_object = xf_inverse(s.to_world);
        F3 dp_du = mat_vector(s.to_world.m, f3(2.f, 0.f, 0.f)), dp_dv = mat_vector(s.to_world.m, f3(0.f, 2.f, 0.f));
        F3 n = normalize(mat_vector(s.to_world.it, f3(0.f, 0.f, 1.f)));
        store3(s.frame_s, dp_du); store3(s.frame_t, dp_dv); store3(s.frame_n, n);
        s.inv_surface_area = pm_rcp(norm(cross(dp_du, dp_dv)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(-1.f, -1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(1.f, -1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(1.f, 1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(-1.f, 1.f, 0.f)));
        prim_count = 1;
    } else if (d.type == MTS_SHAPE_DISK) {                                                     // disk.cpp:74-111
        if (d.flip_normals) s.to_world = xf_mul(s.to_world, xf_scale(f3(1.f, 1.f, -1.f)));
        s.to_object = xf_inverse(s.to_world);
        F3 dp_du = mat_vector(s.to_world.m, f3(1.f, 0.f, 0.f)), dp_dv = mat_vector(s.to_world.m, f3(0.f, 1.f, 0.f));
        float du = norm(dp_du), dv = norm(dp_dv);
        F3 n = normalize(mat_vector(s.to_world.it, f3(0.f, 0.f, 1.f)));
        F3 fs = dp_du / du, ft = dp_dv / dv;
        store3(s.frame_s, fs); store3(s.frame_t, ft); store3(s.frame_n, n);
        float dts = dot(ft * dv, fs);
        float h = pm_sqrt(dv * dv - dts * dts);
        s.surface_area = MTS_PI * du * h;
        s.inv_surface_area = 1.f / s.surface_area;
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(-1.f, -1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(-1.f, 1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(1.f, -1.f, 0.f)));
        bbox_expand(shape_bbox, mat_point_affine(s.to_world.m, f3(1.f, 1.f, 0.f)));
        prim_count = 1;
    } else if (d.type == MTS_SHAPE_CUBE || d.type == MTS_SHAPE_MESH) {
        s.to_object = xf_inverse(s.to_world);
        int nv, nf; const float *pos, *nor, *uv; const uint32_t *fc;
        if (d.type == MTS_SHAPE_CUBE) { nv = 24; nf = 12; pos = &CUBE_VERTICES[0][0]; nor = &CUBE_NORMALS[0][0]; uv = &CUBE_TEXCOORDS[0][0]; fc = &CUBE_TRIANGLES[0][0]; }
        else { nv = d.vertex_count; nf = d.face_count; pos = d.vertex_positions; nor = d.vertex_normals; uv = d.vertex_texcoords; fc = d.faces;
               if (!pos || !fc || nv <= 0 || nf <= 0) throw std::runtime_error("mesh: missing vertex / face data"); }
        // all meshes share one vertex index space; normals / texcoords arrays stay aligned with positions
        s.vertex_offset = (int32_t) (hs.positions.size() / 3);
        s.face_offset = (int32_t) (hs.faces.size() / 3);
        s.has_normals = nor ? 1 : 0; s.has_texcoords = uv ? 1 : 0;
        for (int i = 0; i < nv; ++i) {
            F3 p = mat_point_affine(s.to_world.m, f3(pos + 3 * i));
            bbox_expand(shape_bbox, p);
            hs.positions.push_back(p.x); hs.positions.push_back(p.y); hs.positions.push_back(p.z);
            F3 n = f3s(0.f);
            if (nor) n = normalize(mat_vector(s.to_world.it, f3(nor + 3 * i)));
            hs.normals.push_back(n.x); hs.normals.push_back(n.y); hs.normals.push_back(n.z);
            hs.texcoords.push_back(uv ? uv[2 * i] : 0.f); hs.texcoords.push_back(uv ? uv[2 * i + 1] : 0.f);
        }
        for (int i = 0; i < 3 * nf; ++i) {
            if (fc[i] >= (uint32_t) nv) throw std::runtime_error("mesh: face index out of range");
            hs.faces.push_back(fc[i]);
        }
        prim_count = nf;
    } else if (d.type == MTS_SHAPE_SPHERE) {
        // to_world * translate(center) * scale(radius); radius / rotation recovered from the columns
        // (the reference uses enoki's polar decomposition, absent; identical for rotation * uniform scale)
        DXf tw = xf_mul(s.to_world, xf_mul(xf_translate(f3(d.center)), xf_scale(f3s(d.radius))));
        F3 c0 = f3(tw.m[0], tw.m[4], tw.m[8]), c1 = f3(tw.m[1], tw.m[5], tw.m[9]), c2 = f3(tw.m[2], tw.m[6], tw.m[10]);
        float r0 = norm(c0), r1 = norm(c1), r2 = norm(c2);
        if (pm_abs(r0 - r1) > 1e-6f * r0 || pm_abs(r0 - r2) > 1e-6f * r0 ||
            pm_abs(dot(c0, c1)) > 1e-6f * r0 * r0 || pm_abs(dot(c0, c2)) > 1e-6f * r0 * r0 || pm_abs(dot(c1, c2)) > 1e-6f * r0 * r0)
            throw std::runtime_error("'to_world' transform shouldn't contain any scale or shear along the sphere axes");
        F3 center = f3(tw.m[3], tw.m[7], tw.m[11]);
        store3(s.center, center); s.radius = r0;
        F3 q0 = c0 / r0, q1 = c1 / r0, q2 = c2 / r0;
        float R[9] = { q0.x, q1.x, q2.x, q0.y, q1.y, q2.y, q0.z, q1.z, q2.z };
        DXf rec = xf_identity();
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) rec.m[r * 4 + c] = R[r * 3 + c] * s.radius;
        rec.m[3] = center.x; rec.m[7] = center.y; rec.m[11] = center.z;
        float invm[16]; memset(invm, 0, sizeof(invm));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) invm[r * 4 + c] = R[c * 3 + r] / s.radius;
        for (int r = 0; r < 3; ++r) invm[r * 4 + 3] = -(invm[r * 4] * center.x + invm[r * 4 + 1] * center.y + invm[r * 4 + 2] * center.z);
        invm[15] = 1.f;
        mat_transpose(invm, rec.it);
        s.to_world = rec; s.to_object = xf_inverse(rec);
        s.inv_surface_area = pm_rcp(4.f * MTS_PI * s.radius * s.radius);
        store3(shape_bbox.min, center - f3s(s.radius)); store3(shape_bbox.max, center + f3s(s.radius));
        prim_count = 1;
    } else if (d.type == MTS_SHAPE_CONE) {                                                     // cone.cpp:79-124,187-190
        // to_world = R * diag(r, r, l) + translation: r, l and R recovered from the columns, as the sphere's above (the reference uses
        // enoki's polar decomposition; identical for such a matrix).  The reference only warns about shear and unequal x / y scale and
        // goes on with a record that describes no cone; a mirrored matrix gives it a negative radius or length.  All three are refused here.
        const DXf &tw = s.to_world;
        F3 c0 = f3(tw.m[0], tw.m[4], tw.m[8]), c1 = f3(tw.m[1], tw.m[5], tw.m[9]), c2 = f3(tw.m[2], tw.m[6], tw.m[10]);
        float r0 = norm(c0), r1 = norm(c1), l = norm(c2);
        if (!(r0 > 0.f && r1 > 0.f && l > 0.f))
            throw std::runtime_error("cone: 'to_world' must scale the x / y axes by a radius > 0 and the z axis by a length > 0");
        if (pm_abs(dot(c0, c1)) > 1e-6f * r0 * r0 || pm_abs(dot(c0, c2)) > 1e-6f * r0 * l || pm_abs(dot(c1, c2)) > 1e-6f * r0 * l)
            throw std::runtime_error("cone: 'to_world' transform shouldn't contain any shearing! (refused by this backend: the axes of the cone must stay orthogonal)");
        if (pm_abs(r0 - r1) > 1e-6f * r0)
            throw std::runtime_error("cone: 'to_world' transform shouldn't contain non-uniform scaling along the X and Y axes! (refused by this backend)");
        if (dot(cross(c0, c1), c2) < 0.f)
            throw std::runtime_error("cone: 'to_world' transform shouldn't mirror the cone (negative determinant; refused by this backend)");
        s.radius = r0; s.center[0] = s.center[1] = 0.f; s.center[2] = l;
        F3 q0 = c0 / r0, q1 = c1 / r1, q2 = c2 / l, tr = f3(tw.m[3], tw.m[7], tw.m[11]);
        float R[9] = { q0.x, q1.x, q2.x, q0.y, q1.y, q2.y, q0.z, q1.z, q2.z };
        DXf rec = xf_identity();                                                                 // transform_compose(1, Q, T): rigid
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) rec.m[r * 4 + c] = R[r * 3 + c];
        rec.m[3] = tr.x; rec.m[7] = tr.y; rec.m[11] = tr.z;
        float invm[16]; memset(invm, 0, sizeof(invm));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) invm[r * 4 + c] = R[c * 3 + r];
        for (int r = 0; r < 3; ++r) invm[r * 4 + 3] = -(invm[r * 4] * tr.x + invm[r * 4 + 1] * tr.y + invm[r * 4 + 2] * tr.z);
        invm[15] = 1.f;
        mat_transpose(invm, rec.it);
        s.to_world = rec; s.to_object = xf_inverse(rec);
        s.inv_surface_area = pm_rcp(MTS_PI * s.radius * pm_sqrt(s.radius * s.radius + l * l));
        shape_bbox = cone_bbox(s);
        prim_count = 1;
    } else throw std::runtime_error("unknown shape type");
    return s;
}

static DRFilter build_rfilter(int type, float radius, float stddev, std::vector<float> &values) {
    DRFilter f; memset(&f, 0, sizeof(f));
    f.type = type;
    if (type == MTS_RFILTER_BOX) f.radius = radius + MTS_RAY_EPSILON;                         // box.cpp:31
    else if (type == MTS_RFILTER_GAUSSIAN) {                                                    // gaussian.cpp:33-42
        f.stddev = stddev; f.radius = 4 * stddev; f.alpha = -1.f / (2.f * stddev * stddev); f.bias = pm_exp(f.alpha * (f.radius * f.radius));
    } else throw std::runtime_error("unknown reconstruction filter");
    values.assign(32, 0.f);
    for (int i = 0; i < 31; ++i) {                                                              // rfilter.cpp:9-20 (MTS_FILTER_RESOLUTION = 31)
        float x = (f.radius * i) / 31;
        values[i] = type == MTS_RFILTER_BOX ? (pm_abs(x) <= f.radius ? 1.f : 0.f) : pm_max(0.f, pm_exp(f.alpha * (x * x)) - f.bias);
    }
    values[31] = 0;
    f.scale_factor = 31 / f.radius;
    f.border_size = (int) std::ceil(f.radius - .5f - 2.f * MTS_RAY_EPSILON);
    return f;
}

// Transform::perspective (transform.h:203-220) and perspective_projection (sensor.h:196-231)
static DXf xf_perspective(float fov, float near_, float far_) {
    float recip = 1.f / (far_ - near_);
    float tan_ = std::tan(fov * .5f * (MTS_PI / 180.f)), cot = 1.f / tan_;
    DXf x; memset(&x, 0, sizeof(x));
    x.m[0] = cot; x.m[5] = cot; x.m[10] = far_ * recip; x.m[11] = -near_ * far_ * recip; x.m[14] = 1.f;
    float inv[16]; memset(inv, 0, sizeof(inv));
    inv[0] = tan_; inv[5] = tan_; inv[15] = 1.f / near_; inv[11] = 1.f; inv[14] = (near_ - far_) / (far_ * near_);
    mat_transpose(inv, x.it);
    return x;
}

// Which promises of integrator_dev.h's scene traits (MT_*: what the lean translation units were compiled without) this scene keeps.
// mts_render launches the leanest kernel whose promises are all kept; a scene that keeps none runs on the general kernels.
// `se`: the sensor that renders -- a distant sensor's own target / origin shape counts as the scene's shapes do, so the traits are
// those of a (scene, sensor) pair: HostScene::traits for sensor 0, host_sensor() for any of them.
static int scene_traits(const HostScene &hs, bool spectral, const DSensor &se) {
    if (!hs.instances.empty() || hs.has_cone) return 0;                 // an instanced scene, or one with a cone, promises nothing either: the INST kernels are the general rgb / mono unit's
    if (!hs.bsdf_tex.empty()) return 0;                                 // a scene with textures, a blendbsdf or a twosided promises nothing: the general rgb / mono unit holds the TEX kernels
    int tr = 0;
    bool media = !hs.media.empty();
    for (size_t i = 0; i < hs.media.size(); ++i) {
        const DMedium &m = hs.media[i];
        if (spectral) media = media && !m.is_homogeneous && m.shared_grid == 2 && m.has_spectral_extinction;      // MT_MEDIA of the spectral variant
        else media = media && !m.is_homogeneous && i < hs.pair_data.size() && !hs.pair_data[i].empty() && m.grey && m.has_spectral_extinction;
    }
    if (media) tr |= MT_MEDIA;
    bool homog = !hs.media.empty();
    for (const DMedium &m : hs.media) homog = homog && m.is_homogeneous;
    if (homog) tr |= MT_HOMOG;
    if (hs.bvh_nodes.empty()) tr |= MT_NO_BVH;
    bool sphere = false, rpv = false, shape_emitter = false, tree = false, grid_eval = false;
    for (const DShape &sh : hs.shapes) sphere = sphere || sh.type == MTS_SHAPE_SPHERE;
    sphere = sphere || se.target_shape.type == MTS_SHAPE_SPHERE || se.origin_shape.type == MTS_SHAPE_SPHERE;   // the distant sensors' own shapes
    for (const DBsdf &b : hs.bsdfs) rpv = rpv || b.type == MTS_BSDF_RPV;
    for (const DEmitter &e : hs.emitters) shape_emitter = shape_emitter || e.shape >= 0;
    if (!media)                                                         // a medium that is not on a pair grid reads its grids through volume_eval()
        for (const DMedium &m : hs.media)
            grid_eval = grid_eval || hs.volumes[(size_t) m.sigma_t].type == MTS_VOLUME_GRID || hs.volumes[(size_t) m.albedo].type == MTS_VOLUME_GRID;
    for (const DPhase &ph : hs.phases)
        if (ph.type == MTS_PHASE_BLEND) {
            tree = tree || ph.size > 1;
            grid_eval = grid_eval || (ph.weight_volume >= 0 && hs.volumes[(size_t) ph.weight_volume].type == MTS_VOLUME_GRID);
        }
    if (!sphere) tr |= MT_NO_SPHERE;
    if (!grid_eval) tr |= MT_NO_GRID_EVAL;                               // no grid reaches volume_eval() (pair-grid media do not)
    if (!shape_emitter) tr |= MT_NO_SHAPE_EMITTER;
    if (!tree) tr |= MT_NO_PHASE_TREE;
    if (!rpv) tr |= MT_NO_RPV;
    return tr;
}

// ---------------------------------------------------------------- per-record constructors
// build_host_scene runs them for every record of a description; update_host_scene (mts_scene_update) for the dirty records and the
// records derived from them: creation and update share this code, so an updated scene holds what a fresh one would.

// spectra (spectral variant; uniform.cpp:34-52, regular.cpp:27-58 + distr_1d.h:318-345)
struct SpectrumArrays { std::vector<float> values, wavelengths, cdf; };
static DSpectrum build_spectrum(const mts_spectrum &sp, SpectrumArrays &arrays) {
    DSpectrum ds; memset(&ds, 0, sizeof(ds));
    ds.type = sp.type; ds.value = sp.value; ds.lambda_min = sp.lambda_min; ds.lambda_max = sp.lambda_max;
    if (sp.type == MTS_SPECTRUM_UNIFORM) {
        ds.lambda_min = std::max(sp.lambda_min, 280.f); ds.lambda_max = std::min(sp.lambda_max, 2400.f);       // MTS_WAVELENGTH_MIN / MAX
        if (!(ds.lambda_min < ds.lambda_max)) throw std::runtime_error("UniformSpectrum: 'lambda_min' must be less than 'lambda_max'");
    } else if (sp.type == MTS_SPECTRUM_REGULAR) {
        if (!(sp.lambda_min < sp.lambda_max)) throw std::runtime_error("ContinuousDistribution: invalid range!");
        if (sp.count < 2 || !sp.values) throw std::runtime_error("ContinuousDistribution: needs at least two entries!");
        bool mass = false;
        for (int k = 0; k < sp.count; ++k) { if (sp.values[k] < 0.f) throw std::runtime_error("ContinuousDistribution: entries must be non-negative!"); mass = mass || sp.values[k] > 0.f; }
        if (!mass) throw std::runtime_error("ContinuousDistribution: no probability mass found!");
        arrays.values.assign(sp.values, sp.values + sp.count);
        ds.count = sp.count;
        const double interval_size = (double(sp.lambda_max) - double(sp.lambda_min)) / (sp.count - 1);
        ds.inv_interval_size = (float) (1. / interval_size);
    } else if (sp.type == MTS_SPECTRUM_IRREGULAR) {                  // irregular.cpp:33-63 + IrregularContinuousDistribution (distr_1d.h:560-600)
        if (sp.count < 2 || !sp.values || !sp.wavelengths) throw std::runtime_error("IrregularContinuousDistribution: needs at least two entries!");
        bool mass = false;
        for (int k = 0; k < sp.count; ++k) {
            if (sp.values[k] < 0.f) throw std::runtime_error("IrregularContinuousDistribution: entries must be non-negative!");
            if (k > 0 && !(sp.wavelengths[k] > sp.wavelengths[k - 1])) throw std::runtime_error("IrregularContinuousDistribution: node positions must be strictly increasing!");
            mass = mass || sp.values[k] > 0.f;
        }
        if (!mass) throw std::runtime_error("IrregularContinuousDistribution: no probability mass found!");
        arrays.values.assign(sp.values, sp.values + sp.count);
        arrays.wavelengths.assign(sp.wavelengths, sp.wavelengths + sp.count);
        ds.count = sp.count; ds.lambda_min = sp.wavelengths[0]; ds.lambda_max = sp.wavelengths[sp.count - 1];
    } else if (sp.type == MTS_SPECTRUM_DISCRETE) {                   // discrete.cpp:45-100 + DiscreteDistribution::update (distr_1d.h:49-83)
        if (sp.count < 1 || !sp.values || !sp.wavelengths || !sp.pmf) throw std::runtime_error("DiscreteDistribution: empty distribution!");
        arrays.values.assign(sp.values, sp.values + sp.count);
        arrays.wavelengths.assign(sp.wavelengths, sp.wavelengths + sp.count);
        std::vector<float> &cdf = arrays.cdf; cdf.resize((size_t) sp.count);
        ds.count = sp.count; ds.valid_x = ds.valid_y = (uint32_t) -1;
        double sum = 0.0;
        for (int k = 0; k < sp.count; ++k) {
            const double value = (double) sp.pmf[k];
            sum += value; cdf[(size_t) k] = (float) sum;
            if (value < 0.0) throw std::runtime_error("DiscreteDistribution: entries must be non-negative!");
            else if (value > 0.0) { if (ds.valid_x == (uint32_t) -1) ds.valid_x = (uint32_t) k; ds.valid_y = (uint32_t) k; }
        }
        if (ds.valid_x == (uint32_t) -1) throw std::runtime_error("DiscreteDistribution: no probability mass found!");
        ds.cdf_sum = (float) sum;
    } else throw std::runtime_error("unknown spectrum type");
    return ds;
}

// volumes (texture.cpp:89-92, texture.h:262-269, grid3d.cpp:137-161, volume_data.h:24-33,86-98)
static bool volume_is_grid(const mts_volume &v) { return v.type == MTS_VOLUME_GRID || v.type == MTS_VOLUME_GRID_SPECTRAL; }
// What the constructor derives from a grid's data.  The host loops; grid_update_kernel (kernels.hip) yields the same for a grid in device memory.
// Outside the contract of both: NaNs, and the sign of a maximum that is a tie between -0 and +0 (this loop keeps the zero it met first, the
// kernel's keys put -0 below +0: the two maxima then compare equal and may differ in the sign bit).
struct GridStats { float max; int32_t columns_equal; };
static GridStats grid_stats(const float *data, int nx, int ny, int nz, int channels) {
    GridStats st;
    const size_t n = (size_t) nx * ny * nz * channels;
    float mx = -INFINITY;
    for (size_t k = 0; k < n; ++k) mx = std::max(mx, data[k]);
    st.max = mx;
    {   // a profile that only varies with z (bitwise comparison: the lookups then read column (0, 0) for every corner)
        const size_t row = (size_t) nx * channels, col = (size_t) channels;
        bool equal = true;
        for (size_t z = 0; z < (size_t) nz && equal; ++z) {
            const float *base = data + z * (size_t) ny * row;
            for (size_t c = 1; c < (size_t) ny * nx && equal; ++c) equal = memcmp(base, base + c * col, col * sizeof(float)) == 0;
        }
        st.columns_equal = equal ? 1 : 0;
    }
    return st;
}
// `known`: the statistics of the grid's data when the caller has them already (an update: validation, device grids); NULL: the host
// loops over v.data, once the record has been validated.  `host_data`: v.data is what the grid holds (not so for mts_dirty::device_data).
static void build_volume(const mts_volume &v, bool spectral, int32_t spectrum_count, bool host_data, const GridStats *known, DVolume &dv, DVolumeSp &vsp) {
    memset(&dv, 0, sizeof(dv));
    dv.type = v.type == MTS_VOLUME_GRID_SPECTRAL ? MTS_VOLUME_GRID : v.type; memcpy(dv.value, v.value, 12);
    memset(&vsp, 0, sizeof(vsp)); vsp.value_sp = -1;
    if (spectral && v.type == MTS_VOLUME_CONST) {
        if (v.value_spectrum < 0 || v.value_spectrum >= spectrum_count) throw std::runtime_error("spectral variant: missing spectrum for a constvolume");
        vsp.value_sp = v.value_spectrum;
    }
    if (v.type == MTS_VOLUME_GRID_SPECTRAL) {
        if (!spectral) throw std::runtime_error("This volume data source can only be used with a spectral variant!");     // gridvolume_spectral.cpp:86-88
        if (v.filter_type != MTS_FILTER_TRILINEAR) throw std::runtime_error("Invalid filter type, must be \"trilinear\"!");
        if (v.channels < 2 || v.channels > 255) throw std::runtime_error("gridvolume_spectral: between 2 and 255 spectral nodes are supported");
        vsp.spectral_grid = 1; vsp.lambda_min = v.lambda_min; vsp.lambda_max = v.lambda_max;
    }
    DXf w2l = xf_inverse(xf_from_abi(v.to_world));
    if (volume_is_grid(v)) {
        if (host_data && !v.data) throw std::runtime_error("gridvolume: missing data");
        if ((long) v.nx * v.ny * v.nz < 8) throw std::runtime_error("Invalid grid dimensions (must have at least one value at each corner)");
        if (v.type == MTS_VOLUME_GRID && v.channels != 1 && v.channels != 3) throw std::runtime_error("Unsupported channel count (expected 1 or 3)");
        if (spectral && v.type == MTS_VOLUME_GRID && v.channels != 1)
            throw std::runtime_error("spectral variant: 3-channel grids need the sRGB upsampling model (ext/rgb2spec data, absent); use gridvolume_spectral");
        if ((int64_t) v.nx * v.ny * v.nz * v.channels >= (int64_t) 1 << 31) throw std::runtime_error("gridvolume: more than 2^31 values");
        dv.nx = v.nx; dv.ny = v.ny; dv.nz = v.nz; dv.channels = v.channels; dv.filter = v.filter_type; dv.wrap = v.wrap_mode;
        const GridStats st = known ? *known : grid_stats(v.data, v.nx, v.ny, v.nz, v.channels);
        dv.max = st.max; dv.has_max = 1;
        dv.columns_equal = st.columns_equal;
        if (v.use_grid_bbox) {
            F3 bmin = f3(v.file_bbox_min), bmax = f3(v.file_bbox_max);
            w2l = xf_mul(xf_mul(xf_scale(vrcp(bmax - bmin)), xf_translate(-1.f * bmin)), w2l);
        }
        if (v.has_max_value) dv.max = v.max_value;
    } else if (v.type != MTS_VOLUME_CONST) throw std::runtime_error("unknown volume type");
    memcpy(dv.w2l, w2l.m, 64);
    dv.affine = (w2l.m[12] == 0.f && w2l.m[13] == 0.f && w2l.m[14] == 0.f && w2l.m[15] == 1.f) ? 1 : 0;
    DXf inv = xf_inverse(w2l);
    F3 a = mat_point(inv.m, f3s(0.f)), b = mat_point(inv.m, f3s(1.f));
    store3(dv.bbox.min, a); store3(dv.bbox.max, a); bbox_expand(dv.bbox, b);
}

// phase functions (hg.cpp:43-49, tabphase.cpp:33-51, distr_1d.h:293-345, blendphase.cpp:33-56).  `phases`: the records built so far
// (a blendphase's children come before it); i: this record's index
static DPhase build_phase(const mts_phase &p, int i, const std::vector<DPhase> &phases, int32_t phase_count, int32_t volume_count, std::vector<float> &pdf, std::vector<float> &cdf) {
    DPhase dp; memset(&dp, 0, sizeof(dp));
    dp.type = p.type; dp.g = p.g; dp.child[0] = p.child[0]; dp.child[1] = p.child[1]; dp.weight_volume = p.weight_volume;
    if (p.type == MTS_PHASE_HG && (p.g >= 1 || p.g <= -1)) throw std::runtime_error("The asymmetry parameter must lie in the interval (-1, 1)!");
    if (p.type == MTS_PHASE_BLEND) {
        check_index(p.child[0], phase_count, "blendphase child", false);
        check_index(p.child[1], phase_count, "blendphase child", false);
        check_index(p.weight_volume, volume_count, "blendphase weight", false);
        // nested blendphase plugins (blendphase.cpp:42-66: two arbitrary PhaseFunction children): children come before their parent
        // in the description (the order a loader constructs them in; rules out cycles), DPhase::size = depth of the tree below
        if (p.child[0] >= i || p.child[1] >= i) throw std::runtime_error("blendphase: a nested phase function must precede the blendphase that holds it");
        int depth = 1;
        for (int c = 0; c < 2; ++c)
            if (phases[(size_t) p.child[c]].type == MTS_PHASE_BLEND) depth = std::max(depth, 1 + phases[(size_t) p.child[c]].size);
        if (depth > 8) throw std::runtime_error("blendphase: more than 8 nested levels are not supported by this backend");
        dp.size = depth;
    } else if (p.type == MTS_PHASE_TABULATED) {
        size_t size = (size_t) p.tab_count;
        if (p.tab_count < 2 || !p.tab_values) throw std::runtime_error("ContinuousDistribution: needs at least two entries!");
        pdf.assign(p.tab_values, p.tab_values + size); cdf.resize(size - 1);
        dp.size = (int32_t) size; dp.range_x = -1.f; dp.range_y = 1.f;
        dp.valid_x = dp.valid_y = (uint32_t) -1;
        double range = double(dp.range_y) - double(dp.range_x), interval_size = range / (size - 1), integral = 0.;
        for (size_t k = 0; k < size - 1; ++k) {
            double y0 = (double) pdf[k], y1 = (double) pdf[k + 1];
            double value = 0.5 * interval_size * (y0 + y1);
            integral += value;
            cdf[k] = (float) integral;
            if (y0 < 0. || y1 < 0.) throw std::runtime_error("ContinuousDistribution: entries must be non-negative!");
            else if (value > 0.) { if (dp.valid_x == (uint32_t) -1) dp.valid_x = (uint32_t) k; dp.valid_y = (uint32_t) k; }
        }
        if (dp.valid_x == (uint32_t) -1) throw std::runtime_error("ContinuousDistribution: no probability mass found!");
        dp.integral = (float) integral; dp.normalization = (float) (1. / integral);
        dp.interval_size = (float) interval_size; dp.inv_interval_size = (float) (1. / interval_size);
    } else if (p.type < MTS_PHASE_ISOTROPIC || p.type > MTS_PHASE_TABULATED) throw std::runtime_error("unknown phase function type");
    return dp;
}

// media (medium.cpp:12-29, homogeneous.cpp:21-28, heterogeneous.cpp:21-31), from the volume records they read.  Returns whether the medium
// keeps its two grids interleaved as well (DMedium::pair_grid; build_pair_grid fills it)
static bool build_medium(const mts_medium &m, const HostScene &hs, int32_t volume_count, int32_t phase_count, bool spectral, DMedium &dm) {
    check_index(m.sigma_t_volume, volume_count, "medium sigma_t", false);
    check_index(m.albedo_volume, volume_count, "medium albedo", false);
    check_index(m.phase, phase_count, "medium phase", false);
    memset(&dm, 0, sizeof(dm));
    dm.type = m.type; dm.sigma_t = m.sigma_t_volume; dm.albedo = m.albedo_volume; dm.phase = m.phase; dm.scale = m.scale;
    dm.sample_emitters = m.sample_emitters != 0; dm.has_spectral_extinction = m.has_spectral_extinction != 0;
    dm.is_homogeneous = m.type == MTS_MEDIUM_HOMOGENEOUS;
    if (m.type == MTS_MEDIUM_HETEROGENEOUS) {
        const DVolume &st = hs.volumes[m.sigma_t_volume];
        if (!st.has_max) throw std::runtime_error("max() not implemented (constvolume sigma_t in heterogeneous medium)");
        dm.max_density = dm.scale * st.max;
        // the kernels divide by the majorant two or three times per tracking step: with its correctly rounded reciprocal at hand an
        // IEEE-exact quotient is five multiply-adds instead of the ~11-instruction division sequence (pm_div_by_invariant, pmath.h;
        // the predicate that admits the majorant is pm_invariant_rcp, shared with the tests).
        dm.inv_max_density = pm_invariant_rcp(dm.max_density);
        dm.aabb = st.bbox;
    } else if (m.type != MTS_MEDIUM_HOMOGENEOUS) throw std::runtime_error("unknown medium type");
    // kernel fast paths that do not change a single bit of the result
    const DVolume &a = hs.volumes[m.sigma_t_volume], &b = hs.volumes[m.albedo_volume];
    dm.shared_grid = (a.type == MTS_VOLUME_GRID && b.type == MTS_VOLUME_GRID && a.nx == b.nx && a.ny == b.ny && a.nz == b.nz &&
                      a.filter == b.filter && a.wrap == b.wrap && memcmp(a.w2l, b.w2l, 64) == 0) ? 1 : 0;
    auto grey = [](const DVolume &v) { return v.type == MTS_VOLUME_GRID ? v.channels == 1 : (v.value[0] == v.value[1] && v.value[1] == v.value[2]); };
    dm.grey = (grey(a) && grey(b) && !spectral) ? 1 : 0;       // spectral variant: values depend on the wavelength
    if (spectral && dm.shared_grid) {                          // two gridvolume_spectral grids over one spectral interval: 2
        const DVolumeSp &sa = hs.volume_sp[m.sigma_t_volume], &sb = hs.volume_sp[m.albedo_volume];
        if (sa.spectral_grid && sb.spectral_grid && a.channels == b.channels && sa.lambda_min == sb.lambda_min && sa.lambda_max == sb.lambda_max)
            dm.shared_grid = 2;
    }
    if (!(dm.shared_grid && a.channels == 1 && b.channels == 1 && a.filter == MTS_FILTER_TRILINEAR && a.wrap == MTS_WRAP_CLAMP)) return false;
    memcpy(dm.pair_w2l, a.w2l, 64); dm.pair_nx = a.nx; dm.pair_ny = a.ny; dm.pair_nz = a.nz; dm.pair_affine = (a.affine ? 1 : 0) | ((a.columns_equal && b.columns_equal) ? 2 : 0);
    return true;
}
// the two grids of such a medium interleaved, voxel by voxel {sigma_t, albedo}
static void build_pair_grid(const DVolume &a, const std::vector<float> &ga, const std::vector<float> &gb, std::vector<float> &pair) {
    // rows of at least two voxels (one 16-byte gather = both x-neighbours of both grids): a one-column grid -- the
    // nz x 1 x 1 grids of 1-D atmospheres -- is stored with its column twice; both x-neighbours clamp to voxel 0 anyway
    const size_t sx = a.nx < 2 ? 2 : (size_t) a.nx, rows = (size_t) a.ny * a.nz;
    pair.assign(2 * (sx * rows + 1), 0.f);
    for (size_t r = 0; r < rows; ++r)
        for (size_t x = 0; x < sx; ++x) {
            const size_t src = r * (size_t) a.nx + (x < (size_t) a.nx ? x : (size_t) a.nx - 1);
            pair[2 * (r * sx + x)] = ga[src]; pair[2 * (r * sx + x) + 1] = gb[src];
        }
}

static DBsdf build_bsdf(const mts_bsdf &b) {
    if (b.type < MTS_BSDF_DIFFUSE || b.type > MTS_BSDF_CONDUCTOR || b.type == 5 || b.type == 7) throw std::runtime_error("unknown BSDF type");      // 5, 7: unassigned (mtsamd.h)
    DBsdf db; memset(&db, 0, sizeof(db));
    db.type = b.type;
    if (b.type == MTS_BSDF_DIELECTRIC) {                     // dielectric.cpp:174-199: eta = int_ior / ext_ior; the kernels take its reciprocal
        if (!std::isfinite(b.rho_0[0]) || !(b.rho_0[0] > 0.f)) throw std::runtime_error("dielectric: \"rho_0[0]\" (eta = int_ior / ext_ior) must be finite and positive");
    }
    if (b.type == MTS_BSDF_CONDUCTOR) {                      // conductor.cpp:200-215
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(b.rho_0[c]) || !std::isfinite(b.k[c])) throw std::runtime_error("conductor: \"rho_0\" (eta) and \"k\" must be finite");
    }
    if (b.type == MTS_BSDF_TWOSIDED) {                       // twosided.cpp:63-92: the two child indices and nothing else; flags: resolve_twosided
        memcpy(&db.rho_0[0], &b.spectrum[0], 4); memcpy(&db.rho_0[1], &b.spectrum[1], 4);
        return db;
    }
    if (b.type == MTS_BSDF_BLEND) {                          // blendbsdf.cpp:59-81; DBsdf (dscene.h) says where a blend keeps what; flags: resolve_blend
        if (!std::isfinite(b.reflectance[0])) throw std::runtime_error("blendbsdf: \"reflectance[0]\" (the constant weight) is not finite");
        db.reflectance[0] = b.reflectance[0];
        memcpy(&db.rho_0[0], &b.spectrum[0], 4); memcpy(&db.rho_0[1], &b.spectrum[1], 4);
        return db;
    }
    memcpy(db.reflectance, b.reflectance, 12); memcpy(db.rho_0, b.rho_0, 12); memcpy(db.k, b.k, 12);
    memcpy(db.g, b.g, 12); memcpy(db.rho_c, b.rho_c, 12); memcpy(db.transmittance, b.transmittance, 12); db.flags = bsdf_flags(b.type);
    return db;
}
static int32_t blend_child(const DBsdf &b, int c) { int32_t v; memcpy(&v, &b.rho_0[c], 4); return v; }
// A blend's children, once every record of the description is built (a child may stand behind its blend): the two indices, the kinds
// of BSDF this backend nests, and the blend's flags -- the union of its children's (blendbsdf.cpp:80).  n: the description's bsdf_count
static void resolve_blend(DBsdf &db, int i, const std::vector<DBsdf> &all, int32_t n) {
    for (int c = 0; c < 2; ++c) {
        const std::string field = "bsdf " + std::to_string(i) + ": blendbsdf: \"spectrum[" + std::to_string(c) + "]\" (bsdf_" + std::to_string(c) + ")";
        const int32_t ch = blend_child(db, c);
        if (ch < 0 || ch >= n) throw std::runtime_error("index out of range: " + field);
        if (ch == i) throw std::runtime_error(field + " is the blend itself");
        const int t = all[(size_t) ch].type;
        // a null or a nested child needs the component flags the integrators read (BSDFContext::component); a limit of this backend
        if (t == MTS_BSDF_NULL) throw std::runtime_error(field + " is a null BSDF: null children are not supported by this backend");
        if (t == MTS_BSDF_BLEND) throw std::runtime_error(field + " is a blendbsdf: nested blends are not supported by this backend");
        if (t == MTS_BSDF_TWOSIDED) throw std::runtime_error(field + " is a twosided: a twosided inside a blend is not supported by this backend");
        // a delta lobe in a mixture needs the blend's pdf to stay the child's (blendbsdf.cpp:117-121) through the specular chain: not restated
        if (t == MTS_BSDF_DIELECTRIC) throw std::runtime_error(field + " is a dielectric: specular children are not supported in a blend by this backend");
        if (t == MTS_BSDF_CONDUCTOR) throw std::runtime_error(field + " is a conductor: specular children are not supported in a blend by this backend");
    }
    db.flags = all[(size_t) blend_child(db, 0)].flags | all[(size_t) blend_child(db, 1)].flags;
}
// A twosided's children, once every record is built and every blend resolved (a blend child's flags are its own children's union): the
// two indices, the nesting this backend lacks, the reference's transmission rule (twosided.cpp:90-91; Null is one of
// BSDFFlags::Transmission's bits, bsdf.h) decided from the children's flags, and the record's own flags (:78-88).
static void resolve_twosided(DBsdf &db, int i, const std::vector<DBsdf> &all, int32_t n) {
    uint32_t side[2];
    for (int c = 0; c < 2; ++c) {
        const std::string field = "bsdf " + std::to_string(i) + ": twosided: \"spectrum[" + std::to_string(c) + "]\" (brdf_" + std::to_string(c) + ")";
        const int32_t ch = blend_child(db, c);
        if (ch < 0 || ch >= n) throw std::runtime_error("index out of range: " + field);
        if (ch == i) throw std::runtime_error(field + " is the twosided itself");
        if (all[(size_t) ch].type == MTS_BSDF_TWOSIDED) throw std::runtime_error(field + " is a twosided: nested twosided adapters are not supported by this backend");
        side[c] = all[(size_t) ch].flags;
    }
    db.flags = ((side[0] & ~F_BackSide) | F_FrontSide) | ((side[1] & ~F_FrontSide) | F_BackSide);
    if (db.flags & F_Transmission) throw std::runtime_error("bsdf " + std::to_string(i) + ": twosided: Only materials without a transmission component can be nested!");
}
// which of the six colour parameters each BSDF plugin reads (spectral variant: the spectra it needs); a blend: slot 0 is its weight's texture
// twosided reads no colour parameter and no texture slot (types 5 and 7 are unassigned); a dielectric's eta is a float, a conductor's
// eta and k are constants: their texture slots stay -1
static const bool BSDF_SP_USED[10][6] = { { 1, 0, 0, 0, 0, 0 } /* diffuse */, { 0, 0, 0, 0, 0, 0 } /* null */, { 0, 1, 1, 1, 1, 0 } /* rpv */, { 1, 0, 0, 0, 0, 1 } /* bilambertian */,
                                          { 1, 0, 0, 0, 0, 0 } /* blend */, { 0, 0, 0, 0, 0, 0 } /* unassigned */, { 0, 0, 0, 0, 0, 0 } /* twosided */, { 0, 0, 0, 0, 0, 0 } /* unassigned */,
                                          { 1, 0, 0, 0, 0, 1 } /* dielectric */, { 1, 0, 0, 0, 0, 0 } /* conductor */ };

// A texture's record and (bitmap) its texels as the device holds them: validated as BitmapTexture's / Checkerboard's constructors
// validate (bitmap.cpp:92-206, checkerboard.cpp:40-44).  `with_data` = false: the record alone (an update checks the frozen fields first).
static DTexture build_texture(const mts_texture &t, int i, bool mono, bool with_data, std::vector<float> &texels) {
    const std::string name = "texture " + std::to_string(i) + ": ";
    DTexture dt; memset(&dt, 0, sizeof(dt));
    if (t.type != MTS_TEXTURE_BITMAP && t.type != MTS_TEXTURE_CHECKERBOARD) throw std::runtime_error(name + "unknown texture type");
    dt.type = t.type;
    for (int k = 0; k < 9; ++k) { if (!std::isfinite(t.to_uv[k])) throw std::runtime_error(name + "\"to_uv\" is not finite"); dt.to_uv[k] = t.to_uv[k]; }
    if (t.type == MTS_TEXTURE_CHECKERBOARD) {
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(t.color0[k]) || !std::isfinite(t.color1[k])) throw std::runtime_error(name + "checkerboard: \"color0\" / \"color1\" must be finite");
            dt.color0[k] = t.color0[k]; dt.color1[k] = t.color1[k];
        }
        return dt;
    }
    if (t.channels != 1 && t.channels != 3) throw std::runtime_error(name + "Unsupported channel count: " + std::to_string(t.channels) + " (expected 1 or 3)");       // bitmap.cpp:196
    if (mono && t.channels != 1) throw std::runtime_error(name + "a monochromatic scene takes single-channel bitmaps (the caller reduces rgb texels to their luminance)");
    // bitmap.cpp:155-161 up-samples smaller images with a tent filter, which this backend has not got
    if (t.width < 2 || t.height < 2) throw std::runtime_error(name + "Image must be at least 2x2 pixels in size (got " + std::to_string(t.width) + "x" + std::to_string(t.height) + "; this backend does not up-sample)");
    if ((int64_t) t.width * t.height > ((int64_t) 1 << 28)) throw std::runtime_error(name + "bitmap too large (more than 2^28 texels)");
    if (t.filter_type != MTS_FILTER_NEAREST && t.filter_type != MTS_FILTER_BILINEAR) throw std::runtime_error(name + "Invalid filter type, must be one of: \"nearest\", or \"bilinear\"!");
    if (t.wrap_mode != MTS_WRAP_REPEAT && t.wrap_mode != MTS_WRAP_MIRROR && t.wrap_mode != MTS_WRAP_CLAMP) throw std::runtime_error(name + "Invalid wrap mode, must be one of: \"repeat\", \"mirror\", or \"clamp\"!");
    if (!t.data) throw std::runtime_error(name + "bitmap without data");
    dt.width = t.width; dt.height = t.height; dt.channels = t.channels; dt.filter = t.filter_type; dt.wrap = t.wrap_mode;
    if (!with_data) return dt;
    const size_t n = (size_t) t.width * t.height;
    for (size_t k = 0; k < n * (size_t) t.channels; ++k) if (std::isnan(t.data[k])) throw std::runtime_error(name + "bitmap data contains NaN");
    if (t.channels == 1) texels.assign(t.data, t.data + n);
    else {
        texels.assign(4 * n, 0.f);
        for (size_t k = 0; k < n; ++k) { texels[4 * k] = t.data[3 * k]; texels[4 * k + 1] = t.data[3 * k + 1]; texels[4 * k + 2] = t.data[3 * k + 2]; }
    }
    return dt;
}

// an emitter's record; the scene's bounding sphere comes from set_scene (scene.cpp:95-97)
static DEmitter build_emitter(const mts_emitter &e, const float center[3], float bsphere_radius) {
    DEmitter de; memset(&de, 0, sizeof(de));
    de.type = e.type; de.to_world = xf_from_abi(e.to_world); memcpy(de.radiance, e.radiance, 12); de.shape = e.shape;
    memcpy(de.bsphere_center, center, 12); de.bsphere_radius = bsphere_radius;
    return de;
}
// the response function's weights can be recovered from the sampled wavelengths (srf_weights_of, integrator_dev.h, looks a weight up by its wavelength)
// `srf`: a sensor's response function, an index into hs.spectra or -1
static bool srf_lookup_by_wavelength(const HostScene &hs, int32_t srf) {
    if (srf < 0 || hs.spectra[(size_t) srf].type != MTS_SPECTRUM_DISCRETE) return true;
    const std::vector<float> &w = hs.spectrum_wavelengths[(size_t) srf];
    for (size_t k = 1; k < w.size(); ++k) if (!(w[k] > w[k - 1])) return false;
    return true;
}

// ---------------------------------------------------------------- sections of a description
// build_host_scene runs one function per section, in a fixed order: the order decides which of two faults of a description is reported.
static int32_t spectrum_index(const mts_scene_desc &d, int idx, const char *what) {
    if (idx < 0 || idx >= d.spectrum_count) throw std::runtime_error(std::string("spectral variant: missing spectrum for ") + what);
    return idx;
}
static void build_spectra(const mts_scene_desc &d, HostScene &hs) {
    if (d.integrator.monochrome) throw std::runtime_error("a scene is either monochromatic or spectral");
    for (int i = 0; i < d.spectrum_count; ++i) {
        SpectrumArrays arrays;
        hs.spectra.push_back(build_spectrum(d.spectra[i], arrays));
        hs.spectrum_values.push_back(std::move(arrays.values)); hs.spectrum_wavelengths.push_back(std::move(arrays.wavelengths)); hs.spectrum_cdf.push_back(std::move(arrays.cdf));
    }
}
static int32_t add_uniform_spectrum(HostScene &hs, float value) {
    DSpectrum ds; memset(&ds, 0, sizeof(ds)); ds.type = MTS_SPECTRUM_UNIFORM; ds.value = value; ds.lambda_min = 280.f; ds.lambda_max = 2400.f;
    hs.spectra.push_back(ds); hs.spectrum_values.emplace_back(); hs.spectrum_wavelengths.emplace_back(); hs.spectrum_cdf.emplace_back();
    return (int32_t) hs.spectra.size() - 1;
}
static void build_volumes(const mts_scene_desc &d, bool spectral, HostScene &hs) {
    for (int i = 0; i < d.volume_count; ++i) {
        const mts_volume &v = d.volumes[i];
        DVolume dv; DVolumeSp vsp;
        build_volume(v, spectral, d.spectrum_count, true, nullptr, dv, vsp);
        hs.volumes.push_back(dv); hs.volume_sp.push_back(vsp);
        if (volume_is_grid(v)) hs.grid_data.emplace_back(v.data, v.data + (size_t) v.nx * v.ny * v.nz * v.channels);
        else hs.grid_data.emplace_back();
    }
}
static void build_phases(const mts_scene_desc &d, HostScene &hs) {
    for (int i = 0; i < d.phase_count; ++i) {
        hs.tab_pdf.emplace_back(); hs.tab_cdf.emplace_back();
        hs.phases.push_back(build_phase(d.phases[i], i, hs.phases, d.phase_count, d.volume_count, hs.tab_pdf.back(), hs.tab_cdf.back()));
    }
}
static void build_media(const mts_scene_desc &d, bool spectral, HostScene &hs) {
    for (int i = 0; i < d.medium_count; ++i) {
        const mts_medium &m = d.media[i];
        DMedium dm; std::vector<float> pair;
        if (build_medium(m, hs, d.volume_count, d.phase_count, spectral, dm))
            build_pair_grid(hs.volumes[(size_t) m.sigma_t_volume], hs.grid_data[(size_t) m.sigma_t_volume], hs.grid_data[(size_t) m.albedo_volume], pair);
        hs.pair_data.push_back(std::move(pair)); hs.media.push_back(dm);
    }
}
// BSDFs, and the default ones appended after the user's (shape.cpp:74-80): diffuse 0.5, and diffuse 0 for emitters
struct DefaultBsdfs { int plain, emitter; };
static DefaultBsdfs build_bsdfs(const mts_scene_desc &d, bool spectral, HostScene &hs) {
    for (int i = 0; i < d.bsdf_count; ++i)                               // a blend is refused where textures are, and for the same reasons (build_textures)
        if (d.bsdfs[i].type == MTS_BSDF_BLEND) {
            if (spectral) throw std::runtime_error("bsdf " + std::to_string(i) + ": blendbsdf is not supported in the spectral variant");
            if (d.integrator.moment != 0) throw std::runtime_error("bsdf " + std::to_string(i) + ": blendbsdf is not supported inside a moment integrator's scene");
        } else if (d.bsdfs[i].type == MTS_BSDF_TWOSIDED) {               // and so is a twosided: it renders in the TEX instantiations alone
            if (spectral) throw std::runtime_error("bsdf " + std::to_string(i) + ": twosided is not supported in the spectral variant");
            if (d.integrator.moment != 0) throw std::runtime_error("bsdf " + std::to_string(i) + ": twosided is not supported inside a moment integrator's scene");
        } else if (d.bsdfs[i].type == MTS_BSDF_DIELECTRIC || d.bsdfs[i].type == MTS_BSDF_CONDUCTOR) {     // and so are the smooth specular BSDFs
            const std::string what = d.bsdfs[i].type == MTS_BSDF_DIELECTRIC ? "dielectric" : "conductor";
            if (spectral) throw std::runtime_error("bsdf " + std::to_string(i) + ": " + what + " is not supported in the spectral variant");
            if (d.integrator.moment != 0) throw std::runtime_error("bsdf " + std::to_string(i) + ": " + what + " is not supported inside a moment integrator's scene");
        }
    for (int i = 0; i < d.bsdf_count; ++i) {
        const mts_bsdf &b = d.bsdfs[i];
        try { hs.bsdfs.push_back(build_bsdf(b)); }
        catch (const std::runtime_error &e) { if (b.type != MTS_BSDF_BLEND && b.type != MTS_BSDF_TWOSIDED && b.type != MTS_BSDF_DIELECTRIC && b.type != MTS_BSDF_CONDUCTOR) throw; throw std::runtime_error("bsdf " + std::to_string(i) + ": " + e.what()); }
        if (spectral)                                                    // which of the six colour parameters each plugin reads
            for (int k = 0; k < MTS_BSDF_SP_COUNT; ++k) hs.bsdf_sp.push_back(BSDF_SP_USED[b.type][k] ? spectrum_index(d, b.spectrum[k], "a BSDF parameter") : 0);
    }
    for (int i = 0; i < d.bsdf_count; ++i)
        if (hs.bsdfs[(size_t) i].type == MTS_BSDF_BLEND) resolve_blend(hs.bsdfs[(size_t) i], i, hs.bsdfs, d.bsdf_count);
    for (int i = 0; i < d.bsdf_count; ++i)                               // after every blend: a blend child's flags are read, wherever it stands
        if (hs.bsdfs[(size_t) i].type == MTS_BSDF_TWOSIDED) resolve_twosided(hs.bsdfs[(size_t) i], i, hs.bsdfs, d.bsdf_count);
    DefaultBsdfs ids; DBsdf def; memset(&def, 0, sizeof(def)); def.type = MTS_BSDF_DIFFUSE; def.flags = bsdf_flags(MTS_BSDF_DIFFUSE);
    def.reflectance[0] = def.reflectance[1] = def.reflectance[2] = .5f; ids.plain = (int) hs.bsdfs.size(); hs.bsdfs.push_back(def);
    def.reflectance[0] = def.reflectance[1] = def.reflectance[2] = 0.f; ids.emitter = (int) hs.bsdfs.size(); hs.bsdfs.push_back(def);
    if (spectral) {
        const int32_t half = add_uniform_spectrum(hs, .5f), zero = add_uniform_spectrum(hs, 0.f);
        for (int k = 0; k < MTS_BSDF_SP_COUNT; ++k) hs.bsdf_sp.push_back(half);
        for (int k = 0; k < MTS_BSDF_SP_COUNT; ++k) hs.bsdf_sp.push_back(zero);
    }
    return ids;
}
// the six texture indices of BSDF i as the scene keeps them: range-checked, -1 for a parameter the plugin does not read
static void bsdf_texture_indices(const mts_scene_desc &d, int i, int32_t out[MTS_BSDF_SP_COUNT]) {
    for (int k = 0; k < MTS_BSDF_SP_COUNT; ++k) {
        const int32_t t = d.bsdf_textures ? d.bsdf_textures[(size_t) i * MTS_BSDF_SP_COUNT + k] : -1;
        if (t < -1 || t >= d.texture_count) throw std::runtime_error("index out of range: bsdf " + std::to_string(i) + " texture");
        out[k] = BSDF_SP_USED[d.bsdfs[i].type][k] ? t : -1;
    }
}
// Textures (after the BSDFs: the table has a row for each of them, the two default ones included).  A scene without a texture
// record keeps all three arrays empty, whatever its index table says -- unless it holds a blendbsdf or a twosided: then the table alone exists.
// A non-empty table is what sends a scene to the TEX instantiations (scene_traits, capi.cpp).
static void build_textures(const mts_scene_desc &d, bool spectral, HostScene &hs) {
    if (d.texture_count < 0 || (d.texture_count > 0 && !d.textures)) throw std::runtime_error("textures: a negative count, or records missing");
    if (d.texture_count == 0) {
        for (int i = 0; i < d.bsdf_count; ++i) { int32_t t[MTS_BSDF_SP_COUNT]; bsdf_texture_indices(d, i, t); }        // nothing but -1 is in range
        // a blend, a twosided, a dielectric or a conductor renders in the TEX instantiations, which read the index table: all -1 under a constant weight and plain children
        for (int i = 0; i < d.bsdf_count; ++i)
            if (d.bsdfs[i].type == MTS_BSDF_BLEND || d.bsdfs[i].type == MTS_BSDF_TWOSIDED || d.bsdfs[i].type == MTS_BSDF_DIELECTRIC || d.bsdfs[i].type == MTS_BSDF_CONDUCTOR) { hs.bsdf_tex.assign(hs.bsdfs.size() * MTS_BSDF_SP_COUNT, -1); break; }
        // so does an instanced scene, and one with a cone: the INST kernels are TEX instantiations
        for (int i = 0; i < d.shape_count; ++i)
            if (d.shapes[i].type == MTS_SHAPE_INSTANCE || d.shapes[i].type == MTS_SHAPE_CONE) { hs.bsdf_tex.assign(hs.bsdfs.size() * MTS_BSDF_SP_COUNT, -1); break; }
        return;
    }
    // rgb texels need the sRGB upsampling model (bitmap.cpp:169-178), whose data this backend has not got -- as for three-channel grids
    if (spectral) throw std::runtime_error("textures are not supported in the spectral variant");
    if (d.integrator.moment != 0) throw std::runtime_error("textures are not supported inside a moment integrator's scene");
    for (int i = 0; i < d.texture_count; ++i) {
        hs.texels.emplace_back();
        hs.textures.push_back(build_texture(d.textures[i], i, d.integrator.monochrome != 0, true, hs.texels.back()));
    }
    hs.bsdf_tex.assign(hs.bsdfs.size() * MTS_BSDF_SP_COUNT, -1);
    for (int i = 0; i < d.bsdf_count; ++i) bsdf_texture_indices(d, i, &hs.bsdf_tex[(size_t) i * MTS_BSDF_SP_COUNT]);
    hs.scene.texture_count = d.texture_count;
}
// one shape of the description: its record, its primitives and their rows in the per-primitive tables; the scene's bounding box grows (scene.cpp:31-40)
// `bbox`: the box that grows -- the scene's, or the group's of a shapegroup's member (group space)
static void add_shape(const mts_scene_desc &d, int i, const DefaultBsdfs &defaults, HostScene &hs, DBBox &bbox) {
    const mts_shape &s = d.shapes[i];
    check_index(s.bsdf, d.bsdf_count, "shape bsdf", true); check_index(s.interior_medium, d.medium_count, "shape interior", true);
    check_index(s.exterior_medium, d.medium_count, "shape exterior", true); check_index(s.emitter, d.emitter_count, "shape emitter", true);
    DBBox sb; int prim_count;
    DShape ds = build_shape(s, hs, sb, prim_count);
    if (ds.bsdf < 0) ds.bsdf = ds.emitter >= 0 ? defaults.emitter : defaults.plain;
    ds.bsdf_type = hs.bsdfs[(size_t) ds.bsdf].type; ds.bsdf_flags = hs.bsdfs[(size_t) ds.bsdf].flags;
    ds.prim_offset = (int32_t) hs.prims.size();
    hs.shapes[(size_t) i] = ds; bbox_expand(bbox, sb);
    // DScene::cross_mask: the scene's own shapes only -- a hit on a group's member carries its instance above the shape index (Hit::shape), so no bit could serve it
    if (&bbox == &hs.scene.bbox && i < 64 && ds.bsdf_type == MTS_BSDF_NULL && (ds.bsdf_flags & F_Smooth) == 0 && ds.emitter < 0) hs.scene.cross_mask |= 1ull << i;
    const bool triangles = ds.type == MTS_SHAPE_CUBE || ds.type == MTS_SHAPE_MESH;
    for (int k = 0; k < prim_count; ++k) {
        DPrim p; p.shape = i; p.index = k; hs.prims.push_back(p);
        float rec[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, attr[24] = { 0 };
        if (triangles) {                                                     // mesh.h:201-207: p0, e1 = p1 - p0, e2 = p2 - p0
            const uint32_t *fi = &hs.faces[3 * (ds.face_offset + k)];
            const float *P = &hs.positions[3 * ds.vertex_offset];
            F3 p0 = f3(P + 3 * fi[0]), e1 = f3(P + 3 * fi[1]) - p0, e2 = f3(P + 3 * fi[2]) - p0;
            store3(rec, p0); store3(rec + 3, e1); store3(rec + 6, e2);
            for (int c = 0; c < 3; ++c) {
                memcpy(attr + 3 * c, &hs.positions[3 * (ds.vertex_offset + fi[c])], 12);
                memcpy(attr + 9 + 3 * c, &hs.normals[3 * (ds.vertex_offset + fi[c])], 12);
                memcpy(attr + 18 + 2 * c, &hs.texcoords[2 * (ds.vertex_offset + fi[c])], 8);
            }
        }
        hs.tri.insert(hs.tri.end(), rec, rec + 9); hs.tri_attr.insert(hs.tri_attr.end(), attr, attr + 24);
        DWalkPrim w; memset(&w, 0, sizeof(w)); w.type = ds.type; w.shape = i; w.index = k;
        if (ds.type == MTS_SHAPE_RECTANGLE || ds.type == MTS_SHAPE_DISK) memcpy(w.f, ds.to_object.m, 48);
        else if (ds.type == MTS_SHAPE_SPHERE) { memcpy(w.f, ds.center, 12); w.f[3] = ds.radius; }
        else if (ds.type == MTS_SHAPE_CONE) { memcpy(w.f, ds.to_object.m, 48); memcpy(&w.index, &ds.radius, 4); memcpy(&w.pad, &ds.center[2], 4); }      // dscene.h: DWalkPrim
        else memcpy(w.f, rec, 36);
        hs.walk.push_back(w);
        hs.area_pmf.push_back(triangles ? 0.5f * norm(cross(f3(rec + 3), f3(rec + 6))) : 0.f);      // mesh.h:108-116: face area
    }
    if (triangles) {
        // Mesh::build_pmf (mesh.cpp:285-312) + DiscreteDistribution::update (distr_1d.h:49-83): running sum in double precision
        DShape &sh = hs.shapes[(size_t) i];
        double sum = 0.0; sh.area_lo = sh.area_hi = -1;
        for (int k = 0; k < prim_count; ++k) {
            float a = hs.area_pmf[(size_t) sh.prim_offset + k];
            sum += (double) a; hs.area_cdf.push_back((float) sum);
            if (a > 0.f) { if (sh.area_lo < 0) sh.area_lo = k; sh.area_hi = k; }
        }
        sh.surface_area = (float) sum; sh.inv_surface_area = (float) (1.0 / sum);         // mesh.cpp:346-350,373
    } else for (int k = 0; k < prim_count; ++k) hs.area_cdf.push_back(0.f);
}
// ---- instanced geometry (mtsamd.h: MTS_SHAPE_SHAPEGROUP / MTS_SHAPE_INSTANCE; shapegroup.cpp, instance.cpp)
static bool shape_is_instancing(int type) { return type == MTS_SHAPE_SHAPEGROUP || type == MTS_SHAPE_INSTANCE; }
// Everything the description can get wrong about groups and instances, before any record is built.  member_of[i]: the index of the
// group record shape i is a member of, -1 for the scene's own shapes (groups and instances included).
static std::vector<int32_t> validate_instancing(const mts_scene_desc &d, bool spectral) {
    std::vector<int32_t> member_of((size_t) std::max(d.shape_count, 0), -1);
    bool any = false; int64_t instances = 0;
    for (int i = 0; i < d.shape_count; ++i) any = any || shape_is_instancing(d.shapes[i].type);
    if (!any) return member_of;
    const auto name = [](int i) { return "shape " + std::to_string(i) + ": "; };
    if (spectral) throw std::runtime_error("shapegroup / instance shapes are not supported in the spectral variant");
    if (d.integrator.moment != 0) throw std::runtime_error("shapegroup / instance shapes are not supported inside a moment integrator's scene");
    for (int i = 0; i < d.shape_count; ++i) {
        const mts_shape &s = d.shapes[i];
        if (s.type != MTS_SHAPE_SHAPEGROUP) continue;
        if (member_of[(size_t) i] >= 0) throw std::runtime_error(name(i) + "a shapegroup among the members of shapegroup " + std::to_string(member_of[(size_t) i]) + " (Nested ShapeGroup is not permitted)");
        if (s.face_count < 0 || (int64_t) i + 1 + s.face_count > (int64_t) d.shape_count)
            throw std::runtime_error(name(i) + "shapegroup: its " + std::to_string(s.face_count) + " members (face_count) run past the end of the shape array");
        for (int m = i + 1; m <= i + s.face_count; ++m) {
            const mts_shape &mem = d.shapes[m];
            if (mem.type == MTS_SHAPE_SHAPEGROUP) throw std::runtime_error(name(m) + "a shapegroup among the members of shapegroup " + std::to_string(i) + " (Nested ShapeGroup is not permitted)");
            if (mem.type == MTS_SHAPE_INSTANCE) throw std::runtime_error(name(m) + "an instance among the members of shapegroup " + std::to_string(i) + " (Nested instancing is not permitted)");
            if (mem.emitter != -1) throw std::runtime_error(name(m) + "a member of shapegroup " + std::to_string(i) + " carries an emitter (Instancing of emitters is not supported)");
            if (mem.interior_medium != -1) throw std::runtime_error(name(m) + "a member of shapegroup " + std::to_string(i) + " has an \"interior\" medium: media on instanced shapes are not supported on this backend");
            if (mem.exterior_medium != -1) throw std::runtime_error(name(m) + "a member of shapegroup " + std::to_string(i) + " has an \"exterior\" medium: media on instanced shapes are not supported on this backend");
            member_of[(size_t) m] = i;
        }
    }
    for (int i = 0; i < d.shape_count; ++i) {
        const mts_shape &s = d.shapes[i];
        if (s.type != MTS_SHAPE_INSTANCE) continue;
        ++instances;
        if (s.vertex_count < 0 || s.vertex_count >= d.shape_count) throw std::runtime_error(name(i) + "instance: its group index (vertex_count) " + std::to_string(s.vertex_count) + " is out of range");
        if (d.shapes[s.vertex_count].type != MTS_SHAPE_SHAPEGROUP) throw std::runtime_error(name(i) + "instance: shape " + std::to_string(s.vertex_count) + " is not a shapegroup (Only a shapegroup can be specified in an instance.)");
        if (s.bsdf != -1 || s.interior_medium != -1 || s.exterior_medium != -1 || s.emitter != -1)
            throw std::runtime_error(name(i) + "instance: bsdf, interior, exterior and emitter must be -1 (the members of its shapegroup carry the material)");
    }
    for (int i = 0; i < d.emitter_count; ++i)
        if (d.emitters[i].type == MTS_EMITTER_AREA && d.emitters[i].shape >= 0 && d.emitters[i].shape < d.shape_count &&
            (shape_is_instancing(d.shapes[d.emitters[i].shape].type) || member_of[(size_t) d.emitters[i].shape] >= 0))
            throw std::runtime_error("emitter " + std::to_string(i) + ": its shape " + std::to_string(d.emitters[i].shape) + " is a shapegroup, one of its members or an instance (Instancing of emitters is not supported)");
    if (instances > 0 && d.shape_count > MTS_INST_MAX_SHAPES)
        throw std::runtime_error("an instanced scene holds at most " + std::to_string(MTS_INST_MAX_SHAPES) + " shape records (shape_count = " + std::to_string(d.shape_count) + "): the hit encoding keeps the shape in " + std::to_string(MTS_INST_SHAPE_BITS) + " bits");
    if (instances > MTS_INST_MAX_INSTANCES)
        throw std::runtime_error("at most " + std::to_string(MTS_INST_MAX_INSTANCES) + " instances per scene (the hit encoding), this one has " + std::to_string(instances));
    return member_of;
}
// What a description with a cone (MTS_SHAPE_CONE, plain or a group's member) can get wrong as a scene: such a scene renders in the INST
// kernels, so it shares their limits.  The cone's own transform is checked where its record is built (build_shape).
static bool validate_cones(const mts_scene_desc &d, bool spectral) {
    bool any = false;
    for (int i = 0; i < d.shape_count; ++i) any = any || d.shapes[i].type == MTS_SHAPE_CONE;
    if (!any) return false;
    if (spectral) throw std::runtime_error("cone shapes are not supported in the spectral variant");
    if (d.integrator.moment != 0) throw std::runtime_error("cone shapes are not supported inside a moment integrator's scene");
    if (d.shape_count > MTS_INST_MAX_SHAPES)
        throw std::runtime_error("a scene with a cone holds at most " + std::to_string(MTS_INST_MAX_SHAPES) + " shape records (shape_count = " + std::to_string(d.shape_count) + "): the hit encoding keeps the shape in " + std::to_string(MTS_INST_SHAPE_BITS) + " bits");
    for (int i = 0; i < d.shape_count; ++i)
        if (d.shapes[i].type == MTS_SHAPE_CONE && d.shapes[i].emitter != -1)
            throw std::runtime_error("shape " + std::to_string(i) + ": an area emitter on a cone is not supported on this backend (the cone's sample_position is not built)");
    for (int i = 0; i < d.emitter_count; ++i)
        if (d.emitters[i].type == MTS_EMITTER_AREA && d.emitters[i].shape >= 0 && d.emitters[i].shape < d.shape_count && d.shapes[d.emitters[i].shape].type == MTS_SHAPE_CONE)
            throw std::runtime_error("emitter " + std::to_string(i) + ": its shape " + std::to_string(d.emitters[i].shape) + " is a cone: an area emitter on a cone is not supported on this backend (the cone's sample_position is not built)");
    return true;
}
// A group's bounding box: that of its acceleration structure, the union of its members' (shapegroup.cpp; group space)
static DBBox group_bbox(const mts_scene_desc &d, int g) {
    DBBox b; bbox_reset(b);
    for (int m = g + 1; m <= g + d.shapes[g].face_count; ++m) { HostScene scratch; DBBox sb; int pc; (void) build_shape(d.shapes[m], scratch, sb, pc); bbox_expand(b, sb); }
    return b;
}
// One instance: a shape record that holds its transform, ONE primitive of the scene (instance.cpp:94) whose walk record carries rows
// 0..2 of to_object, and its device record.  `group`: the index of its group in hs.groups, `gb` that group's box.
static void add_instance(const mts_scene_desc &d, int i, int group, const DBBox &gb, const DefaultBsdfs &defaults, HostScene &hs) {
    DShape ds; memset(&ds, 0, sizeof(ds));
    ds.type = MTS_SHAPE_INSTANCE;
    ds.to_world = xf_from_abi(d.shapes[i].to_world); ds.to_object = xf_inverse(ds.to_world);       // instance.cpp:63-64
    ds.bsdf = defaults.plain; ds.interior = ds.exterior = ds.emitter = -1;                          // never read: a hit names a member
    ds.bsdf_type = hs.bsdfs[(size_t) ds.bsdf].type; ds.bsdf_flags = hs.bsdfs[(size_t) ds.bsdf].flags;
    ds.prim_offset = (int32_t) hs.prims.size(); ds.area_lo = ds.area_hi = -1;
    ds.vertex_offset = group;
    hs.shapes[(size_t) i] = ds;
    DBBox ib; bbox_reset(ib);                                                                       // instance.cpp:81-92: the eight transformed corners
    if (gb.min[0] <= gb.max[0] && gb.min[1] <= gb.max[1] && gb.min[2] <= gb.max[2])
        for (int k = 0; k < 8; ++k)
            bbox_expand(ib, mat_point_affine(ds.to_world.m, f3((k & 1) ? gb.max[0] : gb.min[0], (k & 2) ? gb.max[1] : gb.min[1], (k & 4) ? gb.max[2] : gb.min[2])));
    bbox_expand(hs.scene.bbox, ib);
    DPrim p; p.shape = i; p.index = 0; hs.prims.push_back(p);
    const float zero[24] = { 0 };
    hs.tri.insert(hs.tri.end(), zero, zero + 9); hs.tri_attr.insert(hs.tri_attr.end(), zero, zero + 24);
    DWalkPrim w; memset(&w, 0, sizeof(w)); w.type = MTS_SHAPE_INSTANCE; w.shape = (int32_t) hs.instances.size(); w.index = group;
    memcpy(w.f, ds.to_object.m, 48);
    hs.walk.push_back(w); hs.area_pmf.push_back(0.f); hs.area_cdf.push_back(0.f);
    DInstance rec; memset(&rec, 0, sizeof(rec)); rec.to_world = ds.to_world; rec.to_object = ds.to_object; rec.group = group; rec.shape = i;
    hs.instances.push_back(rec); hs.instance_boxes.push_back(ib);
}
// The shapes of a description: the scene's own (instances among them) first, in declaration order -- they are the scene level's
// primitives [0, DScene::prim_count) -- then group by group the members' primitives, in group space.  A scene without groups gets
// exactly the records it always got.
static void build_shapes(const mts_scene_desc &d, const std::vector<int32_t> &member_of, const DefaultBsdfs &defaults, HostScene &hs) {
    DShape none; memset(&none, 0, sizeof(none));
    hs.shapes.assign((size_t) std::max(d.shape_count, 0), none);
    std::vector<int32_t> group_index((size_t) std::max(d.shape_count, 0), -1);
    for (int i = 0; i < d.shape_count; ++i)
        if (d.shapes[i].type == MTS_SHAPE_SHAPEGROUP) {
            DGroup g; memset(&g, 0, sizeof(g)); g.bbox = group_bbox(d, i); g.shape = i;
            group_index[(size_t) i] = (int32_t) hs.groups.size(); hs.groups.push_back(g);
            DShape &ds = hs.shapes[(size_t) i]; ds.type = MTS_SHAPE_SHAPEGROUP; ds.to_world = ds.to_object = xf_identity();
            ds.bsdf = defaults.plain; ds.interior = ds.exterior = ds.emitter = -1; ds.area_lo = ds.area_hi = -1;
            ds.bsdf_type = hs.bsdfs[(size_t) ds.bsdf].type; ds.bsdf_flags = hs.bsdfs[(size_t) ds.bsdf].flags;
        }
    for (int i = 0; i < d.shape_count; ++i) {
        if (member_of[(size_t) i] >= 0 || d.shapes[i].type == MTS_SHAPE_SHAPEGROUP) continue;
        if (d.shapes[i].type == MTS_SHAPE_INSTANCE) { const int g = group_index[(size_t) d.shapes[i].vertex_count]; add_instance(d, i, g, hs.groups[(size_t) g].bbox, defaults, hs); }
        else add_shape(d, i, defaults, hs, hs.scene.bbox);
    }
    hs.scene.prim_count = (int32_t) hs.prims.size();
    for (DGroup &g : hs.groups) {
        g.prim_first = (int32_t) hs.prims.size();
        DBBox gb; bbox_reset(gb);
        for (int m = g.shape + 1; m <= g.shape + d.shapes[g.shape].face_count; ++m) add_shape(d, m, defaults, hs, gb);
        g.prim_count = (int32_t) hs.prims.size() - g.prim_first;
        hs.shapes[(size_t) g.shape].prim_offset = g.prim_first;
    }
    hs.scene.instance_count = (int32_t) hs.instances.size(); hs.scene.group_count = (int32_t) hs.groups.size();
}
// the scene's bounding sphere, which set_scene hands to the emitters and the distant sensors (scene.cpp:95-97, bbox.h:329-332)
struct BSphere { float center[3], radius; };
static BSphere scene_bsphere(const DBBox &bbox) {
    const F3 c = (f3(bbox.max) + f3(bbox.min)) * .5f;
    return { { c.x, c.y, c.z }, pm_max(MTS_RAY_EPSILON, norm(c - f3(bbox.max)) * (1.f + MTS_RAY_EPSILON)) };
}
// emitters (scene.cpp:41-52; directional.cpp:68-73; constant.cpp:35-39)
static void build_emitters(const mts_scene_desc &d, bool spectral, const BSphere &bsphere, HostScene &hs) {
    hs.scene.environment = -1;
    for (int i = 0; i < d.emitter_count; ++i) {
        const mts_emitter &e = d.emitters[i];
        if (e.type == MTS_EMITTER_AREA) {
            check_index(e.shape, d.shape_count, "area emitter shape", false);
            if ((hs.shapes[e.shape].type == MTS_SHAPE_CUBE || hs.shapes[e.shape].type == MTS_SHAPE_MESH) && hs.shapes[e.shape].area_lo < 0)
                throw std::runtime_error("DiscreteDistribution: no probability mass found!");   // distr_1d.h:78-79
        } else if (e.type == MTS_EMITTER_CONSTANT) {
            if (hs.scene.environment >= 0) throw std::runtime_error("Only one environment emitter can be specified per scene.");
            hs.scene.environment = i;
        } else if (e.type != MTS_EMITTER_DIRECTIONAL && e.type != MTS_EMITTER_POINT) throw std::runtime_error("unknown emitter type");
        hs.emitters.push_back(build_emitter(e, bsphere.center, bsphere.radius));
        if (spectral) hs.emitter_sp.push_back(spectrum_index(d, e.radiance_spectrum, "an emitter"));
    }
}
// A sensor's own rectangle, disk or sphere (a distant sensor's target or ray origin), built outside the scene; `refusal`: for any other kind
static DShape build_sensor_shape(const mts_shape &shape, const std::string &refusal) {
    HostScene scratch; DBBox sb; int pc;
    if (shape.type != MTS_SHAPE_RECTANGLE && shape.type != MTS_SHAPE_SPHERE && shape.type != MTS_SHAPE_DISK) throw std::runtime_error(refusal);
    return build_shape(shape, scratch, sb, pc);
}
// The target of distant, distantflux (both "distant", key "ray_target") and mdistant (key "target"): none, a point, or a shape and its area
static void build_ray_target(const mts_sensor &s, const std::string &name, const char *key, DSensor &se) {
    se.target_type = s.distant_target_type;
    memcpy(se.target_point, s.distant_target_point, 12);
    if (se.target_type == MTS_DISTANT_TARGET_SHAPE) {
        const DShape &t = se.target_shape = build_sensor_shape(s.distant_target_shape, name + " " + key + " shape must be a rectangle, a disk or a sphere in this backend");
        se.target_area = t.type == MTS_SHAPE_DISK ? t.surface_area : t.type == MTS_SHAPE_RECTANGLE ? norm(cross(f3(t.frame_s), f3(t.frame_t)))
                                                                   : 4.f * MTS_PI * t.radius * t.radius;
    } else if (se.target_type != MTS_DISTANT_TARGET_NONE && se.target_type != MTS_DISTANT_TARGET_POINT)
        throw std::runtime_error(name + " sensor: unknown " + key + " type");
}
// What a sensor is built against -- the scene as created: its bounding sphere, the number of its media and the integrator's
// samples_per_pass.  mts_scene_create (sensor 0) and mts_scene_add_sensor (the others) run the same constructor.
struct SensorContext { BSphere bsphere; int32_t medium_count, samples_per_pass; };
// sensor, film, sampler.  Fills the filter table and the sub-sensor matrices next to the record it returns
static DSensor build_sensor(const mts_sensor &s, const SensorContext &cx, std::vector<float> &rfilter_values, std::vector<float> &multi_transforms) {
    const BSphere &bsphere = cx.bsphere;
    DSensor se; memset(&se, 0, sizeof(se));
    se.type = s.type; se.to_world = xf_from_abi(s.to_world);
    se.width = s.film_width; se.height = s.film_height;
    se.crop_x = s.crop_offset[0]; se.crop_y = s.crop_offset[1]; se.crop_w = s.crop_size[0]; se.crop_h = s.crop_size[1];
    if (se.width <= 0 || se.height <= 0 || se.crop_w <= 0 || se.crop_h <= 0 || se.crop_x < 0 || se.crop_y < 0 ||
        se.crop_x + se.crop_w > se.width || se.crop_y + se.crop_h > se.height) throw std::runtime_error("film: invalid size / crop window");
    se.rfilter = build_rfilter(s.rfilter_type, s.rfilter_radius, s.rfilter_stddev, rfilter_values);
    if (se.rfilter.radius > 16.f) throw std::runtime_error("reconstruction filter radius too large");
    if (s.sample_count <= 0) throw std::runtime_error("sampler: sample_count must be positive");
    se.sample_count = s.sample_count; se.seed = s.sampler_seed; se.medium = s.medium; se.shutter_open_time = s.shutter_open_time;
    se.wavefront = s.sampler_wavefront != 0;
    // (mts_render clamps samples_per_pass to sample_count as integrator.cpp:58-65 does: a larger value is one pass as well)
    if (se.wavefront && cx.samples_per_pass >= 0 && cx.samples_per_pass < s.sample_count)
        throw std::runtime_error("wavefront streams (mts_sensor.sampler_wavefront): samples_per_pass must cover the whole sample_count (one pass)");
    check_index(s.medium, cx.medium_count, "sensor medium", true);
    if (s.type == MTS_SENSOR_PERSPECTIVE) {
        se.near_clip = s.near_clip; se.far_clip = s.far_clip;
        float fsx = (float) se.width, fsy = (float) se.height;
        float rel_size_x = (float) se.crop_w / fsx, rel_size_y = (float) se.crop_h / fsy, rel_off_x = (float) se.crop_x / fsx, rel_off_y = (float) se.crop_y / fsy;
        float aspect = fsx / fsy;
        DXf c2s = xf_mul(xf_scale(f3(1.f / rel_size_x, 1.f / rel_size_y, 1.f)),
                  xf_mul(xf_translate(f3(-rel_off_x, -rel_off_y, 0.f)),
                  xf_mul(xf_scale(f3(-0.5f, -0.5f * aspect, 1.f)),
                  xf_mul(xf_translate(f3(-1.f, -1.f / aspect, 0.f)), xf_perspective(s.fov_x, s.near_clip, s.far_clip)))));
        DXf s2c = xf_inverse(c2s);                                                             // perspective.cpp:107-111
        memcpy(se.s2c, s2c.m, 64);
        se.ppo[0] = s.principal_point_offset[0] * ((float) se.width / (float) se.crop_w);      // perspective.cpp:101-106
        se.ppo[1] = s.principal_point_offset[1] * ((float) se.height / (float) se.crop_h);
        se.needs_aperture_sample = 0;                                                          // perspective.cpp:122
    } else if (s.type == MTS_SENSOR_DISTANT || s.type == MTS_SENSOR_DISTANTFLUX) {             // distant.cpp:225-297, distantflux.cpp:141-187
        se.direction_type = (se.width == 1 && se.height == 1) ? 0 : (se.height == 1 ? 1 : 2);
        se.flip_directions = s.distant_flip_directions != 0;
        build_ray_target(s, "distant", "ray_target", se);
        if (s.distant_origin_type != 0) {                                                      // distant.cpp:280-289, distantflux.cpp:172-184
            se.origin_type = 1;
            se.origin_shape = build_sensor_shape(s.distant_origin_shape, "distant sensor: the ray origin shape must be a rectangle, a disk or a sphere in this backend");
        }
        memcpy(se.bsphere_center, bsphere.center, 12); se.bsphere_radius = bsphere.radius;
        se.needs_aperture_sample = 1;                                                          // endpoint.h:244
    } else if (s.type == MTS_SENSOR_MRADIANCEMETER || s.type == MTS_SENSOR_MDISTANT) {        // mradiancemeter.cpp:72-132, mdistant.cpp:147-203
        if (s.multi_count <= 0 || s.multi_transforms == nullptr) throw std::runtime_error("multi-sensor: no sub-sensors given");
        if (se.width != s.multi_count || se.height != 1) throw std::runtime_error("Film size must be [sensor_count, 1].");
        multi_transforms.assign(s.multi_transforms, s.multi_transforms + 16 * (size_t) s.multi_count);
        se.multi_count = s.multi_count;
        se.needs_aperture_sample = s.type == MTS_SENSOR_MDISTANT ? 1 : 0;                        // m_needs_sample_3
        se.target_type = MTS_DISTANT_TARGET_NONE;
        if (s.type == MTS_SENSOR_MDISTANT) {
            build_ray_target(s, "mdistant", "target", se);
            memcpy(se.bsphere_center, bsphere.center, 12); se.bsphere_radius = bsphere.radius;   // mdistant.cpp:205-210
        }
    } else throw std::runtime_error("unknown sensor type");
    return se;
}
// A sensor's srf (perspective.cpp:113-121, radiancemeter.cpp:62-68): its index into hs.spectra, -1 for none.  spectrum_count: the
// description's own (two default spectra follow them in hs.spectra)
static int32_t build_sensor_srf(const mts_sensor &s, bool spectral, int32_t spectrum_count, const HostScene &hs) {
    if (!spectral || s.srf == 0) return -1;
    if (s.srf < 0 || s.srf > spectrum_count) throw std::runtime_error("index out of range: sensor srf");
    if (s.type != MTS_SENSOR_PERSPECTIVE && !(s.type == MTS_SENSOR_MRADIANCEMETER && s.multi_count == 1))
        throw std::runtime_error("srf: only perspective and radiancemeter sensors sample their wavelengths from a response function");
    const int t = hs.spectra[(size_t) s.srf - 1].type;
    if (t != MTS_SPECTRUM_UNIFORM && t != MTS_SPECTRUM_DISCRETE) throw std::runtime_error("srf: sample_spectrum is available for uniform and discrete spectra");
    return s.srf - 1;
}
// integrator (integrator.cpp:23-39,302-315), the wrappers around it, the film's channels and the sensor's response function
static void build_integrator(const mts_scene_desc &d, bool spectral, HostScene &hs) {
    DScene &sc = hs.scene;
    const mts_integrator &it = d.integrator;
    if (it.type != MTS_INTEGRATOR_PATH && it.type != MTS_INTEGRATOR_VOLPATH && it.type != MTS_INTEGRATOR_VOLPATHMIS) throw std::runtime_error("unknown integrator type");
    if (it.rr_depth <= 0) throw std::runtime_error("\"rr_depth\" must be set to a value greater than zero!");
    if (it.max_depth < 0 && it.max_depth != -1) throw std::runtime_error("\"max_depth\" must be set to -1 (infinite) or a value >= 0");
    // the regrouping kernel keeps a path's depth in 15 bits of its packed state dword (volpath_flat.h, HotStore::pack): a finite
    // bound beyond that could never trigger, so it is refused instead of being silently treated as infinite
    if (it.max_depth > 32767) throw std::runtime_error("\"max_depth\" must be -1 (infinite) or at most 32767 on this backend");
    sc.integrator.type = it.type; sc.integrator.max_depth = it.max_depth; sc.integrator.rr_depth = it.rr_depth; sc.integrator.hide_emitters = it.hide_emitters != 0;
    sc.integrator.use_spectral_mis = it.use_spectral_mis != 0;
    sc.integrator.monochrome = it.monochrome != 0;
    hs.integrator = it;
    hs.integrator.bin_lo = hs.integrator.bin_hi = nullptr;                                     // copied: the caller's arrays may go away
    // ---- moment (moment.cpp:27-58): six AOV channels around the nested integrator; rgb / mono only on this backend, never around the bins
    if (it.moment != 0) {
        if (it.moment != 1) throw std::runtime_error("integrator: \"moment\" must be 0 or 1");
        if (it.bin_mode != 0) throw std::runtime_error("the moment integrator cannot wrap nbins / bins (\"moment\" together with \"bin_mode\")");
        if (spectral) throw std::runtime_error("the moment integrator is not supported in the spectral variant");
    }
    // ---- nbins / bins (nbins.cpp:55-98, bins.cpp:23-85) and the sensor's srf (perspective.cpp:113-121, radiancemeter.cpp:62-68)
    sc.srf = -1; sc.bin_mode = 0; sc.bin_count = 0; sc.bin_lo = sc.bin_hi = nullptr; sc.film_channels = 5;
    if (it.bin_mode != 0) {
        if (!spectral) throw std::runtime_error("This integrator can only be used with a spectral variant!");
        if (it.bin_mode != 1 && it.bin_mode != 2) throw std::runtime_error("unknown bin mode");
        if (it.bin_count < 0 || it.bin_count > 64 || (it.bin_count > 0 && (!it.bin_lo || !it.bin_hi))) throw std::runtime_error("bins: between 0 and 64 bins with their bounds");
        hs.bin_lo.assign(it.bin_lo, it.bin_lo + it.bin_count); hs.bin_hi.assign(it.bin_hi, it.bin_hi + it.bin_count);
        if (it.bin_mode == 2)                                                                  // a uniform spectrum per bin (bins.cpp:79-84, uniform.cpp:41-46)
            for (int i = 0; i < it.bin_count; ++i) {
                hs.bin_lo[(size_t) i] = std::max(hs.bin_lo[(size_t) i], 280.f); hs.bin_hi[(size_t) i] = std::min(hs.bin_hi[(size_t) i], 2400.f);
                if (!(hs.bin_lo[(size_t) i] < hs.bin_hi[(size_t) i])) throw std::runtime_error("UniformSpectrum: 'lambda_min' must be less than 'lambda_max'");
            }
        sc.bin_mode = it.bin_mode; sc.bin_count = it.bin_count; sc.film_channels = 5 + 2 * it.bin_count;
    } else hs.integrator.bin_count = 0;
    if (it.moment != 0) sc.film_channels = 11;             // X, Y, Z, A, W, then the nested integrator's XYZ and its square (validated above)
    sc.srf = build_sensor_srf(d.sensor, spectral, d.spectrum_count, hs);
    hs.srf_lookup_by_wavelength = srf_lookup_by_wavelength(hs, sc.srf);
}

HostScene *build_host_scene(const mts_scene_desc *d) {
    if (!d) throw std::runtime_error("scene description is NULL");
    if (d->abi_version != MTS_ABI_VERSION) throw std::runtime_error("scene description: ABI version mismatch");
    std::unique_ptr<HostScene> hsp(new HostScene());
    HostScene &hs = *hsp; DScene &sc = hs.scene; memset(&sc, 0, sizeof(sc));
    const bool spectral = d->integrator.spectral != 0;
    if (d->shape_count < 0 || (d->shape_count > 0 && !d->shapes)) throw std::runtime_error("shapes: a negative count, or records missing");
    const std::vector<int32_t> member_of = validate_instancing(*d, spectral);      // groups and instances, ahead of every record
    hs.has_cone = validate_cones(*d, spectral);
    if (spectral) build_spectra(*d, hs);
    build_volumes(*d, spectral, hs);
    build_phases(*d, hs);
    build_media(*d, spectral, hs);
    const DefaultBsdfs defaults = build_bsdfs(*d, spectral, hs);
    build_textures(*d, spectral, hs);
    bbox_reset(sc.bbox);
    build_shapes(*d, member_of, defaults, hs);
    build_bvh(hs);
    const BSphere bsphere = scene_bsphere(sc.bbox);
    build_emitters(*d, spectral, bsphere, hs);
    sc.sensor = build_sensor(d->sensor, SensorContext{ bsphere, d->medium_count, d->integrator.samples_per_pass }, hs.rfilter_values, hs.multi_transforms);
    build_integrator(*d, spectral, hs);
    sc.volume_count = (int) hs.volumes.size(); sc.phase_count = (int) hs.phases.size(); sc.medium_count = (int) hs.media.size();
    sc.bsdf_count = (int) hs.bsdfs.size(); sc.shape_count = (int) hs.shapes.size();      // (prim_count: the scene level's primitives, build_shapes)
    sc.emitter_count = (int) hs.emitters.size();
    hs.traits = scene_traits(hs, spectral, sc.sensor);
    return hsp.release();
}

// ---------------------------------------------------------------- BVH
// A conservative acceleration structure: every node box is enlarged by a margin far above the rounding error of the slab
// test, so a primitive the exact tests would accept is never culled; the hit that wins is decided by the exact tests and
// the order-independent form of the reference's rule (closest t, ties to the later primitive), so results equal the walk
// over the primitive list bit for bit (which is what the CPU restatement does).
namespace {
struct PrimBox { float lo[3], hi[3], c[3]; int32_t prim; };
struct TmpNode { float lo[3], hi[3]; int left = -1, right = -1, first = 0, count = 0, depth = 0, final_index = -1; };
struct BvhBuilder {
    std::vector<PrimBox> &pb; std::vector<TmpNode> &tmp; std::vector<int32_t> &prims;
    int build(int begin, int end, int depth) {
        const int node = (int) tmp.size();
        tmp.emplace_back();
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY }, clo[3], chi[3];
        for (int a = 0; a < 3; ++a) { clo[a] = INFINITY; chi[a] = -INFINITY; }
        for (int i = begin; i < end; ++i) for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], pb[i].lo[a]); hi[a] = std::max(hi[a], pb[i].hi[a]);
            clo[a] = std::min(clo[a], pb[i].c[a]); chi[a] = std::max(chi[a], pb[i].c[a]);
        }
        const int count = end - begin;
        int axis = 0;
        for (int a = 1; a < 3; ++a) if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
        int left = -1, right = -1, first = 0, leaf_count = 0;
        const bool splittable = chi[axis] > clo[axis];
        if (count <= 4 || (!splittable && count <= 7)) {
            first = (int) prims.size(); leaf_count = count;
            for (int i = begin; i < end; ++i) prims.push_back(pb[i].prim);
        } else {
            const int mid = begin + count / 2;
            if (splittable)
                std::nth_element(pb.begin() + begin, pb.begin() + mid, pb.begin() + end,
                                 [axis](const PrimBox &x, const PrimBox &y) { return x.c[axis] < y.c[axis]; });
            left = build(begin, mid, depth + 1); right = build(mid, end, depth + 1);       // coincident centroids: split by index
        }
        TmpNode &n = tmp[(size_t) node];
        for (int a = 0; a < 3; ++a) { n.lo[a] = lo[a]; n.hi[a] = hi[a]; }
        n.left = left; n.right = right; n.first = first; n.count = leaf_count; n.depth = depth;
        return node;
    }
};
// Final layout: the top levels in breadth-first order (they are what the kernels stage in LDS), every subtree below them in
// depth-first order.  A node stores `skip` (where to go when its subtree is missed or done) and `link`: for a leaf
// (first << 3 | count) into bvh_prims, for an inner node minus the index of its left child; the right child is left.skip.
struct BvhLayout {
    std::vector<TmpNode> &tmp; int next = 0;
    void dfs(int n) { tmp[(size_t) n].final_index = next++; if (tmp[(size_t) n].left >= 0) { dfs(tmp[(size_t) n].left); dfs(tmp[(size_t) n].right); } }
    void assign(int root, int top_depth) {
        std::vector<int> level{ root }, below;
        while (!level.empty()) {
            std::vector<int> nxt;
            for (int n : level) {
                tmp[(size_t) n].final_index = next++;
                if (tmp[(size_t) n].left < 0) continue;
                if (tmp[(size_t) n].depth < top_depth) { nxt.push_back(tmp[(size_t) n].left); nxt.push_back(tmp[(size_t) n].right); }
                else { below.push_back(tmp[(size_t) n].left); below.push_back(tmp[(size_t) n].right); }
            }
            level.swap(nxt);
        }
        for (int n : below) dfs(n);
    }
    void emit(int n, int skip, float margin, std::vector<float> &out) {
        const TmpNode &t = tmp[(size_t) n];
        float *o = &out[8 * (size_t) t.final_index];
        for (int a = 0; a < 3; ++a) {
            o[a] = t.lo[a] - margin - 1e-6f * std::fabs(t.lo[a]);
            o[3 + a] = t.hi[a] + margin + 1e-6f * std::fabs(t.hi[a]);
        }
        const int32_t sk = skip;
        const int32_t link = t.left < 0 ? (int32_t) (((uint32_t) t.first << 3) | (uint32_t) t.count) : -(int32_t) tmp[(size_t) t.left].final_index;
        memcpy(&o[6], &sk, 4); memcpy(&o[7], &link, 4);
        if (t.left >= 0) { emit(t.left, tmp[(size_t) t.right].final_index, margin, out); emit(t.right, skip, margin, out); }
    }
};
}

// The BVH of one level: primitives [first, first + n) of prim order, appended to bvh_nodes / bvh_prims with absolute node and leaf
// indices.  `diag`: the diagonal of the level's bounding box, which scales the margin.  Returns the number of nodes (0: the list is walked).
static int32_t build_bvh_level(HostScene &hs, int first, int n, F3 diag, int threshold) {
    if (n <= threshold) return 0;
    std::vector<PrimBox> pb((size_t) n);
    for (int i = 0; i < n; ++i) {
        const DPrim &pr = hs.prims[(size_t) (first + i)]; const DShape &s = hs.shapes[(size_t) pr.shape];
        PrimBox b; b.prim = first + i;
        for (int a = 0; a < 3; ++a) { b.lo[a] = INFINITY; b.hi[a] = -INFINITY; }
        auto add = [&b](F3 p) { const float v[3] = { p.x, p.y, p.z }; for (int a = 0; a < 3; ++a) { b.lo[a] = std::min(b.lo[a], v[a]); b.hi[a] = std::max(b.hi[a], v[a]); } };
        if (s.type == MTS_SHAPE_RECTANGLE || s.type == MTS_SHAPE_DISK) {
            for (int k = 0; k < 4; ++k) add(mat_point_affine(s.to_world.m, f3((k & 1) ? 1.f : -1.f, (k & 2) ? 1.f : -1.f, 0.f)));
        } else if (s.type == MTS_SHAPE_SPHERE) {
            add(f3(s.center) - f3s(s.radius)); add(f3(s.center) + f3s(s.radius));
        } else if (s.type == MTS_SHAPE_CONE) {
            const DBBox cb = cone_bbox(s); add(f3(cb.min)); add(f3(cb.max));
        } else if (s.type == MTS_SHAPE_INSTANCE) {                            // the instance's own box (instance.cpp:81-92)
            const DBBox &ib = hs.instance_boxes[(size_t) hs.walk[(size_t) (first + i)].shape];
            // an instance of an empty group has no box (instance.cpp:84-86): it gets the point of its translation, finite, so that
            // no NaN centroid reaches the builder; the traversal finds nothing inside it
            if (ib.min[0] <= ib.max[0] && ib.min[1] <= ib.max[1] && ib.min[2] <= ib.max[2]) { add(f3(ib.min)); add(f3(ib.max)); }
            else add(f3(s.to_world.m[3], s.to_world.m[7], s.to_world.m[11]));
        } else {
            const float *t = &hs.tri[9 * (size_t) (first + i)];
            F3 p0 = f3(t), e1 = f3(t + 3), e2 = f3(t + 6);
            add(p0); add(p0 + e1); add(p0 + e2);
        }
        for (int a = 0; a < 3; ++a) b.c[a] = .5f * (b.lo[a] + b.hi[a]);
        pb[(size_t) i] = b;
    }
    std::vector<TmpNode> tmp;
    std::vector<int32_t> leaves;
    BvhBuilder bb{ pb, tmp, leaves };
    const int root = bb.build(0, n, 0);
    BvhLayout layout{ tmp };
    layout.assign(root, MTS_BVH_TOP_DEPTH);
    std::vector<float> nodes(8 * tmp.size(), 0.f);
    layout.emit(root, (int) tmp.size(), 1e-5f * norm(diag) + 1e-7f, nodes);
    const int32_t node_base = (int32_t) (hs.bvh_nodes.size() / 8), leaf_base = (int32_t) hs.bvh_prims.size();
    if (node_base != 0 || leaf_base != 0)                                      // behind another level: the indices become absolute
        for (size_t k = 0; k < tmp.size(); ++k) {
            int32_t skip, link; memcpy(&skip, &nodes[8 * k + 6], 4); memcpy(&link, &nodes[8 * k + 7], 4);
            skip += node_base;
            link = link < 0 ? link - node_base : (int32_t) (((uint32_t) ((link >> 3) + leaf_base) << 3) | (uint32_t) (link & 7));
            memcpy(&nodes[8 * k + 6], &skip, 4); memcpy(&nodes[8 * k + 7], &link, 4);
        }
    hs.bvh_nodes.insert(hs.bvh_nodes.end(), nodes.begin(), nodes.end());
    hs.bvh_prims.insert(hs.bvh_prims.end(), leaves.begin(), leaves.end());
    return (int32_t) tmp.size();
}

void build_bvh(HostScene &hs) {
    hs.bvh_nodes.clear(); hs.bvh_prims.clear(); hs.scene.bvh_node_count = 0;
    int threshold = 40;                                                    // at or below this the scalar walk over the list is faster (measured: 31 primitives 584 vs 562 Msamples/s)
    if (const char *e = getenv("MTSAMD_BVH_THRESHOLD")) threshold = atoi(e);
    // the scene level first: its top levels are what the kernels stage in LDS; then every group's, by the same rule on its own count
    hs.scene.bvh_node_count = build_bvh_level(hs, 0, hs.scene.prim_count, f3(hs.scene.bbox.max) - f3(hs.scene.bbox.min), threshold);
    for (DGroup &g : hs.groups) {
        g.node_first = (int32_t) (hs.bvh_nodes.size() / 8);
        g.node_count = build_bvh_level(hs, g.prim_first, g.prim_count, f3(g.bbox.max) - f3(g.bbox.min), threshold);
    }
}

// ---------------------------------------------------------------- upload
#define HIP_CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

template <typename T> static const T *upload(HostScene &hs, const std::vector<T> &v) {
    void *p = nullptr;
    size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_CHECK(hipMalloc(&p, bytes));
    hs.device_allocs.push_back(p);
    if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return (const T *) p;
}

void upload_host_scene(HostScene &hs, int device) {
    HIP_CHECK(hipSetDevice(device));
    hs.device = device;
    for (size_t i = 0; i < hs.volumes.size(); ++i)
        if (hs.volumes[i].type == MTS_VOLUME_GRID) hs.volumes[i].data = upload(hs, hs.grid_data[i]);
    for (size_t i = 0; i < hs.phases.size(); ++i)
        if (hs.phases[i].type == MTS_PHASE_TABULATED) { hs.phases[i].pdf = upload(hs, hs.tab_pdf[i]); hs.phases[i].cdf = upload(hs, hs.tab_cdf[i]); }
    for (size_t i = 0; i < hs.media.size(); ++i)
        if (!hs.pair_data[i].empty()) hs.media[i].pair_grid = upload(hs, hs.pair_data[i]);
    DScene &sc = hs.scene;
    sc.volumes = upload(hs, hs.volumes); sc.phases = upload(hs, hs.phases); sc.media = upload(hs, hs.media);
    sc.bsdfs = upload(hs, hs.bsdfs); sc.shapes = upload(hs, hs.shapes); sc.prims = upload(hs, hs.prims); sc.walk = upload(hs, hs.walk);
    sc.emitters = upload(hs, hs.emitters);
    sc.positions = upload(hs, hs.positions); sc.normals = upload(hs, hs.normals); sc.texcoords = upload(hs, hs.texcoords);
    sc.faces = upload(hs, hs.faces);
    sc.tri = upload(hs, hs.tri);
    sc.tri_attr = upload(hs, hs.tri_attr);
    sc.area_pmf = upload(hs, hs.area_pmf); sc.area_cdf = upload(hs, hs.area_cdf);
    sc.bvh_nodes = nullptr; sc.bvh_prims = nullptr; sc.bvh_lds = nullptr; sc.bvh_lds_count = 0;
    if (!hs.bvh_nodes.empty()) { sc.bvh_nodes = upload(hs, hs.bvh_nodes); sc.bvh_prims = upload(hs, hs.bvh_prims); }
    sc.sensor.rfilter.values = upload(hs, hs.rfilter_values);
    sc.sensor.multi = upload(hs, hs.multi_transforms);
    sc.textures = nullptr; sc.bsdf_tex = nullptr;
    if (!hs.bsdf_tex.empty()) {
        for (size_t i = 0; i < hs.textures.size(); ++i)
            if (hs.textures[i].type == MTS_TEXTURE_BITMAP) hs.textures[i].data = upload(hs, hs.texels[i]);
        sc.textures = upload(hs, hs.textures); sc.bsdf_tex = upload(hs, hs.bsdf_tex);
    }
    sc.instances = nullptr; sc.groups = nullptr;
    // (a scene with a cone and no instance: both arrays empty, both pointers set -- a non-NULL `instances` is what sends mts_sample and
    // mts_ray_intersect to the INST kernels, kernels.hip: launch_sample; no walk record names an instance or a group)
    if (!hs.instances.empty() || hs.has_cone) { sc.instances = upload(hs, hs.instances); sc.groups = upload(hs, hs.groups); }
    sc.spectra = nullptr; sc.bsdf_sp = nullptr; sc.emitter_sp = nullptr; sc.volume_sp = nullptr; sc.cie = nullptr;
    if (hs.integrator.spectral) {
        for (size_t i = 0; i < hs.spectra.size(); ++i)
            if (hs.spectra[i].type != MTS_SPECTRUM_UNIFORM) {
                hs.spectra[i].values = upload(hs, hs.spectrum_values[i]);
                if (!hs.spectrum_wavelengths[i].empty()) hs.spectra[i].wavelengths = upload(hs, hs.spectrum_wavelengths[i]);
                if (!hs.spectrum_cdf[i].empty()) hs.spectra[i].cdf = upload(hs, hs.spectrum_cdf[i]);
            }
        sc.spectra = upload(hs, hs.spectra); sc.bsdf_sp = upload(hs, hs.bsdf_sp); sc.emitter_sp = upload(hs, hs.emitter_sp);
        sc.volume_sp = upload(hs, hs.volume_sp);
        sc.cie = upload(hs, std::vector<float>(MTS_CIE1931_XYZ, MTS_CIE1931_XYZ + 285));
        if (sc.bin_count > 0) { sc.bin_lo = upload(hs, hs.bin_lo); sc.bin_hi = upload(hs, hs.bin_hi); }
    }
    HIP_CHECK(hipDeviceSynchronize());
    hs.uploaded = true;
}

void free_host_scene(HostScene *hs) {
    if (!hs) return;
    if (hs->uploaded) { (void) hipSetDevice(hs->device); for (void *p : hs->device_allocs) (void) hipFree(p); }
    delete hs;
}

// ---------------------------------------------------------------- further sensors (mts_scene_add_sensor)
// Sensor 0's constructor against the scene as created; everything is validated and built before the scene is touched.  The device
// tables of an uploaded scene join device_allocs: they keep their addresses until free_host_scene.
int32_t add_host_sensor(HostScene &hs, const mts_sensor *s) {
    if (!s) throw std::runtime_error("mts_scene_add_sensor: sensor is NULL");
    const bool spectral = hs.integrator.spectral != 0;
    HostSensor rec;
    try {
        const SensorContext cx = { scene_bsphere(hs.scene.bbox), (int32_t) hs.media.size(), hs.integrator.samples_per_pass };
        rec.sensor = build_sensor(*s, cx, rec.rfilter_values, rec.multi_transforms);
        rec.srf = build_sensor_srf(*s, spectral, spectral ? (int32_t) hs.spectra.size() - 2 : 0, hs);
        rec.srf_lookup_by_wavelength = srf_lookup_by_wavelength(hs, rec.srf);
    } catch (const std::runtime_error &e) { throw std::runtime_error(std::string("mts_scene_add_sensor: ") + e.what()); }
    if (hs.uploaded) {
        HIP_CHECK(hipSetDevice(hs.device));
        rec.sensor.rfilter.values = upload(hs, rec.rfilter_values);
        rec.sensor.multi = upload(hs, rec.multi_transforms);
    }
    hs.extra_sensors.push_back(std::move(rec));
    hs.sensor_count.store(1 + (int) hs.extra_sensors.size());
    return (int32_t) hs.extra_sensors.size();
}

SensorView host_sensor(const HostScene &hs, int32_t index) {
    const int32_t n = 1 + (int32_t) hs.extra_sensors.size();
    if (index < 0 || index >= n) throw std::runtime_error("sensor index " + std::to_string(index) + " is out of range (the scene has " + std::to_string(n) + (n == 1 ? " sensor)" : " sensors)"));
    const bool spectral = hs.integrator.spectral != 0;
    if (index == 0) return { &hs.scene.sensor, hs.scene.srf, hs.srf_lookup_by_wavelength, scene_traits(hs, spectral, hs.scene.sensor) };
    const HostSensor &x = hs.extra_sensors[(size_t) index - 1];
    return { &x.sensor, x.srf, x.srf_lookup_by_wavelength, scene_traits(hs, spectral, x.sensor) };
}

// ---------------------------------------------------------------- update (mts_scene_update)
namespace {
[[noreturn]] void refuse(const char *object, int index, const std::string &what) {
    throw std::runtime_error("mts_scene_update: " + std::string(object) + " " + std::to_string(index) + ": " + what);
}
[[noreturn]] void frozen(const char *object, int index, const char *field) {
    refuse(object, index, std::string("'") + field + "' differs from what the scene was created with (the topology of a scene is frozen)");
}
struct StagedSpectrum { DSpectrum rec; SpectrumArrays arrays; };
struct StagedPhase { DPhase rec; std::vector<float> pdf, cdf; };
// a medium's description as it was given, read back from its record (media that follow a dirty volume without being dirty themselves)
mts_medium medium_desc_of(const DMedium &m) {
    mts_medium d; memset(&d, 0, sizeof(d));
    d.type = m.type; d.sigma_t_volume = m.sigma_t; d.albedo_volume = m.albedo; d.scale = m.scale; d.phase = m.phase;
    d.sample_emitters = m.sample_emitters; d.has_spectral_extinction = m.has_spectral_extinction;
    return d;
}
#if !defined(MTSAMD_HOST_ONLY)
template <typename T> void reupload(const T *device, const std::vector<T> &v, hipStream_t stream) {
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync((void *) device, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
}
#endif
} // namespace

void update_host_scene(HostScene &hs, const mts_scene_desc *d, const mts_dirty *dirty, int32_t n, hipStream_t stream) {
    if (!d) throw std::runtime_error("mts_scene_update: scene description is NULL");
    if (d->abi_version != MTS_ABI_VERSION) throw std::runtime_error("mts_scene_update: scene description: ABI version mismatch");
    if (n < 0) throw std::runtime_error("mts_scene_update: n is negative");
    if (n > 0 && !dirty) throw std::runtime_error("mts_scene_update: dirty is NULL");
    const bool spectral = hs.integrator.spectral != 0;
    // the description's own counts (build_host_scene appends two default BSDFs and, in the spectral variant, their two spectra)
    const int32_t n_volumes = (int32_t) hs.volumes.size(), n_phases = (int32_t) hs.phases.size(), n_media = (int32_t) hs.media.size(),
                  n_bsdfs = (int32_t) hs.bsdfs.size() - 2, n_emitters = (int32_t) hs.emitters.size(), n_spectra = spectral ? (int32_t) hs.spectra.size() - 2 : 0,
                  n_textures = (int32_t) hs.textures.size();
    if ((d->integrator.spectral != 0) != spectral || (d->integrator.monochrome != 0) != (hs.scene.integrator.monochrome != 0))
        throw std::runtime_error("mts_scene_update: the description is of another variant than the scene");
    if (d->volume_count != n_volumes || d->phase_count != n_phases || d->medium_count != n_media || d->bsdf_count != n_bsdfs ||
        d->emitter_count != n_emitters || (spectral && d->spectrum_count != n_spectra) || d->texture_count != n_textures)
        throw std::runtime_error("mts_scene_update: the description's record counts differ from what the scene was created with");

    // ---- 1. validate and stage: nothing of the scene is written before every dirty record has passed
    std::map<int, StagedSpectrum> spectra; std::map<int, StagedPhase> phases; std::map<int, DBsdf> bsdfs; std::map<int, DEmitter> emitters;
    std::map<int, std::pair<DTexture, std::vector<float>>> textures;
    std::map<int, const float *> volumes;                  // dirty volume -> mts_dirty::device_data
    std::set<int> media;
    for (int32_t k = 0; k < n; ++k) {
        const int i = dirty[k].index;
        static const char *NAMES[] = { "spectrum", "volume", "phase", "medium", "bsdf", "emitter", "texture" };
        const int32_t counts[] = { n_spectra, n_volumes, n_phases, n_media, n_bsdfs, n_emitters, n_textures };
        if (dirty[k].object < MTS_OBJ_SPECTRUM || dirty[k].object > MTS_OBJ_TEXTURE) throw std::runtime_error("mts_scene_update: dirty[" + std::to_string(k) + "]: unknown object kind");
        const char *name = NAMES[dirty[k].object];
        if (i < 0 || i >= counts[dirty[k].object]) refuse(name, i, "index out of range");
        if (dirty[k].device_data && !(dirty[k].object == MTS_OBJ_VOLUME && hs.volumes[(size_t) i].type == MTS_VOLUME_GRID))
            refuse(name, i, "device_data is for grid volumes only");
        switch (dirty[k].object) {
        case MTS_OBJ_SPECTRUM: {
            const mts_spectrum &sp = d->spectra[i]; const DSpectrum &old = hs.spectra[(size_t) i];
            if (sp.type != old.type) frozen(name, i, "type");
            if (sp.type != MTS_SPECTRUM_UNIFORM && sp.count != old.count) frozen(name, i, "count");
            StagedSpectrum &st = spectra[i]; st.arrays = SpectrumArrays();
            st.rec = build_spectrum(sp, st.arrays);
            break; }
        case MTS_OBJ_VOLUME: {
            const mts_volume &v = d->volumes[i]; const DVolume &old = hs.volumes[(size_t) i]; const DVolumeSp &osp = hs.volume_sp[(size_t) i];
            if (dirty[k].device_data && !hs.uploaded) refuse(name, i, "device_data needs a scene in device memory");
            if ((v.type == MTS_VOLUME_GRID_SPECTRAL ? MTS_VOLUME_GRID : v.type) != old.type || (v.type == MTS_VOLUME_GRID_SPECTRAL) != (osp.spectral_grid != 0)) frozen(name, i, "type");
            if (volume_is_grid(v)) {
                if (v.nx != old.nx) frozen(name, i, "nx");
                if (v.ny != old.ny) frozen(name, i, "ny");
                if (v.nz != old.nz) frozen(name, i, "nz");
                if (v.channels != old.channels) frozen(name, i, "channels");
                if (v.filter_type != old.filter) frozen(name, i, "filter_type");
                if (v.wrap_mode != old.wrap) frozen(name, i, "wrap_mode");
            }
            const GridStats none = { 0.f, 0 };
            DVolume dv; DVolumeSp vsp;
            build_volume(v, spectral, n_spectra, dirty[k].device_data == nullptr, &none, dv, vsp);
            if (memcmp(dv.w2l, old.w2l, 64) != 0) frozen(name, i, "to_world");
            if (vsp.value_sp != osp.value_sp) frozen(name, i, "value_spectrum");
            if (vsp.lambda_min != osp.lambda_min) frozen(name, i, "lambda_min");
            if (vsp.lambda_max != osp.lambda_max) frozen(name, i, "lambda_max");
            volumes[i] = dirty[k].device_data;
            break; }
        case MTS_OBJ_PHASE: {
            const mts_phase &p = d->phases[i]; const DPhase &old = hs.phases[(size_t) i];
            if (p.type != old.type) frozen(name, i, "type");
            if (p.type == MTS_PHASE_BLEND && (p.child[0] != old.child[0] || p.child[1] != old.child[1])) frozen(name, i, "child");
            if (p.type == MTS_PHASE_BLEND && p.weight_volume != old.weight_volume) frozen(name, i, "weight_volume");
            if (p.type == MTS_PHASE_TABULATED && p.tab_count != old.size) frozen(name, i, "tab_count");
            StagedPhase &st = phases[i]; st.pdf.clear(); st.cdf.clear();
            try { st.rec = build_phase(p, i, hs.phases, n_phases, n_volumes, st.pdf, st.cdf); }
            catch (const std::runtime_error &e) { refuse(name, i, std::string(p.type == MTS_PHASE_HG ? "'g': " : p.type == MTS_PHASE_TABULATED ? "'tab_values': " : "") + e.what()); }
            break; }
        case MTS_OBJ_MEDIUM: {
            const mts_medium &m = d->media[i]; const DMedium &old = hs.media[(size_t) i];
            if (m.type != old.type) frozen(name, i, "type");
            if (m.sigma_t_volume != old.sigma_t) frozen(name, i, "sigma_t_volume");
            if (m.albedo_volume != old.albedo) frozen(name, i, "albedo_volume");
            if (m.phase != old.phase) frozen(name, i, "phase");
            media.insert(i);
            break; }
        case MTS_OBJ_BSDF: {
            const mts_bsdf &b = d->bsdfs[i];
            if (b.type != hs.bsdfs[(size_t) i].type) frozen(name, i, "type");
            if (spectral)
                for (int s = 0; s < MTS_BSDF_SP_COUNT; ++s)
                    if (BSDF_SP_USED[b.type][s] && b.spectrum[s] != hs.bsdf_sp[(size_t) i * MTS_BSDF_SP_COUNT + s]) frozen(name, i, "spectrum");
            if (!hs.bsdf_tex.empty()) {
                int32_t t[MTS_BSDF_SP_COUNT]; bsdf_texture_indices(*d, i, t);
                if (memcmp(t, &hs.bsdf_tex[(size_t) i * MTS_BSDF_SP_COUNT], sizeof(t)) != 0) frozen(name, i, "bsdf_textures");
            }
            try { bsdfs[i] = build_bsdf(b); }
            catch (const std::runtime_error &e) { refuse(name, i, e.what()); }
            if (b.type == MTS_BSDF_BLEND || b.type == MTS_BSDF_TWOSIDED) {     // the children are topology; their types are frozen too, so the flags stay
                const DBsdf &old = hs.bsdfs[(size_t) i];
                const bool two = b.type == MTS_BSDF_TWOSIDED;
                if (b.spectrum[0] != blend_child(old, 0)) frozen(name, i, two ? "spectrum[0] (brdf_0)" : "spectrum[0] (bsdf_0)");
                if (b.spectrum[1] != blend_child(old, 1)) frozen(name, i, two ? "spectrum[1] (brdf_1)" : "spectrum[1] (bsdf_1)");
                bsdfs[i].flags = old.flags;
            }
            break; }
        case MTS_OBJ_TEXTURE: {                                // new texels / checkerboard colours (bitmap.cpp:562-564, checkerboard.cpp:92-96)
            if (!d->textures) refuse(name, i, "the description holds no texture records");
            const mts_texture &t = d->textures[i]; const DTexture &old = hs.textures[(size_t) i];
            if (t.type != old.type) frozen(name, i, "type");
            if (t.type == MTS_TEXTURE_BITMAP) {
                if (t.width != old.width) frozen(name, i, "width");
                if (t.height != old.height) frozen(name, i, "height");
                if (t.channels != old.channels) frozen(name, i, "channels");
                if (t.filter_type != old.filter) frozen(name, i, "filter_type");
                if (t.wrap_mode != old.wrap) frozen(name, i, "wrap_mode");
            }
            if (memcmp(t.to_uv, old.to_uv, sizeof(old.to_uv)) != 0) frozen(name, i, "to_uv");
            std::pair<DTexture, std::vector<float>> &st = textures[i]; st.second.clear();
            try { st.first = build_texture(t, i, hs.scene.integrator.monochrome != 0, true, st.second); }
            catch (const std::runtime_error &e) { refuse(name, i, e.what()); }
            break; }
        default: {
            const mts_emitter &e = d->emitters[i]; const DEmitter &old = hs.emitters[(size_t) i];
            if (e.type != old.type) frozen(name, i, "type");
            if (e.shape != old.shape) frozen(name, i, "shape");
            if (spectral && e.radiance_spectrum != hs.emitter_sp[(size_t) i]) frozen(name, i, "radiance_spectrum");
            const DXf xf = xf_from_abi(e.to_world);          // an emitter's placement is geometry: frozen like a volume's transform
            if (memcmp(&xf, &old.to_world, sizeof(xf)) != 0) frozen(name, i, "to_world");
            emitters[i] = build_emitter(e, old.bsphere_center, old.bsphere_radius);
            break; }
        }
    }
    for (int i = 0; i < n_media; ++i)                      // media follow the volumes they read
        if (volumes.count(hs.media[(size_t) i].sigma_t) || volumes.count(hs.media[(size_t) i].albedo)) media.insert(i);

    // ---- 2. the new grids and what the constructors derive from their data
    std::map<int, GridStats> stats;
#if !defined(MTSAMD_HOST_ONLY)
    if (hs.uploaded) {
        HIP_CHECK(hipSetDevice(hs.device));
        int cus = 0;
        HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hs.device));
        std::vector<int> grids;
        for (const auto &kv : volumes) if (hs.volumes[(size_t) kv.first].type == MTS_VOLUME_GRID) grids.push_back(kv.first);
        std::vector<uint32_t> words(2 * grids.size());
        if (!grids.empty()) {
            if (!hs.update_stats) {                        // first use: two words per volume of the scene
                void *p = nullptr;
                HIP_CHECK(hipMalloc(&p, std::max<size_t>(2 * sizeof(uint32_t) * hs.volumes.size(), 16)));
                hs.device_allocs.push_back(p); hs.update_stats = (uint32_t *) p;
            }
            for (size_t g = 0; g < grids.size(); ++g) { words[2 * g] = 0u; words[2 * g + 1] = 1u; }
            HIP_CHECK(hipMemcpyAsync(hs.update_stats, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            for (int v : grids) {                          // the scene owns its copy of the data: into the grid's own allocation first
                const float *src = volumes[v] ? volumes[v] : d->volumes[v].data;
                if (src != hs.volumes[(size_t) v].data)
                    HIP_CHECK(hipMemcpyAsync((void *) hs.volumes[(size_t) v].data, src, hs.grid_data[(size_t) v].size() * sizeof(float), volumes[v] ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
            }
            // one pass per dirty grid: its statistics, fused with the pair grid of a medium that interleaves it (a medium with both grids
            // dirty is written by its sigma_t's pass; further media sharing the grid get a pass without statistics)
            for (size_t g = 0; g < grids.size(); ++g) {
                const DVolume &dv = hs.volumes[(size_t) grids[g]];
                GridUpdateJob job; memset(&job, 0, sizeof(job));
                job.grid = dv.data; job.count = (uint32_t) hs.grid_data[(size_t) grids[g]].size(); job.channels = (uint32_t) dv.channels;
                job.plane = (uint32_t) dv.ny * (uint32_t) dv.nx * (uint32_t) dv.channels; job.nx = (uint32_t) dv.nx;
                job.stats = hs.update_stats + 2 * g;
                bool launched = false;
                for (int m : media) {
                    const DMedium &dm = hs.media[(size_t) m];
                    if (hs.pair_data[(size_t) m].empty() || (dm.sigma_t != grids[g] && dm.albedo != grids[g])) continue;
                    if (dm.albedo == grids[g] && dm.sigma_t != grids[g] && volumes.count(dm.sigma_t)) continue;      // its sigma_t's pass writes it
                    job.pair = (float *) dm.pair_grid; job.slot = dm.sigma_t == grids[g] ? 0u : 1u;
                    job.partner = hs.volumes[(size_t) (job.slot == 0 ? dm.albedo : dm.sigma_t)].data;
                    HIP_CHECK(launch_grid_update(job, cus, stream));
                    job.stats = nullptr; launched = true;
                }
                if (!launched) HIP_CHECK(launch_grid_update(job, cus, stream));
            }
            HIP_CHECK(hipMemcpyAsync(words.data(), hs.update_stats, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        for (size_t g = 0; g < grids.size(); ++g) stats[grids[g]] = GridStats{ grid_key_to_float(words[2 * g]), words[2 * g + 1] != 0u ? 1 : 0 };
    } else
#endif
    for (const auto &kv : volumes) {
        const mts_volume &v = d->volumes[kv.first];
        if (!volume_is_grid(v)) continue;
        stats[kv.first] = grid_stats(v.data, v.nx, v.ny, v.nz, v.channels);
        hs.grid_data[(size_t) kv.first].assign(v.data, v.data + hs.grid_data[(size_t) kv.first].size());
    }

    // ---- 3. the records, through the constructors' own functions; device pointers stay
    for (const auto &kv : volumes) {
        const size_t i = (size_t) kv.first;
        DVolume dv; DVolumeSp vsp;
        build_volume(d->volumes[i], spectral, n_spectra, false, stats.count(kv.first) ? &stats[kv.first] : nullptr, dv, vsp);
        dv.data = hs.volumes[i].data;
        hs.volumes[i] = dv; hs.volume_sp[i] = vsp;
    }
    for (auto &kv : phases) {
        const size_t i = (size_t) kv.first;
        kv.second.rec.pdf = hs.phases[i].pdf; kv.second.rec.cdf = hs.phases[i].cdf;
        hs.phases[i] = kv.second.rec; hs.tab_pdf[i].swap(kv.second.pdf); hs.tab_cdf[i].swap(kv.second.cdf);
    }
    for (int i : media) {
        const bool listed = std::any_of(dirty, dirty + n, [i](const mts_dirty &q) { return q.object == MTS_OBJ_MEDIUM && q.index == i; });
        const mts_medium m = listed ? d->media[i] : medium_desc_of(hs.media[(size_t) i]);
        DMedium dm;
        const bool pair = build_medium(m, hs, n_volumes, n_phases, spectral, dm);
        dm.pair_grid = hs.media[(size_t) i].pair_grid;
        hs.media[(size_t) i] = dm;
        if (pair && !hs.uploaded) build_pair_grid(hs.volumes[(size_t) dm.sigma_t], hs.grid_data[(size_t) dm.sigma_t], hs.grid_data[(size_t) dm.albedo], hs.pair_data[(size_t) i]);
    }
    for (const auto &kv : bsdfs) hs.bsdfs[(size_t) kv.first] = kv.second;
    for (auto &kv : textures) {
        const size_t i = (size_t) kv.first;
        kv.second.first.data = hs.textures[i].data;
        hs.textures[i] = kv.second.first; hs.texels[i].swap(kv.second.second);
    }
    for (const auto &kv : emitters) hs.emitters[(size_t) kv.first] = kv.second;
    for (auto &kv : spectra) {
        const size_t i = (size_t) kv.first;
        DSpectrum &ds = kv.second.rec;
        ds.values = hs.spectra[i].values; ds.wavelengths = hs.spectra[i].wavelengths; ds.cdf = hs.spectra[i].cdf;
        hs.spectra[i] = ds;
        hs.spectrum_values[i].swap(kv.second.arrays.values); hs.spectrum_wavelengths[i].swap(kv.second.arrays.wavelengths); hs.spectrum_cdf[i].swap(kv.second.arrays.cdf);
    }
    hs.srf_lookup_by_wavelength = srf_lookup_by_wavelength(hs, hs.scene.srf);
    for (HostSensor &x : hs.extra_sensors) x.srf_lookup_by_wavelength = srf_lookup_by_wavelength(hs, x.srf);      // a dirty spectrum may be any sensor's srf
    hs.traits = scene_traits(hs, spectral, hs.scene.sensor);       // the next render picks the kernel a fresh scene would (the other sensors': host_sensor)

    // ---- 4. the device's copies of what changed
#if !defined(MTSAMD_HOST_ONLY)
    if (hs.uploaded) {
        const DScene &sc = hs.scene;
        if (!volumes.empty()) { reupload(sc.volumes, hs.volumes, stream); if (spectral) reupload(sc.volume_sp, hs.volume_sp, stream); }
        if (!media.empty()) reupload(sc.media, hs.media, stream);
        if (!bsdfs.empty()) reupload(sc.bsdfs, hs.bsdfs, stream);
        if (!emitters.empty()) reupload(sc.emitters, hs.emitters, stream);
        for (const auto &kv : textures) if (hs.textures[(size_t) kv.first].type == MTS_TEXTURE_BITMAP) reupload(hs.textures[(size_t) kv.first].data, hs.texels[(size_t) kv.first], stream);
        if (!textures.empty()) reupload(sc.textures, hs.textures, stream);
        for (const auto &kv : phases) {
            const size_t i = (size_t) kv.first;
            if (hs.phases[i].type == MTS_PHASE_TABULATED) { reupload(hs.phases[i].pdf, hs.tab_pdf[i], stream); reupload(hs.phases[i].cdf, hs.tab_cdf[i], stream); }
        }
        if (!phases.empty()) reupload(sc.phases, hs.phases, stream);
        for (const auto &kv : spectra) {
            const size_t i = (size_t) kv.first;
            if (hs.spectra[i].type == MTS_SPECTRUM_UNIFORM) continue;
            reupload(hs.spectra[i].values, hs.spectrum_values[i], stream);
            if (hs.spectra[i].wavelengths) reupload(hs.spectra[i].wavelengths, hs.spectrum_wavelengths[i], stream);
            if (hs.spectra[i].cdf) reupload(hs.spectra[i].cdf, hs.spectrum_cdf[i], stream);
        }
        if (!spectra.empty()) reupload(sc.spectra, hs.spectra, stream);
        HIP_CHECK(hipStreamSynchronize(stream));
    }
#else
    (void) stream;
#endif
}

// ---------------------------------------------------------------- digest (tests: "the device scene is the fresh one", "the host scene is the parent's")
namespace {
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(const void *p, size_t bytes) { const unsigned char *c = (const unsigned char *) p; for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 1099511628211ull; } }
    template <typename T> void add(const std::vector<T> &v) { add(v.data(), v.size() * sizeof(T)); }
};
// Where the walk takes an array from: the device's copy (as many elements as the host's vector holds), or the host's vector itself
struct DigestSource {
    bool device;
    template <typename T> std::vector<T> operator()(const T *device_copy, const std::vector<T> &host) const {
        if (!device) return host;
        std::vector<T> v(host.size());
#if !defined(MTSAMD_HOST_ONLY)
        if (!v.empty() && device_copy) HIP_CHECK(hipMemcpy(v.data(), device_copy, v.size() * sizeof(T), hipMemcpyDeviceToHost));
#else
        (void) device_copy;
#endif
        return v;
    }
};
} // namespace

void digest_host_scene(HostScene &hs, bool device, uint64_t out[8]) {
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (device) {
#if defined(MTSAMD_HOST_ONLY)
        throw std::runtime_error("mts_debug_scene_digest: host-only build (no device scene)");
#else
        if (!hs.uploaded) throw std::runtime_error("mts_debug_scene_digest: the scene is not in device memory");
        HIP_CHECK(hipSetDevice(hs.device));
        HIP_CHECK(hipDeviceSynchronize());
#endif
    }
    const DigestSource from{ device };
    const DScene &sc = hs.scene;
    Fnv rec, grid, pair, tab, spec, head, geom, sens;
    std::vector<DVolume> volumes = from(sc.volumes, hs.volumes);
    std::vector<DPhase> phases = from(sc.phases, hs.phases);
    std::vector<DMedium> media = from(sc.media, hs.media);
    for (size_t i = 0; i < volumes.size(); ++i) {
        if (volumes[i].data != hs.volumes[i].data) throw std::runtime_error("mts_debug_scene_digest: a volume record points elsewhere than the host's copy");
        grid.add(from(volumes[i].data, hs.grid_data[i]));
        volumes[i].data = nullptr;
    }
    for (size_t i = 0; i < phases.size(); ++i) {
        if (phases[i].type == MTS_PHASE_TABULATED) { tab.add(from(phases[i].pdf, hs.tab_pdf[i])); tab.add(from(phases[i].cdf, hs.tab_cdf[i])); }
        phases[i].pdf = phases[i].cdf = nullptr;
    }
    for (size_t i = 0; i < media.size(); ++i) {
        if (!hs.pair_data[i].empty()) pair.add(from(media[i].pair_grid, hs.pair_data[i]));
        media[i].pair_grid = nullptr;
    }
    rec.add(volumes); rec.add(phases); rec.add(media);
    rec.add(from(sc.bsdfs, hs.bsdfs)); rec.add(from(sc.emitters, hs.emitters)); rec.add(from(sc.shapes, hs.shapes));
    {                                                      // textures: empty arrays add nothing, so a scene without them hashes as it always did
        std::vector<DTexture> textures = from(sc.textures, hs.textures);
        for (size_t i = 0; i < textures.size(); ++i) {
            if (textures[i].data != hs.textures[i].data) throw std::runtime_error("mts_debug_scene_digest: a texture record points elsewhere than the host's copy");
            tab.add(from(textures[i].data, hs.texels[i]));
            textures[i].data = nullptr;
        }
        rec.add(textures); rec.add(from(sc.bsdf_tex, hs.bsdf_tex));
    }
    if (hs.integrator.spectral) {
        std::vector<DSpectrum> spectra = from(sc.spectra, hs.spectra);
        for (size_t i = 0; i < spectra.size(); ++i) {
            spec.add(from(spectra[i].values, hs.spectrum_values[i]));
            spec.add(from(spectra[i].wavelengths, hs.spectrum_wavelengths[i]));
            spec.add(from(spectra[i].cdf, hs.spectrum_cdf[i]));
            spectra[i].values = spectra[i].wavelengths = spectra[i].cdf = nullptr;
        }
        spec.add(spectra);
        spec.add(from(sc.bsdf_sp, hs.bsdf_sp)); spec.add(from(sc.emitter_sp, hs.emitter_sp)); spec.add(from(sc.volume_sp, hs.volume_sp));
    }
    DScene h = sc;                                         // the kernel argument: its scalars, every pointer zeroed
    h.volumes = nullptr; h.phases = nullptr; h.media = nullptr; h.bsdfs = nullptr; h.shapes = nullptr; h.prims = nullptr; h.walk = nullptr; h.emitters = nullptr;
    h.positions = h.normals = h.texcoords = nullptr; h.faces = nullptr; h.tri = h.tri_attr = h.area_pmf = h.area_cdf = nullptr;
    h.bvh_nodes = nullptr; h.bvh_prims = nullptr; h.bvh_lds = nullptr; h.sensor.rfilter.values = nullptr; h.sensor.multi = nullptr;
    h.spectra = nullptr; h.bsdf_sp = nullptr; h.emitter_sp = nullptr; h.volume_sp = nullptr; h.cie = nullptr; h.bin_lo = h.bin_hi = nullptr;
    head.add(&h, offsetof(DScene, textures));              // the header up to the textured tail, which the record slot holds (texture_count: its array)

    const int32_t tail[2] = { hs.traits, hs.srf_lookup_by_wavelength ? 1 : 0 };
    head.add(tail, sizeof(tail));
    geom.add(from(sc.prims, hs.prims)); geom.add(from(sc.walk, hs.walk));
    geom.add(from(sc.positions, hs.positions)); geom.add(from(sc.normals, hs.normals)); geom.add(from(sc.texcoords, hs.texcoords));
    geom.add(from(sc.faces, hs.faces)); geom.add(from(sc.tri, hs.tri)); geom.add(from(sc.tri_attr, hs.tri_attr));
    geom.add(from(sc.area_pmf, hs.area_pmf)); geom.add(from(sc.area_cdf, hs.area_cdf));
    geom.add(from(sc.bvh_nodes, hs.bvh_nodes)); geom.add(from(sc.bvh_prims, hs.bvh_prims));
    if (!hs.instances.empty()) {                           // instanced scenes: the records behind the tail's pointers and the two counts; nothing for any other scene
        geom.add(from(sc.instances, hs.instances)); geom.add(from(sc.groups, hs.groups));
        const int32_t counts[2] = { sc.instance_count, sc.group_count }; geom.add(counts, sizeof(counts));
    }
    sens.add(from(sc.sensor.rfilter.values, hs.rfilter_values)); sens.add(from(sc.sensor.multi, hs.multi_transforms));
    sens.add(from(sc.bin_lo, hs.bin_lo)); sens.add(from(sc.bin_hi, hs.bin_hi));
    for (const HostSensor &x : hs.extra_sensors) {         // added sensors: nothing for a scene without them, so it hashes as it always did
        DSensor r = x.sensor; r.rfilter.values = nullptr; r.multi = nullptr;
        const int32_t of_sensor[2] = { x.srf, x.srf_lookup_by_wavelength ? 1 : 0 };
        head.add(&r, sizeof(r)); head.add(of_sensor, sizeof(of_sensor));
        sens.add(from(x.sensor.rfilter.values, x.rfilter_values)); sens.add(from(x.sensor.multi, x.multi_transforms));
    }
    out[0] = rec.h; out[1] = grid.h; out[2] = pair.h; out[3] = tab.h; out[4] = spec.h; out[5] = head.h; out[6] = geom.h; out[7] = sens.h;
}

} // namespace mtsamd
