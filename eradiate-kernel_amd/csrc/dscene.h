// dscene.h -- flattened, device-resident scene: what the reference's plugins hold after construction,
// as POD records in HBM.  Built on the host by scene_host.cpp (the "plugin constructors"), read by the
// render kernels through wave-uniform (scalar) loads: every record below is indexed by values that
// are uniform across a wavefront except where noted, so the scene lives in SGPRs / the scalar cache
// and costs no vector memory traffic.  Citations are relative to /root/reference.
#pragma once
#include <stdint.h>

namespace mtsamd {

#define MTS_BVH_TOP_DEPTH 8           // levels 0..8 (at most 511 nodes, 16 KB) are laid out breadth-first and staged in LDS
#define MTS_BVH_LDS_NODES 511

struct DXf { float m[16]; float it[16]; };            // Transform4f: matrix + inverse transpose (transform.h:36-50)

struct DBBox { float min[3], max[3]; };

// Volume (render/texture.h:210-279, textures/grid3d.cpp, textures/constant3d.cpp)
struct DVolume {
    int32_t type;                 // MTS_VOLUME_*
    float value[3];
    float w2l[16];                // world_to_local matrix (row-major)
    int32_t affine;               // last row of w2l is exactly (0, 0, 0, 1): the homogeneous divide is x / 1
    DBBox bbox;
    const float *data;            // device pointer, nz*ny*nx*channels, x fastest
    int32_t nx, ny, nz, channels, filter, wrap;
    float max;
    int32_t has_max;
    int32_t columns_equal;        // every (y, x) column holds the same values (a 1-D, plane-parallel profile stored as a 3-D grid): the eight
                                  // corners of a cell are two distinct voxels (z0, z1) -- the lookups gather those two and run the same arithmetic
};

// Phase functions (phase/*.cpp); the tabulated distribution of tabphase (core/distr_1d.h:293-345)
struct DPhase {
    int32_t type;
    float g;
    int32_t child[2];
    int32_t weight_volume;
    const float *pdf, *cdf;       // device pointers
    int32_t size;
    float range_x, range_y, integral, normalization, interval_size, inv_interval_size;
    uint32_t valid_x, valid_y;
};

// Media (media/homogeneous.cpp, media/heterogeneous.cpp)
struct DMedium {
    int32_t type, sigma_t, albedo, phase;
    int32_t shared_grid;          // sigma_t and albedo are grids with identical transform / resolution / filter / wrap
    int32_t grey;                 // every channel of sigma_t / albedo / combined extinction carries the same value
    float scale;
    int32_t sample_emitters, has_spectral_extinction, is_homogeneous;
    float max_density;
    // RN(1 / max_density) when the kernels may divide by the majorant through it (div_by_invariant, volpath_flat.h): 0 otherwise
    // (homogeneous media, or a majorant whose reciprocal is not safely representable)
    float inv_max_density;
    DBBox aabb;
    // MI355X layout: when sigma_t and albedo are single-channel trilinear clamp-mode grids sharing one transform, the host also
    // uploads them interleaved, voxel by voxel {sigma_t, albedo} (padded by one voxel): the two x-neighbours of both grids are
    // 16 contiguous bytes, so a lookup is 4 wide gathers instead of 16 dword gathers.  NULL otherwise.
    const float *pair_grid;
    // ... together with a copy of what a lookup needs from the sigma_t volume record (one scalar load for the whole step
    // instead of the chain medium -> volume): world_to_local, resolution, affine flag.  Valid when pair_grid != NULL.
    float pair_w2l[16];
    int32_t pair_nx, pair_ny, pair_nz, pair_affine;      // pair_affine: bit 0 = affine, bit 1 = both grids have equal columns (DVolume::columns_equal)
};

// A blendbsdf (MTS_BSDF_BLEND; TEX instantiations only) keeps in the same record: reflectance[0] = its constant weight, the bits of
// rho_0[0] / rho_0[1] = the indices of bsdf_0 / bsdf_1, flags = the union of its children's (blendbsdf.cpp:80); slot 0 of its bsdf_tex
// row = the weight's texture.
// A twosided (MTS_BSDF_TWOSIDED; TEX instantiations only) keeps the bits of rho_0[0] / rho_0[1] = the indices of brdf_0 (the side
// cos_theta(wi) > 0) / brdf_1 (< 0), equal when one child was given, and flags = the union of twosided.cpp:78-88; nothing else is read.
// A dielectric (MTS_BSDF_DIELECTRIC; TEX instantiations only) keeps rho_0[0] = eta = int_ior / ext_ior, reflectance = specular_reflectance,
// transmittance = specular_transmittance.  A conductor (MTS_BSDF_CONDUCTOR; TEX instantiations only) keeps rho_0 = eta and k = k per
// channel, reflectance = specular_reflectance.
struct DBsdf { int32_t type; float reflectance[3], rho_0[3], k[3], g[3], rho_c[3]; uint32_t flags; float transmittance[3]; };

// Textures behind a BSDF's colour parameters (textures/bitmap.cpp, textures/checkerboard.cpp; rgb / mono variants).  to_uv: row-major
// 3x3 (Transform4f::extract, transform.h:327-348).  data: device pointer to height * width texels, texel (x, y) at x + y * width;
// a single-channel texel is one float, a three-channel texel four (r, g, b, 0): one 16-byte load.
struct DTexture { int32_t type; float to_uv[9]; const float *data; int32_t width, height, channels, filter, wrap; float color0[3], color1[3]; };

// Shapes (shapes/rectangle.cpp, shapes/cube.cpp + librender/mesh.cpp, shapes/sphere.cpp)
struct DShape {
    int32_t type;
    DXf to_world, to_object;
    int32_t bsdf, interior, exterior, emitter;   // bsdf always resolved (default diffuse appended by the host)
    float frame_s[3], frame_t[3], frame_n[3];     // rectangle.cpp:66-74
    float inv_surface_area;
    float surface_area;                           // disk (disk.cpp:108-111)
    float center[3], radius;                      // sphere; cone (cone.cpp:98-108): center = the tip in object space (0, 0, length), radius = that of the
                                                  // base circle; to_world / to_object of a cone are rigid (rotation + translation)
    int32_t flip_normals;
    int32_t vertex_offset, face_offset;           // into the scene-wide mesh arrays
    int32_t has_normals, has_texcoords;
    int32_t is_medium_transition;
    int32_t bsdf_type; uint32_t bsdf_flags;       // copies of bsdfs[bsdf].type / .flags: spares the surface blocks a dependent record load
    int32_t prim_offset;                          // index of this shape's first primitive in prim order (DScene::tri_attr)
    int32_t area_lo, area_hi;                     // meshes: first / last face with a non-zero area (distr_1d.h:60-75); -1 = none
};

struct DPrim { int32_t shape, index; };
// Everything the primitive-list walk needs about one primitive in ONE 64-byte record (one scalar load per primitive instead of a
// chain prim -> shape -> geometry): triangle: p0, e1, e2; rectangle: rows 0..2 of to_object; sphere: center, radius.
// cone (read by the INST kernels only): rows 0..2 of its rigid to_object, and the bits of radius / length in index / pad (its one primitive is primitive 0).
struct DWalkPrim { int32_t type, shape, index, pad; float f[12]; };

// Instanced geometry (shapes/shapegroup.cpp, shapes/instance.cpp, librender/shapegroup.cpp; read by the INST kernels only, kernels.hip: render_kernel_inst).
// A shapegroup's members are DShape records like any other, but their primitives are not the scene's: they stand behind the scene's
// own in prims / walk / tri / tri_attr / area_*, group by group, in GROUP space (the members' own to_world and nothing else), and a
// group with more primitives than the BVH threshold has a BVH of its own behind the scene's in bvh_nodes / bvh_prims (node and leaf
// indices absolute).  An instance is ONE primitive of the scene: a DWalkPrim of type MTS_SHAPE_INSTANCE whose shape = its index in
// DScene::instances, index = its group's in DScene::groups, f = rows 0..2 of to_object -- the ray transform (instance.cpp:111-112)
// needs that one record.  DScene::prim_count / bvh_node_count count the scene's own level.
struct DGroup { DBBox bbox; int32_t node_first, node_count, prim_first, prim_count, shape, pad; };      // bbox: of the members (shapegroup.cpp: the group's kd-tree bbox); shape: the group's record
struct DInstance { DXf to_world, to_object; int32_t group, shape, pad[2]; };                            // shape: the instance's record in DScene::shapes
// A hit inside an instance keeps 1 + the instance's index in the bits of Hit::shape above the member's shape index (INST kernels only)
#define MTS_INST_SHAPE_BITS 10
#define MTS_INST_MAX_SHAPES (1 << MTS_INST_SHAPE_BITS)                  // shape records of an instanced scene
#define MTS_INST_MAX_INSTANCES ((1 << (31 - MTS_INST_SHAPE_BITS)) - 2)  // 2^21 - 2 instances

struct DEmitter { int32_t type; DXf to_world; float radiance[3]; int32_t shape; float bsphere_center[3], bsphere_radius; };

struct DRFilter { int32_t type; float radius, stddev, alpha, bias; const float *values /* device, 32 entries (rfilter.cpp:9-20) */; float scale_factor; int32_t border_size; };

struct DSensor {
    int32_t type;
    DXf to_world;
    float s2c[16];                 // sample_to_camera matrix (perspective.cpp:107-111)
    float near_clip, far_clip, ppo[2];
    int32_t direction_type, flip_directions, target_type;
    float target_point[3];
    DShape target_shape;
    float target_area;
    float bsphere_center[3], bsphere_radius;
    int32_t needs_aperture_sample, medium;
    float shutter_open_time;       // > 0: one more draw per sample (integrator.cpp:248-250)
    int32_t origin_type;           // distant / distantflux: 1 = project the target onto origin_shape (distant.cpp:368-375)
    DShape origin_shape;
    int32_t width, height, crop_x, crop_y, crop_w, crop_h;
    DRFilter rfilter;
    int32_t sample_count;
    int32_t wavefront;             // 1: one TEA-seeded stream per (pixel, sample) as the reference's gpu_* variants (seed_wavefront_sample)
    uint64_t seed;
    const float *multi;            // mradiancemeter / mdistant: multi_count 4x4 matrices (device pointer)
    int32_t multi_count;
};

// Spectra (spectral variants): `uniform` (spectra/uniform.cpp:34-62: value inside [lambda_min, lambda_max], 0 outside) and `regular`
// (spectra/regular.cpp: a ContinuousDistribution over [lambda_min, lambda_max], core/distr_1d.h:378-400 eval_pdf)
// `irregular` (spectra/irregular.cpp: values at the nodes `wavelengths`) and `discrete` (spectra/discrete.cpp: a sampling-only sensor
// response: `wavelengths`, `values` and the running sum of the pmf, DiscreteDistribution, core/distr_1d.h:49-83)
struct DSpectrum { int32_t type; float value, lambda_min, lambda_max; const float *values; int32_t count; float inv_interval_size;
                   const float *wavelengths, *cdf; float cdf_sum; uint32_t valid_x, valid_y; };
enum { MTS_BSDF_SP_REFLECTANCE = 0, MTS_BSDF_SP_RHO_0, MTS_BSDF_SP_K, MTS_BSDF_SP_G, MTS_BSDF_SP_RHO_C, MTS_BSDF_SP_TRANSMITTANCE, MTS_BSDF_SP_COUNT };
// constvolume: the spectrum of its value; gridvolume_spectral (textures/gridvolume_spectral.cpp): the spectral interval its channels cover
struct DVolumeSp { int32_t value_sp; int32_t spectral_grid; float lambda_min, lambda_max; };

struct DIntegrator { int32_t type, max_depth, rr_depth, hide_emitters, use_spectral_mis, monochrome; };

// One spiral block (librender/spiral.cpp:27-72) assigned to this launch
// Scene traits (integrator_dev.h: MTS_TRAITS; scene_host.cpp: scene_traits; render_plan.cpp: KERNEL_UNITS, the choice of the lean translation unit).
#define MT_MEDIA 1              // every medium: heterogeneous with spectral extinction and -- rgb / mono: grey, on a pair grid (DMedium::pair_grid);
                                // spectral variant: two gridvolume_spectral grids sharing geometry and interval (DMedium::shared_grid == 2)
#define MT_NO_BVH 2             // the primitive list is walked (no BVH)
#define MT_NO_SPHERE 4          // no sphere shapes
#define MT_NO_GRID_EVAL 8       // no grid volume is evaluated through volume_eval() (media go through their pair grids; no grid as a blend weight ...)
#define MT_NO_SHAPE_EMITTER 16  // no area emitters (shape_sample_direction)
#define MT_NO_PHASE_TREE 32     // no nested blendphase
#define MT_NO_RPV 64            // no rpv BSDF
#define MT_HOMOG 128            // every medium homogeneous (excludes MT_MEDIA)
// what each lean translation unit promises (kernels_lean_*.hip) -- mts_render launches the first one in this order whose promises a scene keeps
#define MT_UNIT_A (MT_MEDIA | MT_NO_BVH | MT_NO_SPHERE | MT_NO_GRID_EVAL | MT_NO_SHAPE_EMITTER | MT_NO_PHASE_TREE | MT_NO_RPV)
#define MT_UNIT_B (MT_MEDIA | MT_NO_BVH | MT_NO_SPHERE | MT_NO_SHAPE_EMITTER | MT_NO_PHASE_TREE)      // also unit s (spectral variant)
#define MT_UNIT_C (MT_MEDIA | MT_NO_SPHERE | MT_NO_SHAPE_EMITTER | MT_NO_PHASE_TREE)
#define MT_UNIT_H (MT_HOMOG | MT_NO_BVH | MT_NO_SPHERE | MT_NO_GRID_EVAL | MT_NO_SHAPE_EMITTER | MT_NO_PHASE_TREE)
#define MT_UNIT_P (MT_NO_BVH | MT_NO_SPHERE | MT_NO_GRID_EVAL | MT_NO_PHASE_TREE | MT_NO_RPV)          // compiled with these ...
#define MT_UNIT_P_NEEDS (MT_NO_BVH | MT_NO_SPHERE | MT_NO_RPV)                                          // ... of which `path` can reach these

struct DBlock { int32_t ox, oy, sx, sy; uint32_t id; uint32_t sample_base; /* wavefront streams: first sample index this entry renders */
                uint32_t film_off_lo, film_off_hi; /* floats from the launch's film pointer to the film this entry adds to: the slot of its pass (capi.cpp) */ };
static_assert(sizeof(DBlock) == 32, "DBlock is read as eight dwords (volpath_flat.h: wg_env)");

struct DScene {
    const DVolume *volumes;
    const DPhase *phases;
    const DMedium *media;
    const DBsdf *bsdfs;
    const DShape *shapes;
    const DPrim *prims;
    const DWalkPrim *walk;                          // prim order, one record per primitive
    const DEmitter *emitters;
    const float *positions, *normals, *texcoords;   // world-space mesh data of all meshes
    const uint32_t *faces;
    const float *tri;                               // per primitive (prim order): p0, e1 = p1 - p0, e2 = p2 - p0 (triangles only)
    const float *tri_attr;                          // per primitive, 24 floats: p0 p1 p2, n0 n1 n2, uv0 uv1 uv2 of a triangle -- what hit_point()
                                                    // and complete_surface() need, in one place instead of behind the face indices
    const float *area_pmf, *area_cdf;               // per primitive (prim order): face area and its running sum within the mesh
                                                    // (Mesh::build_pmf, mesh.cpp:285-312); 0 for other primitives
    // Bounding-volume hierarchy over the primitives, built by the host for scenes with many primitives (NULL otherwise: the
    // primitive list is walked).  32-byte nodes: bmin[3], bmax[3] (conservatively enlarged), skip = the node to visit when this
    // subtree is missed or done, link = (first << 3 | count) into bvh_prims for a leaf, minus the index of the left child for an
    // inner node (the right child is left.skip).  The top MTS_BVH_TOP_DEPTH levels come first, in breadth-first order: the
    // per-lane kernels stage them in LDS (bvh_lds / bvh_lds_count, set by the kernel on its copy of this record).
    const float *bvh_nodes;
    const int32_t *bvh_prims;                       // leaf contents: primitive indices (prim order decides ties, kdtree.h:2152-2154)
    int32_t bvh_node_count;
    const float *bvh_lds; int32_t bvh_lds_count;
    int32_t volume_count, phase_count, medium_count, bsdf_count, shape_count, prim_count, emitter_count;
    int32_t environment;
    DBBox bbox;
    DSensor sensor;
    DIntegrator integrator;
    // Spectral variants only (gpu_spectral; NULL / unused otherwise).  They sit BEHIND the records the rgb kernels load, in arrays of
    // their own, so that the rgb records -- and the scalar loads that fetch them -- stay exactly as they are.
    const DSpectrum *spectra;                       // every spectrum of the scene (spectra/uniform.cpp, spectra/regular.cpp; d65 expands to regular)
    const int32_t *bsdf_sp;                         // per BSDF, MTS_BSDF_SP_COUNT indices into spectra: reflectance, rho_0, k, g, rho_c, transmittance
    const int32_t *emitter_sp;                      // per emitter: radiance / irradiance / intensity
    const DVolumeSp *volume_sp;                     // per volume
    const float *cie;                               // CIE 1931 x, y, z, 95 samples each over 360 .. 830 nm (core/spectrum.h:127-133)
    int32_t srf;                                    // the sensor's spectral response function: index into spectra, -1 = none (perspective.cpp:173-182)
    // integrators/nbins.cpp (bin_mode 1: wavelength bin_lo[i] +- bin_hi[i]) / bins.cpp (2: interval [bin_lo[i], bin_hi[i]]): two AOV
    // channels per bin behind X, Y, Z, A, W; film_channels = 5 + 2 bin_count floats per pixel
    int32_t bin_mode, bin_count;
    const float *bin_lo, *bin_hi;
    int32_t film_channels;
    // Bit i: shape i (i < 64) is a boundary that a main path merely crosses -- a null BSDF, which is not smooth, and no emitter on the
    // shape: no emitter term, no emitter sample, no BSDF evaluation at such a hit.  The ring machines sort these hits into a class of
    // their own (volpath_flat.h: B_CROSS).  Set where the shape records are built (scene_host.cpp: add_shape); a shape beyond 63 has no bit.
    uint64_t cross_mask;
    // Scenes with textures, a blendbsdf or a twosided only (rgb / mono; NULL / 0 otherwise; a blend or twosided scene without textures has bsdf_tex alone), at the END of the record: everything above keeps its offset, so the plain
    // kernels read what they always read.  bsdf_tex: per BSDF (the two default ones included) MTS_BSDF_SP_COUNT indices into
    // textures, in the order reflectance, rho_0, k, g, rho_c, transmittance; -1 = the constant in DBsdf.  Only the TEX
    // instantiations (integrator_dev.h: HitBsdf) read them.
    const DTexture *textures;
    const int32_t *bsdf_tex;
    int32_t texture_count, pad_;
    // Instanced scenes only (NULL / 0 otherwise), behind the textured tail: nothing above moves.  Only the INST kernels read them.
    const DInstance *instances;
    const DGroup *groups;
    int32_t instance_count, group_count;
};

// bsdf.h:38-124
enum : uint32_t { F_Null = 0x1, F_DiffuseReflection = 0x2, F_DiffuseTransmission = 0x4, F_GlossyReflection = 0x8,
                  F_DeltaReflection = 0x20, F_DeltaTransmission = 0x40, F_NonSymmetric = 0x4000,
                  F_FrontSide = 0x8000, F_BackSide = 0x10000,
                  F_Smooth = 0x2 | 0x4 | 0x8 | 0x10, F_Delta = 0x1 | 0x20 | 0x40, F_Transmission = 0x4 | 0x10 | 0x40 | 0x100 | 0x1 };

} // namespace mtsamd
