// scene_host.h -- host-side scene object behind the opaque mts_scene handle.
#pragma once
#include <vector>
#include <string>
#include <memory>
#include <atomic>
#include <stdexcept>
#include <hip/hip_runtime_api.h>
#include "dscene.h"
#include "dmath.h"
#include "../../include/mtsamd.h"

namespace mtsamd {

// A sensor beyond sensor 0 (mts_scene_add_sensor): its record, what the kernel choice reads of it, and its two tables.  The record's
// device pointers (rfilter.values, multi) are allocations of the scene (HostScene::device_allocs): made when the sensor is added,
// freed by free_host_scene and never before.
struct HostSensor {
    DSensor sensor;
    int32_t srf = -1;                           // DScene::srf of a render through this sensor
    bool srf_lookup_by_wavelength = true;
    std::vector<float> rfilter_values, multi_transforms;
};

struct HostScene {
    DScene scene;                               // kernel argument (device pointers filled by upload); its sensor / srf are sensor 0's
    mts_integrator integrator;
    std::vector<DVolume> volumes;
    std::vector<DPhase> phases;
    std::vector<DMedium> media;
    std::vector<DBsdf> bsdfs;
    std::vector<DShape> shapes;
    std::vector<DPrim> prims;
    std::vector<DWalkPrim> walk;
    std::vector<DEmitter> emitters;
    std::vector<float> positions, normals, texcoords;
    std::vector<uint32_t> faces;
    std::vector<float> tri;
    std::vector<float> tri_attr;
    std::vector<float> area_pmf, area_cdf;           // prim order (DScene::area_pmf / area_cdf)
    std::vector<float> bvh_nodes;                    // 8 floats per node (DScene::bvh_nodes); empty = no BVH
    std::vector<int32_t> bvh_prims;
    std::vector<float> rfilter_values;
    std::vector<std::vector<float>> grid_data, tab_pdf, tab_cdf;
    std::vector<float> multi_transforms;            // mradiancemeter / mdistant sub-sensor matrices
    std::vector<std::vector<float>> pair_data;       // per medium: interleaved {sigma_t, albedo} voxels (DMedium::pair_grid), or empty
    // spectral variant (DScene::spectra ...)
    std::vector<DSpectrum> spectra; std::vector<std::vector<float>> spectrum_values, spectrum_wavelengths, spectrum_cdf;
    std::vector<float> bin_lo, bin_hi;
    bool srf_lookup_by_wavelength = true;            // the response function's weights can be recovered from the sampled wavelengths (regrouping kernel)
    std::vector<int32_t> bsdf_sp, emitter_sp; std::vector<DVolumeSp> volume_sp;
    // textured scenes (DScene::textures ...): the records, each bitmap's texels as the device holds them (three-channel texels padded
    // to four floats), and the per-BSDF index table; all three empty in a scene without textures -- but for the table of a scene that
    // holds a blendbsdf, a twosided, a dielectric or a conductor: a non-empty table is what sends a scene to the TEX instantiations
    std::vector<DTexture> textures; std::vector<std::vector<float>> texels; std::vector<int32_t> bsdf_tex;
    // instanced scenes (DScene::instances / groups): one record per MTS_SHAPE_INSTANCE / MTS_SHAPE_SHAPEGROUP, in the order of their
    // shape records; instance_boxes: the world-space box of each instance (instance.cpp:81-92), by its index in `instances` -- what
    // build_bvh puts around the instance's primitive (DWalkPrim::shape of that primitive is the index)
    std::vector<DInstance> instances; std::vector<DGroup> groups; std::vector<DBBox> instance_boxes;
    bool has_cone = false;                           // a shape record is an MTS_SHAPE_CONE (plain or a group's member): the scene renders in the INST kernels as an instanced one does
    std::vector<HostSensor> extra_sensors;           // sensors 1, 2, ... in the order they were added; rendering one never writes `scene`
    std::atomic<int> sensor_count{1};                // 1 + extra_sensors.size(), readable without the handle's mutex
    std::vector<void *> device_allocs;
    // mts_scene_update: two words per volume the grid pass reduces into (launch.h: GridUpdateJob::stats), allocated by the first update
    // that rewrites a grid.  After an update of an uploaded scene, grid_data / pair_data above keep their sizes, not the device's contents.
    uint32_t *update_stats = nullptr;
    int traits = 0;                                  // promises of integrator_dev.h's scene traits this scene keeps (MT_* bits; scene_traits())
    int device = 0;
    bool uploaded = false;
    std::atomic<int> stop{0};
};

HostScene *build_host_scene(const mts_scene_desc *desc);   // throws std::runtime_error
void build_bvh(HostScene &hs);                 // fills bvh_nodes / bvh_prims: the scene level's BVH when it has many primitives, then each group's by the same rule
void upload_host_scene(HostScene &hs, int device);          // throws std::runtime_error
void free_host_scene(HostScene *hs);
// mts_scene_add_sensor: runs sensor 0's constructor (validation included) for `sensor` against the scene as created -- its bounding
// sphere, media, spectra and integrator -- and, for an uploaded scene, uploads its two tables.  Returns the new sensor's index
// (1, 2, ...); throws std::runtime_error with the scene untouched.
int32_t add_host_sensor(HostScene &hs, const mts_sensor *sensor);
// What a render through sensor `index` reads of it: the record, DScene::srf, and the two inputs of the kernel choice that depend on
// the sensor -- traits are those of the (scene, sensor) pair, computed from the scene as it is now.  Throws for an index outside [0, count).
struct SensorView { const DSensor *sensor; int32_t srf; bool srf_lookup_by_wavelength; int traits; };
SensorView host_sensor(const HostScene &hs, int32_t index);
// mts_scene_update: re-runs build_host_scene's per-record work for the dirty records of `desc` and the records derived from them, and
// scene_traits.  Validates everything before it writes (throws std::runtime_error with the scene untouched).  An uploaded scene is
// rewritten in place on `stream` (grid statistics and pair grids by grid_update_kernel); a host-only scene through the host functions.
void update_host_scene(HostScene &hs, const mts_scene_desc *desc, const mts_dirty *dirty, int32_t n, hipStream_t stream);
// FNV-1a over the scene's contents, pointer fields zeroed: [0] record arrays (texture records and the BSDFs' texture indices behind
// them), [1] grid data, [2] pair grids, [3] phase tables (bitmap texels behind them),
// [4] spectra, [5] traits and the scalar header of DScene, [6] geometry (prims, walk, vertex and triangle tables, area tables, BVH; instance
// and group records behind them),
// [7] the sensor's and the bins' arrays (filter table, sub-sensor matrices, bin bounds).  Added sensors enter [5] (records) and [7]
// (tables) only when there are any.  One walk, two sources: `device` reads the
// uploaded copy back (throws for a scene that is not in device memory), otherwise the walk reads HostScene's own vectors -- no
// device is touched, and a fresh scene gives the same eight words either way.
void digest_host_scene(HostScene &hs, bool device, uint64_t out[8]);

} // namespace mtsamd
