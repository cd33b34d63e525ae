"""The ring kernels' geometry table (csrc/integrator_dev.h: MTS_GEOM_LDS), film and loop counters against the oracle bit for bit.

The volpath ring kernels of the lean units a / h keep the triangle attribute rows of a scene without a BVH and with at most 16
primitives in LDS: hit points and surface frames read vertices, normals and texture coordinates from the table per lane.  One small
scene per thing that can go wrong: the common scene (13 primitives) and a ragged film of it; exactly 16 primitives (the last count
the table takes: rectangles and a disk, whose rows are zero, behind the triangles); 17 (the first count that reads the scene records
as before); a mesh with vertex normals and texture coordinates (every part of an attribute row); two coincident rectangles (equal
t: the later primitive wins); unit h, and unit b, which has no table; gpu_mono.  One 32 x 32 block (a 1024-path workgroup) or less,
4 - 8 spp, 8^3 grids; every case is rendered with and without loop counters and asserts the kernel that served it.

Without a GPU: the oracle finishes every scene; the mesh case's film depends on its vertex normals and on its texture coordinates,
and the equal-t case's film on the order of the two rectangles (otherwise those cases would prove nothing); the host-side kernel
table chooses the asserted kernels."""
import ctypes as C
import importlib
import os
import tempfile

import numpy as np
import pytest

import tests.oracle_binding as ob

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

RES = 8
LEAN_A_RING_1024, LEAN_B_RING_1024, LEAN_H_RING_1024 = 111024, 211024, 611024          # mts_stats.kernel_variant

# three triangles that share edges but no plane, every vertex with a normal that is not its faces' and a texture coordinate whose
# map is neither the identity nor degenerate
MESH_OBJ = """v -1 -1 0
v 1 -1 0
v 1 1 0.3
v -1 1 0
v 0 2.2 0.6
vt 0 0
vt 1 0.1
vt 0.9 1
vt 0.1 0.8
vt 0.5 1.7
vn -0.3 -0.2 0.93
vn 0.35 -0.25 0.9
vn 0.4 0.1 0.91
vn -0.25 0.3 0.92
vn 0.05 0.5 0.86
f 1/1/1 2/2/2 3/3/3
f 1/1/1 3/3/3 4/4/4
f 4/4/4 3/3/3 5/5/5
"""
_mesh_dir = []


def mesh_file(texcoords=True):
    """the patch as an OBJ file, with or without its `vt` lines, in a directory that goes away with the interpreter"""
    if not _mesh_dir:
        _mesh_dir.append(tempfile.TemporaryDirectory(prefix="geom_table_"))
    path = os.path.join(_mesh_dir[0].name, "patch.obj" if texcoords else "patch_no_vt.obj")
    if not os.path.exists(path):
        text = MESH_OBJ if texcoords else "".join(
            line + "\n" if not line.startswith("f ") else "f " + " ".join("%s//%s" % (v.split("/")[0], v.split("/")[2]) for v in line.split()[1:]) + "\n"
            for line in MESH_OBJ.splitlines() if not line.startswith("vt "))
        with open(path, "w") as f:
            f.write(text)
    return path


def diffuse(rgb):
    return {"type": "diffuse", "reflectance": {"type": "rgb", "value": rgb}}


def common(width=32, height=32, spp=8):
    """the slab cube (12 triangles) and the ground (a rectangle): 13 primitives; the camera looks down from z = 20 and sees |x|, |y| < 7.4 at z = 2"""
    return scenes.c3_heterogeneous(width, height, spp, res=RES)


def sixteen():
    d = common()
    d["plate_a"] = {"type": "rectangle", "to_world": T.translate([-3, 2, 3]) @ T.scale(1.5), "bsdf": diffuse([0.7, 0.3, 0.2])}
    d["plate_b"] = {"type": "rectangle", "to_world": T.translate([3, -2, 4]) @ T.rotate([1, 0, 0], 20) @ T.scale(1.2), "bsdf": diffuse([0.2, 0.6, 0.8])}
    d["dish"] = {"type": "disk", "to_world": T.translate([1, 3, 3.5]) @ T.rotate([0, 1, 0], -15) @ T.scale(1.3), "bsdf": diffuse([0.6, 0.6, 0.1])}
    return d


def seventeen():
    d = sixteen()
    d["plate_c"] = {"type": "rectangle", "to_world": T.translate([-2, -3, 2.5]) @ T.scale(1.0), "bsdf": diffuse([0.4, 0.8, 0.4])}
    return d


def with_mesh(face_normals=False, texcoords=True):
    d = common()
    d["patch"] = {"type": "obj", "filename": mesh_file(texcoords), "face_normals": face_normals,
                  "to_world": T.translate([0.5, -0.5, 3.2]) @ T.rotate([1, 0, 0], 15) @ T.scale(2.0), "bsdf": diffuse([0.8, 0.8, 0.8])}
    return d


def coincident(first, second):
    d = common()
    xf = T.translate([0.5, 0.5, 3]) @ T.scale(3.0)
    d["sheet_1"] = {"type": "rectangle", "to_world": xf, "bsdf": diffuse([first] * 3)}
    d["sheet_2"] = {"type": "rectangle", "to_world": xf, "bsdf": diffuse([second] * 3)}
    return d


def case_scene(case):
    """-> (scene dict, oracle keywords, package variant, expected kernel_variant, primitives)"""
    if case == "common":
        return common(), {}, "gpu_rgb", LEAN_A_RING_1024, 13
    if case == "ragged_film":
        return common(20, 12), {}, "gpu_rgb", LEAN_A_RING_1024, 13
    if case == "prims_16":
        return sixteen(), {}, "gpu_rgb", LEAN_A_RING_1024, 16
    if case == "prims_17":
        return seventeen(), {}, "gpu_rgb", LEAN_A_RING_1024, 17
    if case == "mesh_attributes":
        return with_mesh(), {}, "gpu_rgb", LEAN_A_RING_1024, 16
    if case == "equal_t":
        return coincident(0.2, 0.8), {}, "gpu_rgb", LEAN_A_RING_1024, 15
    if case == "unit_b":
        return scenes.c4_atmosphere(32, 32, 4, layers=8), {}, "gpu_rgb", LEAN_B_RING_1024, 13
    if case == "unit_h":
        return scenes.c2_homogeneous_slab(32, 32, 4), {}, "gpu_rgb", LEAN_H_RING_1024, 13
    if case == "mono":
        return common(spp=4), {"mono": True}, "gpu_mono", LEAN_A_RING_1024, 13
    # oracle-only neighbours of two cases: what their conditions compare with
    if case == "mesh_no_texcoords":
        return with_mesh(texcoords=False), {}, "gpu_rgb", LEAN_A_RING_1024, 16
    if case == "mesh_face_normals":
        return with_mesh(face_normals=True), {}, "gpu_rgb", LEAN_A_RING_1024, 16
    if case == "equal_t_swapped":
        return coincident(0.8, 0.2), {}, "gpu_rgb", LEAN_A_RING_1024, 15
    raise KeyError(case)


CASES = ["common", "ragged_film", "prims_16", "prims_17", "mesh_attributes", "equal_t", "unit_b", "unit_h", "mono"]
_oracle = {}


def oracle(case):
    """film and (n_iter, n_lookup, n_nee_step) of the oracle, rendered once per case"""
    if case not in _oracle:
        d, kw, _, _, _ = case_scene(case)
        o = ob.OracleScene(d, **kw)
        ref = o.render(threads=16)
        ref.setflags(write=False)
        _oracle[case] = (ref, (o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"]))
    return _oracle[case]


def test_cases_finish_on_the_oracle_and_their_conditions_hold():
    for c in CASES:
        ref, counters = oracle(c)
        assert np.isfinite(ref).all() and ref[..., 4].max() > 0 and counters[0] > 0 and counters[2] > 0, (c, counters)
    assert oracle("ragged_film")[0].shape[:2] == (12, 20)
    # every added shape is seen: the film differs from the one without it
    assert not np.array_equal(oracle("prims_16")[0], oracle("common")[0])
    assert not np.array_equal(oracle("prims_17")[0], oracle("prims_16")[0])
    # the vertex normals reach the film (the shading frame of a diffuse BSDF): without them the attribute rows would only be read for p0 p1 p2
    assert not np.array_equal(oracle("mesh_attributes")[0], oracle("mesh_face_normals")[0])
    # ... and so do the texture coordinates (floats 18 .. 23 of a row set dp_du, the shading frame's tangent)
    assert not np.array_equal(oracle("mesh_attributes")[0], oracle("mesh_no_texcoords")[0])
    # equal t: the later of the two coincident sheets is the one that is hit, so their order shows
    assert not np.array_equal(oracle("equal_t")[0], oracle("equal_t_swapped")[0])


def test_cases_choose_the_ring_kernels():
    A = importlib.import_module("eradiate-kernel_amd._capi")
    SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    L = A.lib()
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    for case in CASES:
        d, kw, _, expect, _ = case_scene(case)
        desc, keep = SD.build_scene_desc(d, spectral=bool(kw.get("spectral")))
        v = C.c_int32(-1)
        assert L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)) == 0, L.mts_last_error()
        assert v.value == expect, (case, v.value)


def primitives_of(d):
    """primitives of a scene dict as the loader counts them: 12 per cube, one per rectangle / disk, a mesh file's triangles"""
    mesh_io = importlib.import_module("eradiate-kernel_amd.mesh_io")
    n = 0
    for v in d.values():
        if isinstance(v, dict) and v.get("type") in ("cube", "rectangle", "disk", "obj"):
            n += {"cube": 12, "rectangle": 1, "disk": 1}.get(v["type"]) or len(mesh_io.read_obj(v["filename"])[3])
    return n


def test_cases_have_the_primitive_counts_they_are_named_after():
    for case in CASES:
        d, _, _, _, prims = case_scene(case)
        assert primitives_of(d) == prims, (case, primitives_of(d))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_geom_table_matches_the_oracle(gpu_rgb, case):
    d, _, variant, expect, _ = case_scene(case)
    ref, counters = oracle(case)
    gpu_rgb.set_variant(variant)
    try:
        for collect in (True, False):                            # the instantiations with and without loop counters
            scene = gpu_rgb.load_dict(d)
            sensor = scene.sensors()[0]
            assert scene.integrator().render(scene, sensor, collect_counters=collect)
            st = scene.integrator().last_stats
            film = np.array(sensor.film().bitmap(raw=True))
            assert st["kernel_variant"] == expect, (case, collect, st["kernel_variant"])
            assert np.array_equal(film, ref), (case, collect, float(np.abs(film - ref).max()), int((film != ref).sum()))
            if collect:
                assert (st["n_iter"], st["n_lookup"], st["n_nee_step"]) == counters, (case, st, counters)
    finally:
        gpu_rgb.set_variant("gpu_rgb")
