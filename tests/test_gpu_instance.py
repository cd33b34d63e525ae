"""`shapegroup` / `instance` on the device (run with -m gpu on an MI355X).

What pins them: (1) the identity instance: every plain shape of a scene moved into one group that is instanced once with the identity
gives the oracle's film of the original dictionary, bit for bit; (2) a closed form -- one diffuse surface inside a rotated, unevenly
scaled and translated instance under a directional emitter, `path` with max_depth = 2, every sample rho E cos(theta) / pi with the
normal restated in float64 through the inverse transpose; (3) the kernels the table's rows map to and the four list / BVH combinations
of the two levels agree bit for bit; (4) K references to one group render what K inline copies render; (5) full transport between
five placed instances agrees with the independent float64 estimator, and wrong placements are rejected; (6) an update in place is a
fresh load; (7) 256 instances of a 4 096-face mesh cost the device the records of one.  The oracle knows no instances, so no RENDER
under a non-identity transform is compared with it bit for bit; intersection is, per ray: on dyadic placements the device's t,
member and primitive are the oracle's on the expanded plain scene (tests/test_gpu_instance_rays.py)."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.kernel_rows as kr
import tests.oracle_binding as ob
import tests.test_gpu_textures as tt
from tests.independent import problems_instance
from tests.sheet_shared import PLACE, place_matrix
from tests.test_gpu_textures import ATOL, CONSTANT_SCENES, bits, digest, render
from tests.test_independent_surface_pin import assert_agrees, rejected, rgb_estimate
from tests.test_independent_textured_pin import hip_render
from tests.test_instance import load_pin

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f


# ================================================================ 1. the identity instance against the oracle
def grouped(d):
    """every shape that carries neither an emitter nor a medium moved into one shapegroup, instanced once with the identity"""
    out, members = {}, {}
    for k, v in d.items():
        plain = isinstance(v, dict) and v.get("type") in ("rectangle", "cube", "sphere", "disk", "mesh") and not any(x in v for x in ("emitter", "interior", "exterior"))
        (members if plain else out)[k] = copy.deepcopy(v)
    assert members
    out["instanced"] = {"type": "instance", "to_world": T(), "group": dict({"type": "shapegroup"}, **members)}
    return out


_ORACLE = {}


def oracle_film(name, integrator):
    """computed once per scene and integrator, left unchanged"""
    if (name, integrator) not in _ORACLE:
        d = CONSTANT_SCENES[name][0]()
        d["integrator"]["type"] = integrator
        _ORACLE[(name, integrator)] = ob.OracleScene(d).render()
    return _ORACLE[(name, integrator)]


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
@pytest.mark.parametrize("name", sorted(CONSTANT_SCENES))
def test_identity_instance_equals_the_oracle(gpu_rgb, name, integrator):
    d = CONSTANT_SCENES[name][0]()
    d["integrator"]["type"] = integrator
    plain_row = render(gpu_rgb.load_dict(d))[1]["kernel_variant"] % 100000      # the row of the table, whichever unit renders the plain scene
    film, st = render(gpu_rgb.load_dict(grouped(d)))
    ref = oracle_film(name, integrator)
    print("%s %s: values differing from the oracle's: %d of %d" % (name, integrator, int(np.sum(bits(film) != bits(ref))), film.size))
    assert st["textured"] == 2 and st["kernel_variant"] == plain_row           # the general unit's row, unchanged
    assert np.array_equal(bits(film), bits(ref))


# ================================================================ 2. a closed form under a rotation, an uneven scale and a translation
def instanced_closed_form(surface, texture, integrator="path"):
    """tests/test_gpu_textures.closed_form_case with the surface inside a group instanced under PLACE: the group-space points and
    normals of that construction carried to world space here -- points by M, normals by the inverse transpose of M -- and the rays
    aimed at the world-space points.  (Under the uneven scale the sphere is an ellipsoid; the construction is the same.)"""
    tt.RNG = np.random.default_rng(2024)
    shape, p, uv, normal, seam = tt.SURFACES[surface](400)
    tex = tt.TEXTURES[texture] if texture else None
    rho, edge = tt.texture_eval(tex, uv) if tex else (np.full((len(p), 3), 0.6), np.full(len(p), np.inf))
    M = place_matrix()
    assert np.allclose(np.asarray(PLACE.matrix, np.float64), M, atol=1e-6)          # the loader's transform is the one restated here
    pw = p @ M[:3, :3].T + M[:3, 3]
    nw = normal @ np.linalg.inv(M[:3, :3])                                            # rows n^T M^-1 = (M^-T n)^T
    nw /= np.linalg.norm(nw, axis=1)[:, None]
    cos_sun = nw @ -tt.SUN
    keep = np.flatnonzero((edge >= tt.MARGIN) & (seam >= 0.02) & (cos_sun > 0.2))[:tt.N_RAYS]
    assert len(keep) == tt.N_RAYS, "not enough rays away from the discontinuities"
    pw, nw, rho, cos_sun = pw[keep], nw[keep], rho[keep], cos_sun[keep]
    tilt = nw + 0.3 * np.cross(nw, [0.3, 0.5, 0.8])
    tilt /= np.linalg.norm(tilt, axis=1)[:, None]
    origins, directions = pw + 1.5 * tilt, -tilt
    assert np.abs(np.r_[origins.ravel(), pw.ravel()]).max() <= 4.0                    # ATOL is derived for coordinates <= 4
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    member = dict(shape, bsdf={"type": "diffuse", "reflectance": copy.copy(tex) if tex else 0.6})
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": 2},
         "sensor": {"type": "mradiancemeter", "origins": fmt(origins), "directions": fmt(directions),
                    "film": {"type": "hdrfilm", "width": tt.N_RAYS, "height": 1, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}},
         "placed": {"type": "instance", "to_world": PLACE, "group": {"type": "shapegroup", "surface": member}},
         "sun": {"type": "directional", "direction": tt.SUN.tolist(), "irradiance": tt.IRRADIANCE}}
    return d, rho, cos_sun


@pytest.mark.parametrize("surface,texture", [("rectangle", None), ("disk", None), ("sphere", None), ("quad_uv", None), ("quad_bary", None),
                                             ("rectangle", "b53rgb_bilinear_mirror")])
def test_closed_form_inside_an_instance(gpu_rgb, surface, texture):
    """the bitmap on the rectangle: uv survives the instance"""
    d, rho, cos_sun = instanced_closed_form(surface, texture)
    film, st = render(gpu_rgb.load_dict(d))
    got = tt.measured_rho(film, cos_sun)
    print("%s / %s: max |rho - expected| = %.3g" % (surface, texture, np.abs(got - rho).max()))
    assert st["textured"] == 2 and st["kernel_variant"] == 1                 # `path`: the flat row, in its INST loop
    assert np.abs(got - rho).max() <= ATOL


@pytest.mark.parametrize("how", ["nested", "volpath", "volpathmis"])
def test_closed_form_other_kernels(gpu_rgb, monkeypatch, how):
    d, rho, cos_sun = instanced_closed_form("quad_uv", None, integrator="path" if how == "nested" else how)
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    film, st = render(gpu_rgb.load_dict(d))
    got = tt.measured_rho(film, cos_sun)
    print("%s: max |rho - expected| = %.3g" % (how, np.abs(got - rho).max()))
    assert st["textured"] == 2 and st["kernel_variant"] == 0
    assert np.abs(got - rho).max() <= ATOL


# ================================================================ 3. rows and structures agree
def leaf_mesh(n=5, seed=3):
    """a bumpy n x n grid: 2 n^2 = 50 triangles, one unit wide"""
    g = np.linspace(-0.5, 0.5, n + 1)
    x, y = np.meshgrid(g, g)
    z = 0.15 * np.random.default_rng(seed).random(x.shape)
    pos = np.c_[x.ravel(), y.ravel(), z.ravel()].astype(np.float32)
    faces = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            faces += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    return {"type": "mesh", "vertex_positions": pos, "faces": np.array(faces, np.uint32)}


def grove(slab=True, count=60, inline=False, size=32):
    """the heterogeneous slab of kernel_rows._c3 over `count` instances of a 50-triangle group and two plain rectangles"""
    d = kr._c3()
    d["sensor"]["film"]["width"] = d["sensor"]["film"]["height"] = size
    if not slab:
        del d["slab"]
        d["integrator"]["type"] = "path"
    leaf = dict(leaf_mesh(), bsdf={"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.6, 0.1]}})
    group = {"type": "shapegroup", "leaf": leaf, "stem": {"type": "sphere", "center": [0, 0, -0.2], "radius": 0.12, "bsdf": {"type": "diffuse", "reflectance": 0.3}}}
    if not inline:
        d["a_group"] = dict(group, id="leafy")
    rng = np.random.default_rng(11)
    for k in range(count):
        xf = (T.translate([float(rng.uniform(-7, 7)), float(rng.uniform(-7, 7)), float(rng.uniform(0.3, 1.8))]) @ T.rotate(rng.normal(size=3).tolist(), float(rng.uniform(0, 360)))
              @ T.scale([float(rng.uniform(1.5, 3.0)), float(rng.uniform(1.5, 3.0)), float(rng.uniform(0.5, 1.5)) * (-1.0 if k % 7 == 0 else 1.0)]))
        d["tree_%02d" % k] = {"type": "instance", "to_world": xf, "group": copy.deepcopy(group) if inline else {"type": "ref", "id": "leafy"}}
    d["wall_a"] = {"type": "rectangle", "to_world": T.translate([0, 6, 1]) @ T.rotate([1, 0, 0], 90) @ T.scale([6.0, 1.0, 1.0]), "bsdf": {"type": "diffuse", "reflectance": 0.7}}
    d["wall_b"] = {"type": "rectangle", "to_world": T.translate([-6, 0, 1]) @ T.rotate([0, 1, 0], 90) @ T.scale([1.0, 6.0, 1.0]), "bsdf": {"type": "diffuse", "reflectance": 0.4}}
    return d


def test_rows_and_structures_agree(gpu_rgb, monkeypatch):
    """`volpath`: ring, flat and nested kernels, and list / BVH at the scene level and inside the group, all one film.  The scene level
    has 75 primitives (the slab's 12 triangles, the ground, two walls, 60 instances), the group 51: thresholds 100, 60 and 0 give
    list / list, BVH / list and BVH / BVH; test_list_over_bvh has the fourth."""
    d = grove()
    film, st = render(gpu_rgb.load_dict(d))
    assert st["textured"] == 2 and st["kernel_variant"] == 11024 and film[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
        other, so = render(gpu_rgb.load_dict(d))
        assert so["textured"] == 2 and so["kernel_variant"] == row
        assert np.array_equal(bits(film), bits(other)), kernel
    monkeypatch.delenv("MTSAMD_KERNEL")
    L = A.lib()
    seen = set()
    for threshold in ("100", "60", "0"):
        monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", threshold)
        scene = gpu_rgb.load_dict(d)
        counts, box = (C.c_int32 * 6)(), (C.c_float * 6)()
        A.check(L.mts_debug_scene_geometry(C.byref(scene._desc), counts, box))
        seen.add((counts[4] > 0, counts[5] > counts[4]))
        other, so = render(scene)
        assert so["textured"] == 2
        assert np.array_equal(bits(film), bits(other)), threshold
    assert (True, True) in seen and (False, False) in seen and (True, False) in seen      # BVH / BVH, list / list, BVH / list


def test_list_over_bvh(gpu_rgb, monkeypatch):
    """the fourth combination: a scene level of few primitives walked as a list over a group with a BVH"""
    d = grove(count=20)
    film, _ = render(gpu_rgb.load_dict(d))
    monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", "45")
    scene = gpu_rgb.load_dict(d)
    L = A.lib()
    counts, box = (C.c_int32 * 6)(), (C.c_float * 6)()
    A.check(L.mts_debug_scene_geometry(C.byref(scene._desc), counts, box))
    assert counts[4] == 0 and counts[5] > 0                                 # list / BVH
    other, so = render(scene)
    assert so["textured"] == 2 and np.array_equal(bits(film), bits(other))
    monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", "0")
    assert np.array_equal(bits(film), bits(render(gpu_rgb.load_dict(d))[0]))


def test_path_flat_against_nested(gpu_rgb, monkeypatch):
    d = grove(slab=False)
    film, st = render(gpu_rgb.load_dict(d))
    assert st["textured"] == 2 and st["kernel_variant"] == 1 and film[..., :3].std() > 0
    monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    other, so = render(gpu_rgb.load_dict(d))
    assert so["textured"] == 2 and so["kernel_variant"] == 0
    assert np.array_equal(bits(film), bits(other))


# ================================================================ 4. sharing
def test_references_render_what_inline_copies_render(gpu_rgb):
    shared, copies = gpu_rgb.load_dict(grove(count=12, size=16)), gpu_rgb.load_dict(grove(count=12, size=16, inline=True))
    assert shared._desc.shape_count == 3 + 12 + 2 + 2 and copies._desc.shape_count == 12 * 4 + 2 + 2      # group and members, instances, slab and ground, walls
    film, st = render(shared)
    other, so = render(copies)
    assert st["textured"] == so["textured"] == 2
    assert np.array_equal(bits(film), bits(other))
    assert digest(shared) != digest(copies)


# ================================================================ 5. full transport against the independent float64 estimator
@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0)])
def test_grove_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    """Five placements of one group in the box -- different rotations, an uneven scale, a mirror -- against twenty world-space
    primitives worked out by hand; `path` in the flat INST loop, `volpath` in the nested INST kernel; test_independent_surface_pin's
    own acceptance"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = problems_instance.box_grove()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 2)}, seen
    assert_agrees(mean, var, gm, gv, "hip box with five instances %s" % integrator)


@pytest.mark.parametrize("mutation", ["unscaled", "unmirrored", "order"])
def test_pin_rejects_a_wrong_placement(gpu_rgb, monkeypatch, mutation):
    """the mutations this pin must reject: one instance without its scale, one without its mirror, one with scale and rotation in
    the wrong order"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), problems_instance.box_grove(mutation=mutation)[0], 16, 1024)
    assert rejected(mean, var, gm, gv, "hip box with five instances, %s" % mutation)


# ================================================================ 6. update in place
def test_update_of_a_member_s_material_is_a_fresh_load(gpu_rgb):
    a = grove(count=12, size=16)
    a["a_bark"] = {"type": "diffuse", "id": "bark", "reflectance": {"type": "rgb", "value": [0.2, 0.6, 0.1]}}
    a["a_group"]["leaf"]["bsdf"] = {"type": "ref", "id": "bark"}

    def assert_is_fresh(scene, d):
        film, st = render(scene)
        fresh = gpu_rgb.load_dict(d)
        fresh_film, fresh_st = render(fresh)
        assert digest(scene) == digest(fresh)
        assert st["kernel_variant"] == fresh_st["kernel_variant"] and st["textured"] == fresh_st["textured"] == 2
        assert np.array_equal(bits(film), bits(fresh_film))
        return film
    scene = gpu_rgb.load_dict(a)
    first = assert_is_fresh(scene, a)
    params = gpu_rgb.traverse(scene)
    with pytest.raises(RuntimeError, match="geometry updates are not supported yet"):
        params["tree_03.to_world"] = T.translate([0, 0, 1])
    params["bark.reflectance.value"] = [0.8, 0.1, 0.3]
    params.update()
    b = copy.deepcopy(a)
    b["a_bark"]["reflectance"]["value"] = [0.8, 0.1, 0.3]
    second = assert_is_fresh(scene, b)
    assert not np.array_equal(bits(first), bits(second))


# ================================================================ 7. memory
def test_instances_cost_the_records_of_one_group(gpu_rgb):
    """256 instances of a 4 096-face grid mesh (64 x 32 cells of two triangles).  Expanded, 4 096 x 256 faces x (64 B walk + 96 B
    attributes + 36 B triangle, csrc/dscene.h) = 205 MB; instanced, about 1 MB of records -- the margin is for allocation granularity."""
    import torch
    nx, ny = 64, 32
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, nx + 1), np.linspace(-0.5, 0.5, ny + 1))
    pos = np.c_[gx.ravel(), gy.ravel(), 0.05 * np.sin(7 * gx.ravel()) * np.cos(5 * gy.ravel())].astype(np.float32)
    faces = np.array([f for j in range(ny) for i in range(nx) for f in ([j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1],
                                                                          [j * (nx + 1) + i, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i])], np.uint32)
    assert len(faces) == 4096
    d = scenes.c1_cornell(16, 16, 1)
    d["a_group"] = {"type": "shapegroup", "id": "sheet", "sheet": {"type": "mesh", "vertex_positions": pos, "faces": faces, "bsdf": {"type": "diffuse", "reflectance": 0.5}}}
    for k in range(256):
        d["sheet_%03d" % k] = {"type": "instance", "group": {"type": "ref", "id": "sheet"},
                               "to_world": T.translate([-4 + 8 * (k % 16) / 15.0, -4 + 8 * (k // 16) / 15.0, 0.5 + 0.02 * k]) @ T.rotate([1, 1, 0], 3.0 * k) @ T.scale(0.6)}
    warm = gpu_rgb.load_dict(scenes.c1_cornell(16, 16, 1))                  # the context and the library's own buffers exist before the measurement
    render(warm)
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    scene = gpu_rgb.load_dict(d)
    torch.cuda.synchronize()
    used = free_before - torch.cuda.mem_get_info()[0]
    print("free device memory consumed by load_dict: %.2f MB" % (used / 2 ** 20))
    assert used < 32 * 2 ** 20
    film, st = render(scene)
    assert st["textured"] == 2 and np.isfinite(film).all() and film[..., :3].sum() > 0
