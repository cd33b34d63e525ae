"""The `cone` shape (src/shapes/cone.cpp) without a GPU: loading from dictionaries and XML, the reference's own fixtures restated
(src/shapes/tests/test_cone.py: test_create, test_bbox), what loader and library refuse, the kernel routing (a scene with a cone anywhere
renders in the INST kernels: no traits, the general unit's row), and the float64 reference of tests/cone_ref.py against itself with the
5 % cap on what its exclusion rules leave out of each ray set."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.cone_ref as cr
from tests.test_blendbsdf import kernel_row
from tests.test_textures import desc_digest, describe, dict_digest, library_refusal, refusal

A = importlib.import_module("eradiate-kernel_amd._capi")
PKG = importlib.import_module("eradiate-kernel_amd")
XML = importlib.import_module("eradiate-kernel_amd.xml_io")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

CONE = {"type": "cone", "to_world": T.translate([0.5, 0.25, 1]) @ T.rotate([1, 2, 3], 40) @ T.scale([0.5, 0.5, 2.0])}


def kinds(desc):
    return [desc.shapes[i].type for i in range(desc.shape_count)]


def geometry(desc):
    counts, box = (C.c_int32 * 6)(), (C.c_float * 6)()
    A.check(A.lib().mts_debug_scene_geometry(C.byref(desc), counts, box))
    return list(counts), np.array(list(box))


def box_with(**shapes):
    d = scenes.c1_cornell(8, 8, 2)
    d.update(copy.deepcopy(shapes))
    return d


def in_a_group(cone=CONE, **more):
    return {"a_group": dict({"type": "shapegroup", "id": "tree", "crown": copy.deepcopy(cone)}, **more),
            "tree_0": {"type": "instance", "to_world": T.translate([0, 0, 3]) @ T.scale([1.0, 2.0, 0.5]), "g": {"type": "ref", "id": "tree"}}}


# ---------------------------------------------------------------- loading
XML_SCENE = """<scene version="2.0.0">
    <bsdf type="diffuse" id="bark"><rgb name="reflectance" value="0.2, 0.4, 0.6"/></bsdf>
    <shape type="cone" name="z_cone"><ref id="bark"/><boolean name="flip_normals" value="true"/>
        <transform name="to_world"><scale x="0.5" y="0.5" z="2"/><rotate x="1" y="2" z="3" angle="40"/><translate x="0.5" y="0.25" z="1"/></transform></shape>
    <shape type="shapegroup" id="tree">
        <shape type="cone" name="crown"><ref id="bark"/><transform name="to_world"><scale x="1" y="1" z="3"/><translate x="0" y="0" z="1"/></transform></shape>
        <shape type="disk" name="ground"><ref id="bark"/></shape>
    </shape>
    <shape type="instance" name="t_0"><ref id="tree"/><transform name="to_world"><scale x="1" y="2" z="0.5"/><translate x="-1" y="0" z="2"/></transform></shape>
    <emitter type="directional"><vector name="direction" x="0" y="0" z="-1"/></emitter>
    <sensor type="perspective"><film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/></film></sensor>
</scene>"""


def test_xml_and_dict_give_the_same_description():
    dx, kx = describe(XML.xml_to_dict(XML_SCENE))
    bark = {"type": "ref", "id": "bark"}
    as_dict = {"type": "scene",
               "bark": {"type": "diffuse", "id": "bark", "reflectance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}},
               "z_cone": dict(CONE, bsdf=bark, flip_normals=True),
               "grp": {"type": "shapegroup", "id": "tree",
                       "crown": {"type": "cone", "bsdf": bark, "to_world": T.translate([0, 0, 1]) @ T.scale([1, 1, 3])},
                       "ground": {"type": "disk", "bsdf": bark}},
               "t_0": {"type": "instance", "g": {"type": "ref", "id": "tree"}, "to_world": T.translate([-1, 0, 2]) @ T.scale([1, 2, 0.5])},
               "sun": {"type": "directional", "direction": [0, 0, -1]},
               "sensor": {"type": "perspective", "film": {"type": "hdrfilm", "width": 4, "height": 4}}}
    dd, kd = describe(as_dict)
    assert A.SHAPE_CONE == 8
    assert kinds(dx) == kinds(dd) == [A.SHAPE_SHAPEGROUP, A.SHAPE_CONE, A.SHAPE_DISK, A.SHAPE_INSTANCE, A.SHAPE_CONE]
    assert dx.shapes[4].flip_normals == 1 and dx.shapes[1].flip_normals == 0 and dx.shapes[0].face_count == 2
    assert desc_digest(dx) == desc_digest(dd) and all(desc_digest(dx)[k] for k in (0, 5, 6))
    # the digest tells a cone's transform and its flag
    turned = copy.deepcopy(as_dict)
    turned["z_cone"]["to_world"] = T.translate([0.5, 0.25, 1]) @ T.rotate([1, 2, 3], 41) @ T.scale([0.5, 0.5, 2.0])
    assert dict_digest(turned)[6] != desc_digest(dd)[6]
    unflipped = copy.deepcopy(as_dict)
    del unflipped["z_cone"]["flip_normals"]
    assert dict_digest(unflipped)[0] != desc_digest(dd)[0] and dict_digest(unflipped)[6] == desc_digest(dd)[6]


def test_traverse_lists_what_it_lists_for_a_sphere():
    keys = {}
    for kind in ("cone", "sphere"):
        d = box_with(thing={"type": kind, "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}}})
        desc, keep = describe(d)
        p = PKG.ParameterMap(desc, keep)
        keys[kind] = [k for k in p.keys() if k.startswith("thing.")]
        with pytest.raises(RuntimeError, match="geometry updates are not supported yet"):
            p["thing.to_world"] = T.translate([0, 0, 1])
    assert keys["cone"] == keys["sphere"] and sorted(keys["cone"]) == ["thing.bsdf.reflectance.value", "thing.to_world"]


# ---------------------------------------------------------------- the reference's fixtures (src/shapes/tests/test_cone.py)
def lone(cone):
    return {"type": "scene", "foo": cone, "sun": {"type": "directional", "direction": [0, 0, -1]},
            "sensor": {"type": "perspective", "film": {"type": "hdrfilm", "width": 4, "height": 4}}}


def test_create():
    desc, keep = describe(lone({"type": "cone"}))
    counts, box = geometry(desc)
    assert counts[:4] == [1, 1, 0, 0]                                      # primitive_count() == 1
    assert np.array_equal(box, [-1, -1, 0, 1, 1, 1])
    # (surface_area() == sqrt(2) pi: no debug entry exposes it; the furnace of tests/test_gpu_cone_pin.py would miss a wrong pdf)


@pytest.mark.parametrize("h", [1, 5, 10])
def test_bbox(h):
    """cone.cpp:113-124: the box of the two end circles of radius r -- at the tip too"""
    for r in [1, 2, 4, 8]:
        desc, keep = describe(lone({"type": "cone", "to_world": T.scale([r, r, h])}))
        counts, box = geometry(desc)
        assert np.allclose(box[:3], [-r, -r, 0.0]) and np.allclose(box[3:], [r, r, h]), (r, h, box)
    # turned by 90 degrees about x the axis lies along -y: the end circles span x and z
    desc, keep = describe(lone({"type": "cone", "to_world": T.translate([1, 2, 3]) @ T.rotate([1, 0, 0], 90) @ T.scale([2, 2, h])}))
    counts, box = geometry(desc)
    assert np.allclose(box, [1 - 2, 2 - h, 3 - 2, 1 + 2, 2, 3 + 2], atol=1e-5), box


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_loader():
    for key, value in (("radius", 0.3), ("p0", [0, 0, 0]), ("p1", [0, 0, 1])):
        msg = refusal(box_with(crown=dict(CONE, **{key: value})))
        assert "unreferenced propert" in msg and key in msg and "\"cone\"" in msg, msg
    assert "unreferenced propert" in refusal(box_with(**in_a_group(dict(CONE, radius=0.3))))
    shear = np.eye(4)
    shear[0, 2] = 0.25
    msg = refusal(box_with(crown={"type": "cone", "to_world": T(shear)}))
    assert "shouldn't contain any shearing" in msg and "crown" in msg and "this backend" in msg, msg
    msg = refusal(box_with(crown={"type": "cone", "to_world": T.scale([1.0, 1.5, 2.0])}))
    assert "shouldn't contain non-uniform scaling along the X and Y axes" in msg and "this backend" in msg, msg
    msg = refusal(box_with(crown={"type": "cone", "to_world": T.scale([1.0, 1.0, -2.0])}))
    assert "shouldn't mirror the cone" in msg and "this backend" in msg, msg
    msg = refusal(box_with(**in_a_group({"type": "cone", "to_world": T.scale([1.0, 1.5, 2.0])})))
    assert "non-uniform scaling" in msg and "a_group.crown" in msg, msg
    lamp = dict(CONE, emitter={"type": "area", "radiance": 1.0})
    msg = refusal(box_with(crown=lamp))
    assert "\"area\" emitter on a cone is not supported by this backend" in msg and "crown" in msg, msg
    assert refusal(box_with(**in_a_group(lamp))) == "Instancing of emitters is not supported"
    spectral = scenes.c5_atmosphere_spectral(8, 8, 2, layers=8)
    spectral["crown"] = copy.deepcopy(CONE)
    msg = refusal(spectral, spectral=True)
    assert "\"cone\"" in msg and "gpu_spectral" in msg and "crown" in msg, msg
    for extra in (dict(crown=CONE), in_a_group()):
        d = box_with(**extra)
        d["integrator"] = {"type": "moment", "nested": d["integrator"]}
        msg = refusal(d)
        assert "moment" in msg and ("\"cone\"" in msg or "\"shapegroup\"" in msg), msg
    d = box_with(crown=CONE)
    d["integrator"] = {"type": "moment", "nested": d["integrator"]}
    assert "\"cone\" (crown) inside a moment integrator's scene" in refusal(d)
    # `cylinder` stays what it was: no plugin of the scene, no member of a group
    assert refusal(box_with(pipe={"type": "cylinder"})) == "Unknown / unsupported plugin \"cylinder\" (key \"pipe\")"
    assert "Tried to add an unsupported object of type \"cylinder\"" in refusal(box_with(**in_a_group(pipe={"type": "cylinder"})))
    # a sensor's target shape: the existing message covers the cone
    d = box_with()
    d["sensor"] = {"type": "distant", "direction": [0, 0, -1], "ray_target": dict(CONE), "film": d["sensor"]["film"], "sampler": d["sensor"]["sampler"]}
    desc, keep = describe(d)
    assert "shape must be a rectangle, a disk or a sphere in this backend" in library_refusal(desc)


def poked(poke, d=None):
    desc, keep = describe(box_with(crown=CONE) if d is None else d)
    poke(desc, kinds(desc).index(A.SHAPE_CONE))
    return library_refusal(desc)


def set_linear(rows):
    def poke(s, i):
        m = np.array(list(s.shapes[i].to_world.matrix), np.float32).reshape(4, 4)
        m[:3, :3] = np.asarray(rows, np.float32)
        inv = np.linalg.pinv(m.astype(np.float64))                         # (a singular matrix has no inverse: the check comes before it is read)
        s.shapes[i].to_world.matrix[:] = [float(x) for x in m.ravel()]
        s.shapes[i].to_world.inverse_transpose[:] = [float(x) for x in inv.T.astype(np.float32).ravel()]
    return poke


def test_refusals_of_the_library():
    assert desc_digest(describe(box_with(crown=CONE))[0])[6] != 0
    assert "unknown shape type" in poked(lambda s, i: setattr(s.shapes[i], "type", 7))           # 7 stays unassigned
    assert "unknown shape type" in poked(lambda s, i: setattr(s.shapes[i], "type", 9))
    assert "shouldn't contain any shearing" in poked(set_linear([[1, 0, 0.25], [0, 1, 0], [0, 0, 2]]))
    assert "non-uniform scaling along the X and Y axes" in poked(set_linear([[1, 0, 0], [0, 1.5, 0], [0, 0, 2]]))
    assert "shouldn't mirror the cone" in poked(set_linear([[1, 0, 0], [0, 1, 0], [0, 0, -2]]))
    assert "radius > 0" in poked(set_linear([[1, 0, 0], [0, 1, 0], [0, 0, 0]]))
    msg = poked(lambda s, i: setattr(s.shapes[i], "emitter", 0))
    assert "an area emitter on a cone is not supported on this backend" in msg and msg.startswith("shape "), msg
    msg = poked(lambda s, i: setattr(s.emitters[0], "shape", i))
    assert "an area emitter on a cone is not supported on this backend" in msg and msg.startswith("emitter 0"), msg
    assert "cone shapes are not supported in the spectral variant" in poked(lambda s, i: setattr(s.integrator, "spectral", 1))
    assert "cone shapes are not supported inside a moment integrator's scene" in poked(lambda s, i: setattr(s.integrator, "moment", 1))
    # inside a group the same checks, and the group's own come first
    msg = poked(lambda s, i: setattr(s.integrator, "moment", 1), box_with(**in_a_group()))
    assert "not supported inside a moment integrator's scene" in msg, msg
    # 1024 shape records: the hit encoding of the INST kernels
    many = box_with(crown=CONE, **{"pad_%04d" % k: {"type": "rectangle", "to_world": T.translate([0.001 * k, 0, 1])} for k in range(1024 - 6 - 1)})
    desc, keep = describe(many)
    assert desc.shape_count == 1024 and desc_digest(desc)[6] != 0
    many["one_more"] = {"type": "rectangle"}
    desc, keep = describe(many)
    msg = library_refusal(desc)
    assert "at most 1024 shape records" in msg and "shape_count = 1025" in msg, msg
    del many["crown"]
    desc, keep = describe(many)
    assert desc_digest(desc)[6] != 0                                      # without the cone the scene has no such limit


# ---------------------------------------------------------------- kernel routing
def choices(desc):
    """traits and row three ways: mts_debug_scene_traits + mts_debug_kernel_choice, mts_debug_sensor_choice, mts_debug_update_plan"""
    L = A.lib()
    t, v = C.c_int32(-1), C.c_int32(-1)
    A.check(L.mts_debug_sensor_choice(C.byref(desc), None, 0, 0, C.byref(t), C.byref(v)))
    by_sensor = (t.value, v.value)
    A.check(L.mts_debug_update_plan(C.byref(desc), C.byref(desc), None, 0, C.byref(t), C.byref(v)))
    assert by_sensor == (t.value, v.value) == kernel_row(desc)
    return by_sensor


@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 11024), ("volpathmis", None)])
def test_traits_and_kernel_row(integrator, row):
    """A scene with a cone and no instance, and one with a cone inside a group, present no traits and take the general unit's row, where
    mts_render runs the INST kernel of that row (mts_stats.textured == 2: tests/test_gpu_cone_rays.py, test_gpu_cone_pin.py); the
    cone-free scene keeps its traits.  `path`: the flat row; `volpath` over a heterogeneous medium: the ring row; `volpathmis`: nested."""
    d = scenes.c3_heterogeneous(8, 8, 2, res=8)
    d["integrator"]["type"] = integrator
    free = choices(describe(d)[0])
    assert free[0] != 0
    plain = dict(d, crown=copy.deepcopy(CONE))
    member = dict(d, **in_a_group())
    lone_group = dict(d, a_group={"type": "shapegroup", "crown": copy.deepcopy(CONE)})      # a cone anywhere: even in a group nobody places
    for dd in (plain, member, lone_group):
        got = choices(describe(dd)[0])
        assert got[0] == 0, got
        if row is not None:
            assert got[1] == row, got
        # an instanced scene without a cone goes where it went: the same row
        assert got == choices(describe(dict(d, **in_a_group({"type": "rectangle"})))[0])
    assert choices(describe(d)[0]) == free


# ---------------------------------------------------------------- cone_ref against itself
@pytest.mark.parametrize("which", sorted(cr.SCENES))
def test_reference_hits_lie_on_their_cones(which):
    d, prims = cr.scene(which)
    seen = 0
    for name in cr.ray_sets(which):
        ref = cr.reference(which, name)
        for i, (_, pl) in enumerate(prims):
            sel = ref["winner"] == i
            if not isinstance(pl.prim, cr.Cone) or not sel.any():
                continue
            cone, q = pl.prim, (ref["p"][sel] - pl.t) @ pl.Pi.T            # the hit in the cone's own space
            assert np.abs(cone.off_surface(q)).max() <= 1e-12
            h = (q - cone.base) @ cone.u
            assert np.all((h >= 0.0) & (h < cone.l))
            n = cone.normal(q)
            line = (cone.apex - q) / np.linalg.norm(cone.apex - q, axis=1, keepdims=True)       # the generator through the hit
            e, rho = cone.radial(q)
            # (the normal's radial part is e / rho: a point that lies on the cone to 1e-12 gives its direction to 1e-12 / rho)
            tol = 1e-12 * np.maximum(1.0, 8.0 / rho)
            assert np.all(np.abs((n * line).sum(1)) <= tol) and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12
            assert np.all((n * e).sum(1) * (-1.0 if cone.flip else 1.0) > 0.0)                   # outwards (inwards when flipped)
            # the placed normal stays orthogonal to the placed surface: to the images of the generator and of the tangent about the axis
            nw = pl.normal(ref["p"][sel])
            tangent = np.cross(cone.u, e) @ pl.P.T
            scale = np.abs(pl.P).sum()
            assert np.all(np.abs((nw * (line @ pl.P.T)).sum(1)) <= scale * tol) and np.all(np.abs((nw * tangent).sum(1)) <= scale * tol * np.maximum(rho, 1e-12))
            seen += int(sel.sum())
    assert seen >= 1024


def test_reference_against_a_brute_force_march():
    """the closed form against a construction that solves nothing: the sign of r (l - z) / l - |xy| sampled along the ray"""
    cone = cr.Cone([0.25, -0.5, 0.125], [0.3, -0.2, 1.0], 0.75, 1.5)
    rng = np.random.default_rng(11)
    o = cr._unit(rng, 256) * 3.0
    d = cone.point(rng) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ref = cr.reference_hits([("c", cr.Placed(cone))], o, d)
    o, d = o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)
    ts = np.linspace(0.0, 6.0, 60001)
    for i in range(0, 256, 8):
        p = o[i] + ts[:, None] * d[i]
        h = (p - cone.base) @ cone.u
        f = np.where((h >= 0.0) & (h < cone.l), cone.off_surface(p), np.nan)
        cross = np.flatnonzero(np.isfinite(f[:-1]) & np.isfinite(f[1:]) & (np.sign(f[:-1]) != np.sign(f[1:])))
        if np.isfinite(ref["t"][i]) and ref["rim"][i] > 1e-2:
            assert len(cross) and abs(ts[cross[0]] - ref["t"][i]) <= 2e-4, i
        elif not np.isfinite(ref["t"][i]) and ref["rim"][i] > 1e-2:
            assert len(cross) == 0, i


@pytest.mark.parametrize("which", sorted(cr.SCENES))
def test_the_rules_leave_out_at_most_five_percent(which):
    """with a generous E_t (1e-5: ten times what instance_rays.fp32_scale measures) the float64 reference alone stays inside the cap"""
    for name, rays in cr.ray_sets(which).items():
        assert all(len(a) == cr.N_RAYS for a in rays)
        ref = cr.reference(which, name)
        out = float(np.mean(~cr.kept(ref, 1e-5)))
        hits = int(np.isfinite(ref["t"]).sum())
        print("%s %s: %d hits, %.2f %% left out" % (which, name, hits, 100 * out))
        assert out <= cr.MAX_LEFT_OUT, (which, name, out)
        assert hits >= cr.N_RAYS // 10
    for r in cr.GRID_R:
        for l in cr.GRID_L:
            o, d = cr.grid_rays(r, l)
            ref = cr.reference_hits([("foo", cr.Placed(cr.Cone([0, 0, 0], cr.Z, r, l)))], o, d)
            assert len(o) == 100 and np.mean(~cr.kept(ref, 1e-5)) <= 0.2 and np.isfinite(ref["t"]).sum() >= 20


# ---------------------------------------------------------------- the independent estimator's cone problem (tests/independent/problems_cone.py)
def load_pin():
    import os
    from tests.test_independent_pin import GOLDEN
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_conifers_16x16.npz"))
    return z["mean"], z["var"], z


def test_problem_is_well_posed():
    from tests.independent import problems_cone, surface
    d, scene, cam, max_depth, vertices = problems_cone.conifers()
    mean, var, z = load_pin()
    assert mean.shape == (16, 16, 3) and np.all(mean > 0)
    assert int(z["walks"]) == int(z["per_pixel"]) * 256 and float(z["seconds"]) > 0
    se = np.sqrt(var.sum((0, 1))) / 256 / mean.mean((0, 1))
    assert se.max() < 1.5e-3                                              # below 0.15 % per channel
    assert max(p.material.max_albedo() for p in scene.prims) == problems_cone.MAX_ALBEDO
    assert surface.remainder_bound(scene, vertices) < 1e-4 * mean.mean()
    kinds_by_hand = [type(p).__name__ for p in scene.prims]
    assert kinds_by_hand.count("Cone") == 7 and kinds_by_hand.count("Box") == 3 and kinds_by_hand.count("Disk") == 2
    desc, keep = describe(d)
    assert kinds(desc).count(A.SHAPE_CONE) == 2 and kinds(desc).count(A.SHAPE_INSTANCE) == 3 and kernel_row(desc) == (0, 1)
    # the walk's cone against cone_ref's, which is written from the same definition a second time: one cone under an uneven placement
    from tests.independent.problems_instance import linear_part
    t, axis, angle, s = problems_cone.PLACES[2]
    P = linear_part(axis, angle, np.asarray(s, np.float64))
    mine = cr.Placed(cr.Cone(problems_cone.CROWN["base"], cr.Z, problems_cone.CROWN["r"], problems_cone.CROWN["l"]), P, t)
    theirs = [p for p in scene.prims if type(p).__name__ == "Cone" and not p.inward][2]
    rng = np.random.default_rng(5)
    o = cr._unit(rng, 512) * 4.0 + np.asarray(t)
    w = np.array([mine.point(rng) for _ in range(512)]) - o
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    o, w = o.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)
    ref = cr.reference_hits([("c", mine)], o, w)
    got = theirs.hit(o, w)
    hit = np.isfinite(ref["t"])
    assert hit.sum() > 400 and np.array_equal(np.isfinite(got), hit) and np.abs(got[hit] - ref["t"][hit]).max() < 1e-12
    assert np.abs(theirs.normal(ref["p"][hit]) - ref["n"][hit]).max() < 1e-9


def test_fixture_comes_from_the_committed_estimator():
    """A short live run of the estimator agrees with its fixture (same code, other seed, 64 walks per pixel)."""
    import math
    from tests.independent import problems_cone, surface
    from tests.test_independent_pin import z_test
    mean, var, _ = load_pin()
    _, scene, cam, max_depth, vertices = problems_cone.conifers()
    m, v = surface.render(scene, cam, 64, 77, max_depth, vertices)
    for c in range(3):
        se = math.sqrt(v[..., c].sum() + var[..., c].sum()) / m[..., c].size
        assert abs(m[..., c].mean() - mean[..., c].mean()) < 4 * se
        tm, tv = m[..., c].reshape(4, 4, 4, 4).mean((1, 3)), v[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        fm, fv = mean[..., c].reshape(4, 4, 4, 4).mean((1, 3)), var[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        p, alpha, _ = z_test(tm, tv, fm, fv)
        assert (p > alpha).all()


def test_update_of_a_cone_s_material_is_a_fresh_load():
    """mts_scene_update: geometry is frozen as for every shape; a BSDF on a cone is rewritten in place and the scene stays on its kernels"""
    paint = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}}
    d = box_with(crown=dict(CONE, bsdf=paint))
    desc, keep = describe(d)
    p = PKG.ParameterMap(desc, keep)
    p["crown.bsdf.reflectance.value"] = [0.7, 0.1, 0.3]
    p.update()
    fresh = copy.deepcopy(d)
    fresh["crown"]["bsdf"]["reflectance"]["value"] = [0.7, 0.1, 0.3]
    fd, fk = describe(fresh)
    assert desc_digest(desc) == desc_digest(fd) and kernel_row(desc) == kernel_row(fd) == (0, 1)
