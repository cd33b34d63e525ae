"""`blendbsdf` on the device (run with -m gpu on an MI355X).  The oracle knows no blend, so it is pinned as the textures are:

  1. identities -- a blend that must be the scene's own BSDF (weight 0 / 1 beside a decoy, two equal children under any weight):
     the film is the oracle's film of the unblended dictionary, bit for bit;
  2. a closed form -- two diffuse children under a directional emitter, `max_depth` = 2: every sample is
     ((1 - w) rho_0 + w rho_1) E cos(theta) / pi, w = clamp(eval_1 of the weight) restated here in float64;
  3. the table's rows (ring, flat, nested) render the same film bit for bit;
  4. the independent float64 estimator's existing fixtures, with materials re-expressed as blends that are the same material in
     expectation -- which pins the selection probabilities and the unnormalised weight of the chosen child;
  5. an update in place is a fresh load."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.kernel_rows as kr
import tests.oracle_binding as ob
import tests.test_gpu_textures as gt
from tests.independent import problems_surface, problems_textured
from tests.sheet_shared import WEIGHTS
from tests.test_gpu_textures import ATOL, CONSTANT_SCENES, IRRADIANCE, MARGIN, N_RAYS, SUN, assert_is_fresh, bits, measured_rho, render
from tests.test_independent_surface_pin import assert_agrees, fixture_for, load_surf_pin, rejected, rgb_estimate
from tests.test_independent_textured_pin import hip_render, load_pin

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

W22 = np.array([[0.0, 1.0], [0.5, 0.5]], np.float32)                    # the 2 x 2 weight bitmap of the identities: 0, 1, 0.5, 0.5


# ================================================================ 1. identities against the oracle's film of the unblended dictionary
def decoy_for(bsdf):
    """a BSDF of another type and colour than the scene's own"""
    if bsdf["type"] == "diffuse":
        return {"type": "rpv", "rho_0": [0.3, 0.5, 0.2], "k": 0.7, "g": 0.1}
    return {"type": "diffuse", "reflectance": [0.9, 0.2, 0.4]}


def blended_copy(d, identity):
    """every diffuse / rpv BSDF of the dictionary's shapes replaced by a blend that is that BSDF"""
    out = copy.deepcopy(d)
    count = 0
    for key, shape in d.items():
        own = shape.get("bsdf") if isinstance(shape, dict) else None
        if not own or own["type"] not in ("diffuse", "rpv"):
            continue
        same = lambda: copy.deepcopy(own)
        out[key]["bsdf"] = {
            "weight_0": {"type": "blendbsdf", "weight": 0.0, "a_own": same(), "b_decoy": decoy_for(own)},
            "weight_1": {"type": "blendbsdf", "weight": 1.0, "a_decoy": decoy_for(own), "b_own": same()},
            "equal_half": {"type": "blendbsdf", "weight": 0.5, "x": same(), "y": same()},
            "equal_bitmap": {"type": "blendbsdf", "x": same(), "y": same(),
                             "weight": {"type": "bitmap", "data": W22, "filter_type": "nearest", "to_uv": T.scale([3.0, 5.0, 1.0])}},
        }[identity]
        count += 1
    assert count >= 1
    return out


_ORACLE = {}


def oracle_film(name, integrator):
    """computed once per scene and integrator, shared by the identities, left unchanged"""
    if (name, integrator) not in _ORACLE:
        d = CONSTANT_SCENES[name][0]()
        d["integrator"]["type"] = integrator
        _ORACLE[(name, integrator)] = ob.OracleScene(d).render()
    return _ORACLE[(name, integrator)]


@pytest.mark.parametrize("identity", ["weight_0", "weight_1", "equal_half", "equal_bitmap"])
@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
@pytest.mark.parametrize("name", sorted(CONSTANT_SCENES))
def test_identities_equal_the_oracle(gpu_rgb, name, integrator, identity):
    """A weight of exactly 0 meets sample1 == 0 with probability 2^-24 per draw, where the reference divides 0 by 0 and the decoy
    samples; no seed used here hits it (the films are equal), so none had to be changed."""
    d = CONSTANT_SCENES[name][0]()
    d["integrator"]["type"] = integrator
    scene = gpu_rgb.load_dict(blended_copy(d, identity))
    assert any(scene._desc.bsdfs[i].type == A.BSDF_BLEND for i in range(scene._desc.bsdf_count))
    film, st = render(scene)
    ref = oracle_film(name, integrator)
    print("%s %s %s: values differing from the oracle's: %d of %d" % (name, integrator, identity, int(np.sum(bits(film) != bits(ref))), film.size))
    assert st["textured"] == 1
    if integrator == ("path" if name == "c1" else "volpath"):                # the scene's own integrator
        assert st["kernel_variant"] == CONSTANT_SCENES[name][1]           # the row the unblended scene gets on the general unit
    assert np.array_equal(bits(film), bits(ref))


# ================================================================ 2. closed form
RHO_0, RHO_1 = np.array([0.15, 0.55, 0.35]), np.array([0.85, 0.25, 0.6])
LUMINANCE = np.array([0.212671, 0.715160, 0.072169])                      # core/spectrum.h:246-248


def weight_eval(weight, uv):
    """clamp(eval_1(si), 0, 1) (blendbsdf.cpp:162-164), float64 -> the weight and the distance to the lookup's nearest discontinuity"""
    if not isinstance(weight, dict):
        return np.full(len(uv), float(weight)), np.full(len(uv), np.inf)
    value, edge = gt.texture_eval(weight, uv)
    data = np.asarray(weight.get("data", 0.0))
    w = value @ LUMINANCE if data.ndim == 3 else value[:, 0]             # bitmap.cpp:285-302
    return np.clip(w, 0.0, 1.0), edge


def blend_case(surface, weight_name, integrator="path", medium=False):
    """test_gpu_textures.closed_form_case with the surface's BSDF a blend of two diffuse children -> dictionary, rho (n, 3), cos(theta)"""
    gt.RNG = np.random.default_rng(2024)                                  # as closed_form_case: the same rays whichever cases run
    shape, p, uv, normal, seam = gt.SURFACES[surface](400)
    weight = WEIGHTS[weight_name]
    w, edge = weight_eval(weight, uv)
    cos_sun = normal @ -SUN
    keep = np.flatnonzero((edge >= MARGIN) & (seam >= 0.02) & (cos_sun > 0.2))[:N_RAYS]
    assert len(keep) == N_RAYS, "not enough rays away from the discontinuities"
    p, normal, w, cos_sun = p[keep], normal[keep], w[keep], cos_sun[keep]
    tilt = normal + 0.3 * np.cross(normal, [0.3, 0.5, 0.8])
    tilt /= np.linalg.norm(tilt, axis=1)[:, None]
    origins, directions = p + 1.5 * tilt, -tilt
    assert np.abs(np.r_[origins.ravel(), p.ravel()]).max() <= 4.0            # ATOL is derived for coordinates <= 4
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    bsdf = {"type": "blendbsdf", "weight": copy.copy(weight), "bsdf_a": {"type": "diffuse", "reflectance": RHO_0.tolist()},
            "bsdf_b": {"type": "diffuse", "reflectance": RHO_1.tolist()}}
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": 2},
         "sensor": {"type": "mradiancemeter", "origins": fmt(origins), "directions": fmt(directions),
                    "film": {"type": "hdrfilm", "width": N_RAYS, "height": 1, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}},
         "surface": dict(shape, bsdf=bsdf),
         "sun": {"type": "directional", "direction": SUN.tolist(), "irradiance": IRRADIANCE}}
    if medium:
        # a medium thin enough to change nothing (optical depth < 1e-7 across the scene) puts `volpath` on its ring row
        xf = T.translate([-8, -8, -8]) @ T.scale(16.0)
        grid = lambda v: {"type": "gridvolume", "data": np.full((2, 2, 2), v, np.float32), "to_world": xf}
        d["air"] = {"type": "cube", "to_world": T.scale(8.0), "bsdf": {"type": "null"},
                    "interior": {"type": "heterogeneous", "sigma_t": grid(1e-9), "albedo": grid(0.5), "phase": {"type": "isotropic"}}}
    rho = (1.0 - w)[:, None] * RHO_0 + w[:, None] * RHO_1
    return d, rho, cos_sun


def test_the_clamp_case_reaches_both_ends():
    """(no device needed, but it belongs to the cases below) texels -0.5 and 1.5 are met, so rho is rho_0 and rho_1 at some rays"""
    d, rho, cos_sun = blend_case("rectangle", "nearest_clamped")
    assert np.any(np.all(rho == RHO_0, axis=1)) and np.any(np.all(rho == RHO_1, axis=1))


# The bound: test_gpu_textures.ATOL (1e-4: the texture lookup's error for these shapes and texel counts); the blend adds two roundings
# of values <= 1 (~1.2e-7), which that bound's factor of five covers.
@pytest.mark.parametrize("weight", sorted(WEIGHTS))
@pytest.mark.parametrize("surface", ["rectangle", "disk", "sphere", "quad_uv"])
def test_closed_form(gpu_rgb, surface, weight):
    d, rho, cos_sun = blend_case(surface, weight)
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s / %s: max |rho - expected| = %.3g" % (surface, weight, np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == 1                 # `path`: the flat row, in its TEX loop
    assert np.abs(got - rho).max() <= ATOL


@pytest.mark.parametrize("weight", sorted(WEIGHTS))
@pytest.mark.parametrize("surface", ["rectangle", "disk", "sphere", "quad_uv"])
def test_closed_form_mono(gpu_rgb, surface, weight):
    """gpu_mono: colours are their luminance, a colour weight bitmap is reduced to its luminance by the loader"""
    d, rho, cos_sun = blend_case(surface, weight)
    gpu_rgb.set_variant("gpu_mono")
    try:
        film, st = render(gpu_rgb.load_dict(d))
    finally:
        gpu_rgb.set_variant("gpu_rgb")
    w = (rho[:, 0] - RHO_0[0]) / (RHO_1[0] - RHO_0[0])
    lum = (1.0 - w) * (RHO_0 @ LUMINANCE) + w * (RHO_1 @ LUMINANCE)
    got = measured_rho(film, cos_sun, mono=True)
    print("mono %s / %s: max |rho - expected| = %.3g" % (surface, weight, np.abs(got[:, 0] - lum).max()))
    assert st["textured"] == 1 and np.abs(got[:, 0] - lum).max() <= ATOL


@pytest.mark.parametrize("weight", sorted(WEIGHTS))
@pytest.mark.parametrize("how,row", [("nested", 0), ("volpath", 0), ("volpathmis", 0), ("ring", 11024)])
def test_closed_form_other_rows(gpu_rgb, monkeypatch, how, row, weight):
    """the rectangle through the nested TEX kernel (`path` under MTSAMD_KERNEL=nested, the volumetric integrators without a medium)
    and through the ring TEX kernel (`volpath` inside a medium of no effect)"""
    d, rho, cos_sun = blend_case("rectangle", weight, integrator="path" if how == "nested" else "volpath" if how == "ring" else how, medium=how == "ring")
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s / %s: max |rho - expected| = %.3g" % (how, weight, np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == row
    assert np.abs(got - rho).max() <= ATOL


@pytest.mark.parametrize("weight", sorted(WEIGHTS))
def test_closed_form_through_the_sample_entry(gpu_rgb, weight):
    """SamplingIntegrator::sample (mts_sample) of a blend scene runs the TEX kernel -- also under a constant weight, without a texture record"""
    d, rho, cos_sun = blend_case("rectangle", weight)
    scene = gpu_rgb.load_dict(d)
    o = np.array([float(x) for x in d["sensor"]["origins"].split(",")], np.float32).reshape(-1, 3)
    w = np.array([float(x) for x in d["sensor"]["directions"].split(",")], np.float32).reshape(-1, 3)
    n = len(o)
    rgb, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    cols = [np.ascontiguousarray(a) for a in (o[:, 0], o[:, 1], o[:, 2], w[:, 0], w[:, 1], w[:, 2])]
    A.check(A.lib().mts_sample(scene._handle, n, 0, *[c.ctypes.data_as(A.fp) for c in cols], rgb.ctypes.data_as(A.fp), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert valid.all()
    assert np.abs(rgb.astype(np.float64) * np.pi / (IRRADIANCE * cos_sun[:, None]) - rho).max() <= ATOL


# ================================================================ 3. the formulations agree
def varying_blend_c3(width, height):
    d = scenes.c3_heterogeneous(width, height, 8, res=8)
    weight = {"type": "bitmap", "data": np.random.default_rng(11).random((4, 4), dtype=np.float32), "to_uv": T.scale([7.0, 5.0, 1.0])}
    d["ground"]["bsdf"] = {"type": "blendbsdf", "weight": weight, "background": {"type": "diffuse", "reflectance": [0.6, 0.5, 0.3]},
                           "target": {"type": "rpv", "rho_0": [0.1, 0.3, 0.05], "k": 0.6, "g": -0.2}}
    return d


@pytest.mark.parametrize("width,height", [(16, 16), (13, 11)])
def test_rows_agree(gpu_rgb, monkeypatch, width, height):
    d = varying_blend_c3(width, height)
    film, st = render(gpu_rgb.load_dict(d))
    assert st["textured"] == 1 and st["kernel_variant"] == 11024             # the ring row ran, in its TEX kernel
    assert film[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
        other, so = render(gpu_rgb.load_dict(d))
        assert so["textured"] == 1 and so["kernel_variant"] == row
        assert np.array_equal(bits(film), bits(other)), kernel


def test_wavefront_streams_and_counters(gpu_rgb, monkeypatch):
    d = varying_blend_c3(16, 16)
    d["sensor"]["sampler"]["wavefront"] = True
    scene = gpu_rgb.load_dict(d)
    film, st = render(scene)
    assert st["textured"] == 1 and np.isfinite(film).all() and film[..., :3].std() > 0
    sensor = scene.sensors()[0]
    assert scene.integrator().render(scene, sensor, collect_counters=True)
    assert scene.integrator().last_stats["n_iter"] > 0
    assert np.array_equal(bits(film), bits(np.array(sensor.film().bitmap(raw=True))))      # the counting instantiation: the same film
    monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    nested, sn = render(gpu_rgb.load_dict(d))
    assert sn["textured"] == 1 and sn["kernel_variant"] == 0
    assert np.array_equal(bits(film), bits(nested))


# ================================================================ 4. the independent estimator's existing fixtures
def as_blend(bsdf, f0=1.2, f1=0.7, w=0.4):
    """diffuse rho -> blend(diffuse f0 rho, diffuse f1 rho; w): (1 - w) f0 + w f1 = 1, the same material in expectation"""
    assert abs((1 - w) * f0 + w * f1 - 1.0) < 1e-12
    rho = np.asarray(bsdf["reflectance"]["value"], np.float64)
    assert np.all(f0 * rho <= 1.0) and np.all(f1 * rho <= 1.0)
    return {"type": "blendbsdf", "weight": w, "bsdf_a": {"type": "diffuse", "reflectance": (f0 * rho).tolist()},
            "bsdf_b": {"type": "diffuse", "reflectance": (f1 * rho).tolist()}}


def blended_box(integrator):
    d = problems_surface.box()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    walls = [k for k, v in d.items() if isinstance(v, dict) and isinstance(v.get("bsdf"), dict) and v["bsdf"]["type"] == "diffuse"]
    assert sorted(walls) == ["back", "ceiling", "floor", "left", "right"]
    for k in walls:
        d[k]["bsdf"] = as_blend(d[k]["bsdf"])
    return d


@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0)])
def test_blended_box_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var, _ = load_surf_pin(fixture_for("box", integrator))
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), blended_box(integrator), 16, 1024)
    assert seen == {(row, 1)}, seen
    assert_agrees(mean, var, gm, gv, "hip blended box %s" % integrator)


def blended_textured_box(exchanged=False):
    """box_textured with the right wall's checkerboard reflectance as a blend of its two colours under a 0 / 1 checkerboard weight, and the
    floor as a weight-0.5 blend of two equal children that both carry the FLOOR bitmap"""
    d = problems_textured.box_textured()[0]
    checker = d["right"]["bsdf"]["reflectance"]
    c0, c1 = {"type": "diffuse", "reflectance": list(checker["color0"])}, {"type": "diffuse", "reflectance": list(checker["color1"])}
    # the weight is 0 where the reflectance was color0 (bsdf_a) and 1 where it was color1 (bsdf_b)
    d["right"]["bsdf"] = {"type": "blendbsdf", "weight": {"type": "checkerboard", "color0": 0.0, "color1": 1.0, "to_uv": checker["to_uv"]},
                          "bsdf_a": c1 if exchanged else c0, "bsdf_b": c0 if exchanged else c1}
    floor = d["floor"]["bsdf"]
    d["floor"]["bsdf"] = {"type": "blendbsdf", "weight": 0.5, "bsdf_a": copy.deepcopy(floor), "bsdf_b": copy.deepcopy(floor)}
    return d


@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0)])
def test_blended_textured_box_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = blended_textured_box()
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 1)}, seen
    assert_agrees(mean, var, gm, gv, "hip blended textured box %s" % integrator)


def test_pin_rejects_exchanged_children(gpu_rgb, monkeypatch):
    """the mutation this pin must reject: bsdf_0 and bsdf_1 of the right wall's blend exchanged"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), blended_textured_box(exchanged=True), 16, 1024)
    assert rejected(mean, var, gm, gv, "hip blended textured box, children exchanged")


# ================================================================ 5. update in place is a fresh load
def test_update_in_place(gpu_rgb):
    a = varying_blend_c3(16, 16)
    a["slab"]["bsdf"] = {"type": "null"}
    a["wall"] = {"type": "rectangle", "to_world": T.translate([0, 0, 0.5]) @ T.scale(20.0),
                 "bsdf": {"type": "blendbsdf", "weight": 0.3, "bsdf_a": {"type": "diffuse", "reflectance": [0.7, 0.6, 0.2]}, "bsdf_b": {"type": "bilambertian", "reflectance": 0.4, "transmittance": 0.3}}}
    scene = gpu_rgb.load_dict(a)
    first = assert_is_fresh(gpu_rgb, scene, a)
    params = gpu_rgb.traverse(scene)
    new = np.random.default_rng(12).random((4, 4), dtype=np.float32)
    b = copy.deepcopy(a)
    b["wall"]["bsdf"]["weight"] = 0.65
    b["wall"]["bsdf"]["bsdf_a"]["reflectance"] = [0.2, 0.3, 0.8]
    b["ground"]["bsdf"]["weight"]["data"] = new
    b["ground"]["bsdf"]["target"]["k"] = 0.8
    params["wall.bsdf.weight.value"] = 0.65
    params["wall.bsdf.bsdf_0.reflectance.value"] = [0.2, 0.3, 0.8]
    params["ground.bsdf.weight.data"] = new
    params["ground.bsdf.bsdf_1.k.value"] = 0.8
    params.update()
    second = assert_is_fresh(gpu_rgb, scene, b)
    assert not np.array_equal(bits(first), bits(second))
    before = gt.digest(scene)
    params["wall.bsdf.weight.value"] = float("nan")
    with pytest.raises(RuntimeError, match="not finite"):
        params.update()
    assert gt.digest(scene) == before
    assert np.array_equal(bits(render(scene)[0]), bits(second))
    params["wall.bsdf.weight.value"] = 0.3
    params["wall.bsdf.bsdf_0.reflectance.value"] = [0.7, 0.6, 0.2]
    params["ground.bsdf.weight.data"] = a["ground"]["bsdf"]["weight"]["data"]
    params["ground.bsdf.bsdf_1.k.value"] = 0.6
    params.update()
    assert np.array_equal(bits(assert_is_fresh(gpu_rgb, scene, a)), bits(first))
