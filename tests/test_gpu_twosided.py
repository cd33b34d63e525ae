"""`twosided` on the device (run with -m gpu on an MI355X).  The oracle knows no adapter, so it is pinned as blends are:

  6. identities -- an adapter whose front side is the scene's own BSDF, in scenes where no path reaches a back side: the film is
     the oracle's film of the unwrapped dictionary, bit for bit;
  7. a closed form -- a sheet with diffuse rho_0 in front and rho_1 behind under a directional emitter, `max_depth` = 2: every
     sample is rho_side E |cos(theta)| / pi when rays and sun meet the same side, 0 otherwise;
  8. mirror symmetry -- a one-child adapter on a rectangle in z = 0 renders the same film, bit for bit, when rays and sun are
     mirrored in z: the adapter's flips are exact negations (this covers the back side of rpv);
  9. the table's rows (ring, flat, nested) render the same film bit for bit with a sheet hit from both sides: the ring kernel's
     per-lane choice of the child;
 10. full transport against the independent float64 estimator (tests/independent/problems_twosided.py);
 11. an update in place is a fresh load."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.kernel_rows as kr
import tests.test_gpu_textures as gt
from tests.independent import problems_twosided
from tests.test_gpu_blendbsdf import decoy_for, oracle_film
from tests.test_gpu_textures import ATOL, CONSTANT_SCENES, IRRADIANCE, MARGIN, N_RAYS, SUN, assert_is_fresh, bits, measured_rho, render
from tests.test_independent_surface_pin import assert_agrees, rejected, rgb_estimate
from tests.test_independent_textured_pin import hip_render
from tests.test_twosided import load_pin

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f


# ================================================================ 6. identities against the oracle's film of the unwrapped dictionary
def wrapped_copy(d, wrapping):
    """every diffuse / rpv BSDF of the dictionary's shapes wrapped in a twosided whose front side is that BSDF"""
    out = copy.deepcopy(d)
    count = 0
    for key, shape in d.items():
        own = shape.get("bsdf") if isinstance(shape, dict) else None
        if not own or own["type"] not in ("diffuse", "rpv"):
            continue
        same = lambda: copy.deepcopy(own)
        out[key]["bsdf"] = {
            "one_child": {"type": "twosided", "own": same()},
            "decoy_behind": {"type": "twosided", "a_own": same(), "b_decoy": decoy_for(own)},
            "blend_child": {"type": "twosided", "child": {"type": "blendbsdf", "weight": 0.0, "a_own": same(), "b_decoy": decoy_for(own)}},
        }[wrapping]
        count += 1
    assert count >= 1
    return out


@pytest.mark.parametrize("wrapping", ["one_child", "decoy_behind", "blend_child"])
@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
@pytest.mark.parametrize("name", sorted(CONSTANT_SCENES))
def test_identities_equal_the_oracle(gpu_rgb, name, integrator, wrapping):
    """In these scenes no path can reach a back side, so the decoy behind is never evaluated and a one-sided BSDF is its own
    two-sided version: the cornell box is closed but for the opening the camera looks through, and is seen from inside (a path that
    leaves through the opening meets nothing); the grounds of c3 and c4 lie below everything that scatters and extend beyond the
    media, so nothing arrives from below them."""
    d = CONSTANT_SCENES[name][0]()
    d["integrator"]["type"] = integrator
    scene = gpu_rgb.load_dict(wrapped_copy(d, wrapping))
    assert any(scene._desc.bsdfs[i].type == A.BSDF_TWOSIDED for i in range(scene._desc.bsdf_count))
    film, st = render(scene)
    ref = oracle_film(name, integrator)
    print("%s %s %s: values differing from the oracle's: %d of %d" % (name, integrator, wrapping, int(np.sum(bits(film) != bits(ref))), film.size))
    assert st["textured"] == 1
    if integrator == ("path" if name == "c1" else "volpath"):                # the scene's own integrator
        assert st["kernel_variant"] == CONSTANT_SCENES[name][1]           # the row the unwrapped scene gets on the general unit
    assert np.array_equal(bits(film), bits(ref))


# ================================================================ 7. closed form
RHO_0, RHO_1, RHO_2 = np.array([0.15, 0.55, 0.35]), np.array([0.85, 0.25, 0.6]), np.array([0.3, 0.7, 0.1])
BLEND_W = 0.3
BACK_TEXTURE = "b44rgb_bilinear_clamp"
# (rays, sun): the side of the surface's own (unflipped) normal they are on; "flip": the sphere with flip_normals, whose outside is
# its back -- a closed surface's inside is in its own shadow, so its back side is lit only that way
SHEET_SIDES = [("front", "front"), ("back", "back"), ("front", "back"), ("back", "front")]


def sheet_case(surface, rays="front", sun="front", back="diffuse", flip=False, integrator="path", medium=False):
    """test_gpu_textures.closed_form_case with a twosided on the surface -> dictionary, expected rho (n, 3), |cos(theta)| of the sun"""
    gt.RNG = np.random.default_rng(2024)                                  # as closed_form_case: the same rays whichever cases run
    shape, p, uv, normal, seam = gt.SURFACES[surface](400)
    back_bsdf = {"diffuse": {"type": "diffuse", "reflectance": RHO_1.tolist()},
                 "textured": {"type": "diffuse", "reflectance": copy.copy(gt.TEXTURES[BACK_TEXTURE])},
                 "blend": {"type": "blendbsdf", "weight": BLEND_W, "x": {"type": "diffuse", "reflectance": RHO_1.tolist()},
                           "y": {"type": "diffuse", "reflectance": RHO_2.tolist()}}}[back]
    if back == "textured":
        rho_back, edge = gt.texture_eval(gt.TEXTURES[BACK_TEXTURE], uv)
    else:
        rho_back = np.tile(RHO_1 if back == "diffuse" else (1.0 - BLEND_W) * RHO_1 + BLEND_W * RHO_2, (len(uv), 1))
        edge = np.full(len(uv), np.inf)
    ray_sign, sun_sign = (1.0 if rays == "front" else -1.0), (1.0 if sun == "front" else -1.0)
    sun_dir = SUN * sun_sign                                               # -SUN: the same light from the other side of the sheet
    cos_sun = (normal * sun_sign) @ -sun_dir
    keep = np.flatnonzero((edge >= MARGIN) & (seam >= 0.02) & (cos_sun > 0.2))[:N_RAYS]
    assert len(keep) == N_RAYS, "not enough rays away from the discontinuities"
    p, normal, rho_back, cos_sun = p[keep], normal[keep], rho_back[keep], cos_sun[keep]
    towards = normal * ray_sign
    tilt = towards + 0.3 * np.cross(towards, [0.3, 0.5, 0.8])
    tilt /= np.linalg.norm(tilt, axis=1)[:, None]
    origins, directions = p + 1.5 * tilt, -tilt
    assert np.abs(np.r_[origins.ravel(), p.ravel()]).max() <= 4.0            # ATOL is derived for coordinates <= 4
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    bsdf = {"type": "twosided", "brdf_a": {"type": "diffuse", "reflectance": RHO_0.tolist()}, "brdf_b": back_bsdf}
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": 2},
         "sensor": {"type": "mradiancemeter", "origins": fmt(origins), "directions": fmt(directions),
                    "film": {"type": "hdrfilm", "width": N_RAYS, "height": 1, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}},
         "surface": dict(shape, bsdf=bsdf, **({"flip_normals": True} if flip else {})),
         "sun": {"type": "directional", "direction": sun_dir.tolist(), "irradiance": IRRADIANCE}}
    if medium:
        # a medium thin enough to change nothing (optical depth < 1e-7 across the scene) puts `volpath` on its ring row
        xf = T.translate([-8, -8, -8]) @ T.scale(16.0)
        grid = lambda v: {"type": "gridvolume", "data": np.full((2, 2, 2), v, np.float32), "to_world": xf}
        d["air"] = {"type": "cube", "to_world": T.scale(8.0), "bsdf": {"type": "null"},
                    "interior": {"type": "heterogeneous", "sigma_t": grid(1e-9), "albedo": grid(0.5), "phase": {"type": "isotropic"}}}
    if rays != sun:
        rho = np.zeros((N_RAYS, 3))
    else:
        front_side = (ray_sign > 0) != flip                                # the side of incidence against the shading normal
        rho = np.tile(RHO_0, (N_RAYS, 1)) if front_side else rho_back
    return d, rho, cos_sun


CLOSED_FORM = [(s, r, u, "diffuse", False) for s in ("rectangle", "disk", "quad_uv") for r, u in SHEET_SIDES] \
    + [("sphere", "front", "front", "diffuse", False), ("sphere", "front", "front", "diffuse", True), ("sphere", "back", "front", "diffuse", False)] \
    + [(s, "back", "back", b, False) for s in ("rectangle", "disk", "quad_uv") for b in ("textured", "blend")] \
    + [("sphere", "front", "front", b, True) for b in ("textured", "blend")]


def test_the_cases_reach_both_children():
    """(no device needed, but it belongs to the cases below)"""
    seen = set()
    for case in CLOSED_FORM:
        d, rho, cos_sun = sheet_case(*case)
        seen.add("front" if np.all(rho == RHO_0) else "dark" if not rho.any() else "back")
    assert seen == {"front", "back", "dark"}


# The bound: test_gpu_textures.ATOL (1e-4: the texture lookup's error for these shapes and texel counts).  The adapter adds no
# rounding -- its flips are negations -- and a blend child two roundings of values <= 1, which that bound's factor of five covers.
@pytest.mark.parametrize("surface,rays,sun,back,flip", CLOSED_FORM)
def test_closed_form(gpu_rgb, surface, rays, sun, back, flip):
    d, rho, cos_sun = sheet_case(surface, rays, sun, back, flip)
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s rays %s sun %s, %s%s: max |rho - expected| = %.3g" % (surface, rays, sun, back, " flipped" if flip else "", np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == 1                 # `path`: the flat row, in its TEX loop
    assert np.abs(got - rho).max() <= ATOL


@pytest.mark.parametrize("rays,sun,back", [("front", "front", "diffuse"), ("back", "back", "diffuse"), ("front", "back", "diffuse"), ("back", "back", "textured"), ("back", "back", "blend")])
@pytest.mark.parametrize("how,row", [("nested", 0), ("volpath", 0), ("volpathmis", 0), ("ring", 11024)])
def test_closed_form_other_rows(gpu_rgb, monkeypatch, how, row, rays, sun, back):
    """the rectangle through the nested TEX kernel (`path` under MTSAMD_KERNEL=nested, the volumetric integrators without a medium)
    and through the ring TEX kernel (`volpath` with the sheet inside a medium of no effect)"""
    d, rho, cos_sun = sheet_case("rectangle", rays, sun, back, integrator="path" if how == "nested" else "volpath" if how == "ring" else how, medium=how == "ring")
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s rays %s sun %s, %s: max |rho - expected| = %.3g" % (how, rays, sun, back, np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == row
    assert np.abs(got - rho).max() <= ATOL


@pytest.mark.parametrize("back", ["diffuse", "textured", "blend"])
def test_closed_form_mono(gpu_rgb, back):
    """gpu_mono: colours are their luminance"""
    lum = np.array([0.212671, 0.715160, 0.072169])                          # core/spectrum.h:246-248
    d, rho, cos_sun = sheet_case("rectangle", "back", "back", back)
    gpu_rgb.set_variant("gpu_mono")
    try:
        film, st = render(gpu_rgb.load_dict(d))
    finally:
        gpu_rgb.set_variant("gpu_rgb")
    got = measured_rho(film, cos_sun, mono=True)
    print("mono %s: max |rho - expected| = %.3g" % (back, np.abs(got[:, 0] - rho @ lum).max()))
    assert st["textured"] == 1 and np.abs(got[:, 0] - rho @ lum).max() <= ATOL


@pytest.mark.parametrize("rays,back", [("back", "diffuse"), ("back", "textured"), ("front", "diffuse")])
def test_closed_form_through_the_sample_entry(gpu_rgb, rays, back):
    """SamplingIntegrator::sample (mts_sample) with caller-supplied rays onto the back (and the front) of the sheet"""
    d, rho, cos_sun = sheet_case("rectangle", rays, rays, back)
    scene = gpu_rgb.load_dict(d)
    o = np.array([float(x) for x in d["sensor"]["origins"].split(",")], np.float32).reshape(-1, 3)
    w = np.array([float(x) for x in d["sensor"]["directions"].split(",")], np.float32).reshape(-1, 3)
    n = len(o)
    rgb, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    cols = [np.ascontiguousarray(a) for a in (o[:, 0], o[:, 1], o[:, 2], w[:, 0], w[:, 1], w[:, 2])]
    A.check(A.lib().mts_sample(scene._handle, n, 0, *[c.ctypes.data_as(A.fp) for c in cols], rgb.ctypes.data_as(A.fp), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert valid.all()
    assert np.abs(rgb.astype(np.float64) * np.pi / (IRRADIANCE * cos_sun[:, None]) - rho).max() <= ATOL


# ================================================================ 8. mirror symmetry
def mirror_case(child, below):
    """a rectangle in z = 0 under a one-child twosided; rays and sun from above, or (`below`) all of them mirrored in z"""
    rng = np.random.default_rng(808)
    p = np.c_[rng.uniform(-1.8, 1.8, N_RAYS), rng.uniform(-1.3, 1.3, N_RAYS), np.zeros(N_RAYS)]
    w = np.c_[rng.uniform(-0.5, 0.5, (N_RAYS, 2)), -np.ones(N_RAYS)]
    w /= np.linalg.norm(w, axis=1)[:, None]
    o, w, sun = (p - 1.5 * w).astype(np.float32), w.astype(np.float32), SUN.astype(np.float32)
    if below:
        o[:, 2], w[:, 2], sun[2] = -o[:, 2], -w[:, 2], -sun[2]
    tex = {"type": "bitmap", "data": np.random.default_rng(9).random((4, 4, 3), dtype=np.float32), "to_uv": T.scale([3.0, 2.0, 1.0])}
    x = {"diffuse": {"type": "diffuse", "reflectance": tex}, "rpv": {"type": "rpv", "rho_0": tex, "k": 0.6, "g": -0.2}}[child]
    fmt = lambda a: ", ".join("%.9g" % v for v in a.ravel())
    return {"type": "scene", "integrator": {"type": "path", "max_depth": 3},
            "sensor": {"type": "mradiancemeter", "origins": fmt(o), "directions": fmt(w),
                       "film": {"type": "hdrfilm", "width": N_RAYS, "height": 1, "rfilter": {"type": "box"}},
                       "sampler": {"type": "independent", "sample_count": 4}},
            "sheet": {"type": "rectangle", "to_world": T.scale([2.0, 1.5, 1.0]), "bsdf": {"type": "twosided", "x": x}},
            "sun": {"type": "directional", "direction": [float(v) for v in sun], "irradiance": IRRADIANCE}}


@pytest.mark.parametrize("child", ["diffuse", "rpv"])
def test_mirror_symmetry(gpu_rgb, child):
    """The adapter's flip is an exact negation and the streams are per film column: the render from below equals the render from
    above bit for bit.  Nothing else pins the back side of rpv."""
    above, sa = render(gpu_rgb.load_dict(mirror_case(child, False)))
    below, sb = render(gpu_rgb.load_dict(mirror_case(child, True)))
    differing = int(np.sum(bits(above) != bits(below)))
    scale = float(np.abs(above[..., :3]).mean())
    print("%s: values differing between above and below: %d of %d; max |difference| / film mean = %.3g"
          % (child, differing, above.size, np.abs(above.astype(np.float64) - below).max() / scale))
    assert sa["textured"] == sb["textured"] == 1 and np.all(above[..., 1] > 0)          # every ray sees the lit sheet
    assert np.array_equal(bits(above), bits(below))


# ================================================================ 9. the formulations agree
def sheet_in_c3(width, height, exchanged=False):
    """c3 with a horizontal sheet half-way up the slab and smaller than it: the camera and the sun meet it from above, light
    scattered in the medium and reflected by the ground from below"""
    d = scenes.c3_heterogeneous(width, height, 8, res=8)
    front = {"type": "diffuse", "reflectance": copy.deepcopy(gt.varying_c3(width, height)["ground"]["bsdf"]["reflectance"])}      # its 4 x 4 rgb bitmap
    back = {"type": "rpv", "rho_0": [0.1, 0.3, 0.05], "k": 0.6, "g": -0.2}
    if exchanged:
        front, back = back, front
    d["sheet"] = {"type": "rectangle", "to_world": T.translate([0, 0, 1.0]) @ T.scale(6.0), "bsdf": {"type": "twosided", "a": front, "b": back}}
    return d


@pytest.mark.parametrize("width,height", [(16, 16), (13, 11)])
def test_rows_agree(gpu_rgb, monkeypatch, width, height):
    """the ring kernel resolves the child per lane before its wave-uniform record loads: a wrong uniform load shows here as a
    disagreement with the per-lane kernels, not as a plausible picture"""
    d = sheet_in_c3(width, height)
    film, st = render(gpu_rgb.load_dict(d))
    assert st["textured"] == 1 and st["kernel_variant"] == 11024             # the ring row ran, in its TEX kernel
    assert film[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
        other, so = render(gpu_rgb.load_dict(d))
        assert so["textured"] == 1 and so["kernel_variant"] == row
        assert np.array_equal(bits(film), bits(other)), kernel
    monkeypatch.delenv("MTSAMD_KERNEL")
    turned, stt = render(gpu_rgb.load_dict(sheet_in_c3(width, height, exchanged=True)))
    assert stt["kernel_variant"] == 11024 and not np.array_equal(bits(film), bits(turned))      # both sides were hit


def test_wavefront_streams_and_counters(gpu_rgb, monkeypatch):
    d = sheet_in_c3(16, 16)
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


# ================================================================ 10. full transport against the independent float64 estimator
@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0)])
def test_panel_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    """`path` in the flat TEX loop, `volpath` in the nested TEX kernel; test_independent_surface_pin's own acceptance"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = problems_twosided.box_panel()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 1)}, seen
    assert_agrees(mean, var, gm, gv, "hip box with a two-sided panel %s" % integrator)


def test_pin_rejects_exchanged_children(gpu_rgb, monkeypatch):
    """the mutation this pin must reject: brdf_0 and brdf_1 of the panel exchanged"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), problems_twosided.box_panel(exchanged=True)[0], 16, 1024)
    assert rejected(mean, var, gm, gv, "hip box with a two-sided panel, children exchanged")


# ================================================================ 11. update in place is a fresh load
def test_update_in_place(gpu_rgb):
    a = sheet_in_c3(16, 16)                                                  # front: a bitmap, back: rpv
    a["sheet"]["bsdf"]["b"] = {"type": "diffuse", "reflectance": [0.7, 0.6, 0.2]}
    texels = np.random.default_rng(21).random((4, 4, 3), dtype=np.float32)
    a["shelf"] = {"type": "rectangle", "to_world": T.translate([3, -2, 1.5]) @ T.scale(4.0),
                  "bsdf": {"type": "twosided", "a": {"type": "rpv", "rho_0": 0.2, "k": 0.7, "g": 0.1},
                           "b": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": texels, "to_uv": T.scale([3.0, 2.0, 1.0])}}}}
    scene = gpu_rgb.load_dict(a)
    first = assert_is_fresh(gpu_rgb, scene, a)
    params = gpu_rgb.traverse(scene)
    new = np.random.default_rng(22).random((4, 4, 3), dtype=np.float32)
    b = copy.deepcopy(a)
    b["sheet"]["bsdf"]["b"]["reflectance"] = [0.2, 0.3, 0.8]
    b["shelf"]["bsdf"]["b"]["reflectance"]["data"] = new
    params["sheet.bsdf.brdf_1.reflectance.value"] = [0.2, 0.3, 0.8]
    params["shelf.bsdf.brdf_1.reflectance.data"] = new
    params.update()
    second = assert_is_fresh(gpu_rgb, scene, b)
    assert not np.array_equal(bits(first), bits(second))                    # the back sides are seen
    params["sheet.bsdf.brdf_1.reflectance.value"] = [0.7, 0.6, 0.2]
    params["shelf.bsdf.brdf_1.reflectance.data"] = texels
    params.update()
    assert np.array_equal(bits(assert_is_fresh(gpu_rgb, scene, a)), bits(first))
