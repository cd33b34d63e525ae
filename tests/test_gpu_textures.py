"""`bitmap` / `checkerboard` textures on the device (run with -m gpu on an MI355X).

What pins them: (1) a closed form -- one textured diffuse surface under a directional emitter, `path` with max_depth = 2, so that every
sample is rho(uv) E cos(theta) / pi with uv and rho restated here in float64 from the reference's formulas; (2) constant texels: the
film is the oracle's film of the untextured dictionary, bit for bit; (3) the kernels the table's rows map to agree bit for bit;
(5) an update in place is a fresh load.  Nothing compares a spatially varying render with the oracle: it knows no textures."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.oracle_binding as ob
import tests.transport_cases as tc

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f


def render(scene):
    sensor = scene.sensors()[0]
    assert scene.integrator().render(scene, sensor)
    return np.array(sensor.film().bitmap(raw=True)), dict(scene.integrator().last_stats)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def digest(scene):
    out = (C.c_uint64 * 8)()
    A.check(A.lib().mts_debug_scene_digest(scene._handle, out))
    return list(out)


# ================================================================ 1. uv and lookup against a float64 restatement
# ---- the reference's formulas, float64
def to_uv3(t):
    """Transform4f::extract (transform.h:327-348) of a 4x4, as transform_affine uses it (:91-98): 2x2 and the translation's x, y"""
    m = np.asarray(t.matrix, np.float64).reshape(4, 4)
    return np.array([[m[0, 0], m[0, 1], m[0, 3]], [m[1, 0], m[1, 1], m[1, 3]]])


def wrap(mode, v, res):
    """bitmap.cpp:386-401"""
    v = np.asarray(v, np.int64)
    if mode == "clamp":
        return np.clip(v, 0, res - 1)
    div = np.trunc(v / res).astype(np.int64)                      # the divisor<int> of enoki: C division, toward zero
    mod = v - div * res
    mod = np.where(mod < 0, mod + res, mod)
    if mode == "mirror":
        mod = np.where(((div & 1) == 0) ^ (v < 0), mod, res - 1 - mod)
    return mod


def bitmap_eval(tex, uv):
    """bitmap.cpp:403-474 -> (n, 3) values and the distance, in texels, to the nearest discontinuity of the lookup"""
    data = np.asarray(tex["data"], np.float64)
    if data.ndim == 2:
        data = data[..., None]
    if data.shape[2] == 1:
        data = np.repeat(data, 3, axis=2)
    h, w = data.shape[:2]
    m = to_uv3(tex.get("to_uv", T()))
    st = uv @ m[:, :2].T + m[:, 2]
    res = np.array([w, h], np.float64)
    mode = tex.get("wrap_mode", "repeat")
    if tex.get("filter_type", "bilinear") == "nearest":
        p = st * res
        i = np.floor(p).astype(np.int64)
        edge = np.min(np.minimum(p - i, 1.0 - (p - i)), axis=1)
        return data[wrap(mode, i[:, 1], h), wrap(mode, i[:, 0], w)], edge
    p = st * res - 0.5
    i = np.floor(p).astype(np.int64)
    w1 = p - i
    w0 = 1.0 - w1
    x0, x1, y0, y1 = wrap(mode, i[:, 0], w), wrap(mode, i[:, 0] + 1, w), wrap(mode, i[:, 1], h), wrap(mode, i[:, 1] + 1, h)
    v0 = w0[:, :1] * data[y0, x0] + w1[:, :1] * data[y0, x1]
    v1 = w0[:, :1] * data[y1, x0] + w1[:, :1] * data[y1, x1]
    return w0[:, 1:] * v0 + w1[:, 1:] * v1, np.full(len(uv), np.inf)            # bilinear interpolation is continuous


def checker_eval(tex, uv):
    """checkerboard.cpp:46-65"""
    m = to_uv3(tex.get("to_uv", T()))
    st = uv @ m[:, :2].T + m[:, 2]
    f = st - np.floor(st)
    mask = f > 0.5
    c0, c1 = (np.broadcast_to(np.asarray(tex.get(k, d), np.float64), (3,)) for k, d in (("color0", 0.4), ("color1", 0.2)))
    # the pattern's cells are half a unit wide: the distance to an edge in cells
    edge = np.min(np.minimum(np.minimum(f, np.abs(f - 0.5)), 1.0 - f), axis=1) * 2.0
    return np.where((mask[:, 0] == mask[:, 1])[:, None], c0, c1), edge


def texture_eval(tex, uv):
    return checker_eval(tex, uv) if tex["type"] == "checkerboard" else bitmap_eval(tex, uv)


# ---- surfaces: each gives world points with their reference uv (float64) and the surface normal there
RNG = np.random.default_rng(2024)
RECT_XF = T.translate([0.5, -0.25, 0.75]) @ T.rotate([1, 0, 0], 25) @ T.scale([2.0, 1.5, 1.0])
SPHERE_XF = T.translate([0.25, 0.5, 1.0]) @ T.rotate([0, 1, 0], 30) @ T.rotate([0, 0, 1], 40) @ T.scale(1.25)
QUAD = np.array([[-1.5, -1, 0], [1.5, -1, 0.5], [1.5, 1, 0.5], [-1.5, 1, 0]], np.float32)
QUAD_UV = np.array([[0.1, 0.2], [0.9, 0.15], [0.95, 0.85], [0.05, 0.9]], np.float32)
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def mat(t):
    return np.asarray(t.matrix, np.float64).reshape(4, 4)


def rectangle(n, rng=None):
    s = (rng or RNG).random((n, 2))
    m = mat(RECT_XF)
    p = (np.c_[2 * s - 1, np.zeros(n), np.ones(n)] @ m.T)[:, :3]
    normal = m[:3, 2] / np.linalg.norm(m[:3, 2])
    return {"type": "rectangle", "to_world": RECT_XF}, p, s, np.tile(normal, (n, 1)), np.full(n, 1.0)          # rectangle.cpp:205: uv = prim_uv / 2 + 1 / 2


def disk(n, rng=None):
    rng = rng or RNG
    r, phi = 0.1 + 0.85 * rng.random(n), 2 * np.pi * rng.random(n)
    m = mat(RECT_XF)
    p = (np.c_[r * np.cos(phi), r * np.sin(phi), np.zeros(n), np.ones(n)] @ m.T)[:, :3]
    normal = m[:3, 2] / np.linalg.norm(m[:3, 2])
    uv = np.c_[r, phi / (2 * np.pi)]                                   # disk.cpp:206-211
    seam = np.minimum(uv[:, 1], 1 - uv[:, 1])
    return {"type": "disk", "to_world": RECT_XF}, p, uv, np.tile(normal, (n, 1)), seam


def sphere(n, rng=None):
    rng = rng or RNG
    theta, phi = np.pi * (0.08 + 0.84 * rng.random(n)), 2 * np.pi * rng.random(n)
    local = np.c_[np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)]
    m = mat(SPHERE_XF)
    p = (np.c_[local, np.ones(n)] @ m.T)[:, :3]
    normal = local @ (m[:3, :3] / 1.25).T
    uv = np.c_[phi / (2 * np.pi), theta / np.pi]                       # sphere.cpp:362-370
    seam = np.minimum(np.minimum(uv[:, 0], 1 - uv[:, 0]), np.minimum(uv[:, 1], 1 - uv[:, 1]))
    return {"type": "sphere", "to_world": SPHERE_XF}, p, uv, normal, seam


def quad(n, texcoords, rng=None):
    rng = rng or RNG
    face = rng.integers(0, 2, n)
    b = 0.05 + 0.9 * rng.random((n, 2))
    flip = b.sum(axis=1) > 1.0
    b[flip] = 1.0 - b[flip]
    b = np.clip(b, 0.03, None)                                         # strictly inside the triangle
    v = QUAD.astype(np.float64)[QUAD_FACES[face]]                      # (n, 3, 3)
    b0 = 1.0 - b[:, 0] - b[:, 1]
    p = v[:, 0] * b0[:, None] + v[:, 1] * b[:, :1] + v[:, 2] * b[:, 1:]
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    normal /= np.linalg.norm(normal, axis=1)[:, None]
    shape = {"type": "mesh", "vertex_positions": QUAD, "faces": QUAD_FACES}
    if texcoords:                                                      # mesh.cpp:490-497
        shape["vertex_texcoords"] = QUAD_UV
        t = QUAD_UV.astype(np.float64)[QUAD_FACES[face]]
        uv = t[:, 0] * b0[:, None] + t[:, 1] * b[:, :1] + t[:, 2] * b[:, 1:]
    else:
        uv = b.copy()
    return shape, p, uv, normal, np.minimum(np.minimum(b[:, 0], b[:, 1]), b0)      # the margin: away from the triangle's edges


SURFACES = {"rectangle": rectangle, "disk": disk, "sphere": sphere, "quad_uv": lambda n, rng=None: quad(n, True, rng), "quad_bary": lambda n, rng=None: quad(n, False, rng)}
B44 = np.random.default_rng(44).random((4, 4), dtype=np.float32)
B53 = np.random.default_rng(53).random((3, 5, 3), dtype=np.float32)                  # 5 x 3 texels, rgb
B44C = np.random.default_rng(45).random((4, 4, 3), dtype=np.float32)
B53G = np.random.default_rng(54).random((3, 5), dtype=np.float32)
UV23 = T.scale([2.0, 3.0, 1.0])
CHECKER = {"type": "checkerboard", "color0": [0.7, 0.5, 0.3], "color1": 0.15, "to_uv": T.scale([4.0, 4.0, 1.0])}
TEXTURES = {
    "b44_bilinear_repeat": {"type": "bitmap", "data": B44, "to_uv": UV23},
    "b44_nearest_mirror": {"type": "bitmap", "data": B44, "filter_type": "nearest", "wrap_mode": "mirror", "to_uv": UV23},
    "b44rgb_bilinear_clamp": {"type": "bitmap", "data": B44C, "wrap_mode": "clamp", "to_uv": UV23},
    "b44rgb_nearest_repeat": {"type": "bitmap", "data": B44C, "filter_type": "nearest", "to_uv": UV23},
    "b53rgb_bilinear_mirror": {"type": "bitmap", "data": B53, "wrap_mode": "mirror", "to_uv": UV23},
    "b53rgb_nearest_clamp": {"type": "bitmap", "data": B53, "filter_type": "nearest", "wrap_mode": "clamp", "to_uv": UV23},
    "b53_bilinear_repeat_offset": {"type": "bitmap", "data": B53G, "to_uv": T.translate([0.3, -0.2, 5.0]) @ UV23},
    "b53_nearest_repeat": {"type": "bitmap", "data": B53G, "filter_type": "nearest", "to_uv": UV23},
    "checker": CHECKER,
}
CASES = [("rectangle", t) for t in TEXTURES] + [(s, t) for s in ("disk", "sphere", "quad_uv", "quad_bary") for t in ("b53rgb_bilinear_mirror", "b44_nearest_mirror", "checker")]
N_RAYS, IRRADIANCE = 24, 3.0
SUN = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
MARGIN = 0.05                                                           # texels (cells of a checkerboard), and 0.05 / 2 pi .. of the seams


def closed_form_case(surface, texture, integrator="path"):
    """-> dictionary, expected rho (n, 3), cos(theta) of the sun at every hit"""
    global RNG
    RNG = np.random.default_rng(2024)                                    # the same rays whichever cases run, in whatever order
    shape, p, uv, normal, seam = SURFACES[surface](400)
    tex = TEXTURES[texture]
    rho, edge = texture_eval(tex, uv)
    cos_sun = normal @ -SUN
    keep = np.flatnonzero((edge >= MARGIN) & (seam >= 0.02) & (cos_sun > 0.2))[:N_RAYS]
    assert len(keep) == N_RAYS, "not enough rays away from the discontinuities"
    p, uv, normal, rho, cos_sun = p[keep], uv[keep], normal[keep], rho[keep], cos_sun[keep]
    assert np.all(edge[keep] >= MARGIN) and np.all(seam[keep] >= 0.02)
    # every sub-sensor looks at its point from 1.5 units above it, a little off the normal
    tilt = normal + 0.3 * np.cross(normal, [0.3, 0.5, 0.8])
    tilt /= np.linalg.norm(tilt, axis=1)[:, None]
    origins, directions = p + 1.5 * tilt, -tilt
    assert np.abs(np.r_[origins.ravel(), p.ravel()]).max() <= 4.0            # the tolerance below is derived for coordinates <= 4
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": 2},
         "sensor": {"type": "mradiancemeter", "origins": fmt(origins), "directions": fmt(directions),
                    "film": {"type": "hdrfilm", "width": N_RAYS, "height": 1, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}},
         "surface": dict(shape, bsdf={"type": "diffuse", "reflectance": copy.copy(tex)}),
         "sun": {"type": "directional", "direction": SUN.tolist(), "irradiance": IRRADIANCE}}
    return d, rho, cos_sun


def measured_rho(film, cos_sun, mono=False):
    """every sample is rho E cos(theta) / pi: the film's mean radiance back to rho"""
    a = np.asarray(film, np.float64)[0]
    assert np.all(a[:, 4] == 4.0) and np.all(a[:, 3] == 4.0)                 # four valid samples per ray
    radiance = np.repeat((a[:, 1] / a[:, 4])[:, None], 3, axis=1) if mono else tc.radiance_rgb(film)[0]
    return radiance * np.pi / (IRRADIANCE * cos_sun[:, None])


# Tolerance: scene coordinates <= 4, so the fp32 hit point is good to ~1e-6, uv to ~1e-6, the texel coordinate to res * scale * 1e-6 <=
# 5 * 3 * 1e-6; the bilinear value of texels in [0, 1] then to <= 2e-5; x 5 for atan2f / asinf and the evaluation's own rounding.
ATOL = 1e-4


@pytest.mark.parametrize("surface,texture", CASES)
def test_closed_form(gpu_rgb, surface, texture):
    d, rho, cos_sun = closed_form_case(surface, texture)
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s / %s: max |rho - expected| = %.3g" % (surface, texture, np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == 1                 # `path`: the flat row, in its TEX loop
    assert np.abs(got - rho).max() <= ATOL


def test_closed_form_mono(gpu_rgb):
    d, rho, cos_sun = closed_form_case("rectangle", "b53rgb_bilinear_mirror")
    gpu_rgb.set_variant("gpu_mono")
    try:
        film, st = render(gpu_rgb.load_dict(d))
    finally:
        gpu_rgb.set_variant("gpu_rgb")
    lum = rho @ np.array([0.212671, 0.715160, 0.072169])
    got = measured_rho(film, cos_sun, mono=True)
    print("mono: max |rho - expected| = %.3g" % np.abs(got[:, 0] - lum).max())
    assert st["textured"] == 1 and np.abs(got[:, 0] - lum).max() <= ATOL


@pytest.mark.parametrize("how", ["nested", "volpath", "volpathmis"])
def test_closed_form_other_kernels(gpu_rgb, monkeypatch, how):
    """the rectangle case through the nested TEX kernel: `path` under MTSAMD_KERNEL=nested, and the volumetric integrators"""
    d, rho, cos_sun = closed_form_case("rectangle", "b53rgb_bilinear_mirror", integrator="path" if how == "nested" else how)
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    film, st = render(gpu_rgb.load_dict(d))
    got = measured_rho(film, cos_sun)
    print("%s: max |rho - expected| = %.3g" % (how, np.abs(got - rho).max()))
    assert st["textured"] == 1 and st["kernel_variant"] == 0                 # no medium: the nested row
    assert np.abs(got - rho).max() <= ATOL


def test_sample_entry_of_a_textured_scene(gpu_rgb):
    """SamplingIntegrator::sample (mts_sample) of a textured scene goes through the textures as the render does"""
    d, rho, cos_sun = closed_form_case("rectangle", "checker")
    scene = gpu_rgb.load_dict(d)
    o = np.array([float(x) for x in d["sensor"]["origins"].split(",")], np.float32).reshape(-1, 3)
    w = np.array([float(x) for x in d["sensor"]["directions"].split(",")], np.float32).reshape(-1, 3)
    n = len(o)
    rgb, valid = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    cols = [np.ascontiguousarray(a) for a in (o[:, 0], o[:, 1], o[:, 2], w[:, 0], w[:, 1], w[:, 2])]
    A.check(A.lib().mts_sample(scene._handle, n, 0, *[c.ctypes.data_as(A.fp) for c in cols], rgb.ctypes.data_as(A.fp), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert valid.all()
    assert np.abs(rgb.astype(np.float64) * np.pi / (IRRADIANCE * cos_sun[:, None]) - rho).max() <= ATOL


# ================================================================ 2. constant texels: the oracle's film of the untextured dictionary
def constant_bitmap(value, filter_type):
    v = np.asarray(value, np.float32).reshape(-1)
    data = np.empty((2, 2, v.size), np.float32)
    data[...] = v
    return {"type": "bitmap", "data": data[..., 0] if v.size == 1 else data, "filter_type": filter_type, "to_uv": T.scale([3.0, 5.0, 1.0])}


def textured_copy(d, filter_type, value=None):
    """every diffuse / rpv parameter of the dictionary's shapes replaced by a 2 x 2 bitmap of its value (or of `value`); -> (textured, plain)"""
    tex, plain = copy.deepcopy(d), copy.deepcopy(d)
    for key, shape in d.items():
        bsdf = shape.get("bsdf") if isinstance(shape, dict) else None
        if not bsdf or bsdf["type"] == "null":
            continue
        for name in ("reflectance", "rho_0", "k", "g", "rho_c"):
            if name in bsdf:
                v = bsdf[name]["value"] if isinstance(bsdf[name], dict) else bsdf[name]
                if value is not None:
                    v = value if name != "g" else -value
                    plain[key]["bsdf"][name] = v
                tex[key]["bsdf"][name] = constant_bitmap(v, filter_type)
    return tex, plain


CONSTANT_SCENES = {
    "c3": (lambda: scenes.c3_heterogeneous(16, 16, 8, res=8), 11024),
    "c4": (lambda: scenes.c4_atmosphere(16, 16, 8, layers=8), 11024),
    "c1": (lambda: scenes.c1_cornell(16, 16, 8), 1),
}


@pytest.mark.parametrize("name", sorted(CONSTANT_SCENES))
@pytest.mark.parametrize("filter_type,value", [("nearest", None), ("bilinear", 0.5), ("bilinear", 0.25)])
def test_constant_texels_equal_the_oracle(gpu_rgb, name, filter_type, value):
    """nearest: the texel itself.  bilinear: w0 v + w1 v rounds back to v for a power of two (checked: not for 0.3), so those values"""
    build, row = CONSTANT_SCENES[name]
    tex, plain = textured_copy(build(), filter_type, value)
    scene = gpu_rgb.load_dict(tex)
    assert scene._desc.texture_count >= (5 if name == "c1" else 1)           # the cornell box: a texture of its own per wall
    film, st = render(scene)
    ref = ob.OracleScene(plain).render()
    print("%s %s: values differing from the oracle's: %d of %d" % (name, filter_type, int(np.sum(bits(film) != bits(ref))), film.size))
    assert st["textured"] == 1 and st["kernel_variant"] == row               # the row the untextured scene gets on the general unit
    assert np.array_equal(bits(film), bits(ref))


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_constant_texels_volpathmis(gpu_rgb, name):
    tex, plain = textured_copy(CONSTANT_SCENES[name][0](), "nearest")
    for d in (tex, plain):
        d["integrator"]["type"] = "volpathmis"
    film, st = render(gpu_rgb.load_dict(tex))
    assert st["textured"] == 1 and st["kernel_variant"] == 10512             # the 512-path ring row; rendered by the nested TEX kernel
    assert np.array_equal(bits(film), bits(ob.OracleScene(plain).render()))


# ================================================================ 3. the formulations agree
def varying_c3(width, height, ground="diffuse"):
    d = scenes.c3_heterogeneous(width, height, 8, res=8)
    tex = {"type": "bitmap", "data": np.random.default_rng(9).random((4, 4, 3), dtype=np.float32), "to_uv": T.scale([7.0, 5.0, 1.0])}
    d["ground"]["bsdf"] = {"type": "diffuse", "reflectance": tex} if ground == "diffuse" else {"type": "rpv", "rho_0": tex, "k": 0.6, "g": -0.2}
    return d


@pytest.mark.parametrize("width,height,ground", [(16, 16, "diffuse"), (13, 11, "diffuse"), (16, 16, "rpv")])
def test_rows_agree_with_the_nested_kernel(gpu_rgb, monkeypatch, width, height, ground):
    """The film of the row a scene gets (ring 1024) equals the film under MTSAMD_KERNEL=nested and MTSAMD_KERNEL=flat bit for bit: same
    functions, same streams: the ring TEX kernel (`volpath` on 1024-path rings) against the nested TEX kernel, twice."""
    d = varying_c3(width, height, ground)
    film, st = render(gpu_rgb.load_dict(d))
    assert st["textured"] == 1 and st["kernel_variant"] == 11024
    assert film[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
        other, so = render(gpu_rgb.load_dict(d))
        assert so["textured"] == 1 and so["kernel_variant"] == row
        assert np.array_equal(bits(film), bits(other)), kernel


def test_wavefront_streams_and_counters(gpu_rgb):
    d = varying_c3(16, 16)
    d["sensor"]["sampler"]["wavefront"] = True
    scene = gpu_rgb.load_dict(d)
    film, st = render(scene)
    assert st["textured"] == 1 and np.isfinite(film).all() and film[..., :3].std() > 0
    sensor = scene.sensors()[0]
    assert scene.integrator().render(scene, sensor, collect_counters=True)
    assert scene.integrator().last_stats["n_iter"] > 0
    assert np.array_equal(bits(film), bits(np.array(sensor.film().bitmap(raw=True))))      # the counting instantiation: the same film


# ================================================================ 5. update in place
def assert_is_fresh(pkg, scene, d):
    film, st = render(scene)
    fresh = pkg.load_dict(d)
    fresh_film, fresh_st = render(fresh)
    assert digest(scene) == digest(fresh)
    assert st["kernel_variant"] == fresh_st["kernel_variant"] and st["textured"] == fresh_st["textured"] == 1
    assert np.array_equal(bits(film), bits(fresh_film))
    return film


def test_update_in_place(gpu_rgb):
    a = varying_c3(16, 16)
    a["slab"]["bsdf"] = {"type": "null"}
    a["wall"] = {"type": "rectangle", "to_world": T.translate([0, 0, 0.5]) @ T.scale(20.0),
                 "bsdf": {"type": "bilambertian", "reflectance": {"type": "checkerboard", "to_uv": T.scale([6.0, 6.0, 1.0])}, "transmittance": 0.3}}
    scene = gpu_rgb.load_dict(a)
    first = assert_is_fresh(gpu_rgb, scene, a)
    params = gpu_rgb.traverse(scene)
    new = np.random.default_rng(10).random((4, 4, 3), dtype=np.float32)
    b = copy.deepcopy(a)
    b["ground"]["bsdf"]["reflectance"]["data"] = new
    b["wall"]["bsdf"]["reflectance"].update(color0=[0.9, 0.2, 0.1], color1=0.05)
    params["ground.bsdf.reflectance.data"] = new
    params["wall.bsdf.reflectance.color0.value"] = [0.9, 0.2, 0.1]
    params["wall.bsdf.reflectance.color1.value"] = 0.05
    params.update()
    second = assert_is_fresh(gpu_rgb, scene, b)
    assert not np.array_equal(bits(first), bits(second))
    # a refused update leaves film and digest as they were
    before = digest(scene)
    params["ground.bsdf.reflectance.data"] = np.zeros((4, 5, 3), np.float32)
    with pytest.raises(RuntimeError, match="the topology of a scene is frozen"):
        params.update()
    params["ground.bsdf.reflectance.data"] = np.full((4, 4, 3), np.nan, np.float32)
    params["wall.bsdf.reflectance.color0.value"] = 0.5
    with pytest.raises(RuntimeError, match="NaN"):
        params.update()
    assert digest(scene) == before
    assert np.array_equal(bits(render(scene)[0]), bits(second))
    # and back
    params["ground.bsdf.reflectance.data"] = a["ground"]["bsdf"]["reflectance"]["data"]
    params["wall.bsdf.reflectance.color0.value"] = 0.4
    params["wall.bsdf.reflectance.color1.value"] = 0.2
    params.update()
    assert np.array_equal(bits(assert_is_fresh(gpu_rgb, scene, a)), bits(first))
