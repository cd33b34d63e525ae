"""`dielectric` and `conductor` on the device (run with -m gpu on an MI355X).

  a. the float64 pin -- SamplingIntegrator::sample on 4 099 caller-supplied rays per case against tests/specular_ref.restate, lane by
     lane: `path` for every case, `volpath` rgb and `volpath` in gpu_mono for a subset.  On every kept lane `valid` and the pattern of
     zeros agree exactly and the value agrees within DEVICE_FACTOR * E_SPEC (E_SPEC: measured on the CPU, tests/test_specular.py;
     nothing measured here enters the bound).
  b. the rows -- the same dictionaries through an mradiancemeter of 300 of the rays: the flat TEX / INST loop of `path` equals
     MTSAMD_KERNEL=nested bit for bit; with a medium of no effect the ring row of `volpath` (11024) equals nested and flat, and
     `volpathmis` is shown to map from its table row to the nested TEX kernel.  One case carries an area emitter on the specular sheet itself, one puts a
     diffuse plate before the mirror of `twosided(conductor, diffuse)`: there the draws after the mirror decide the film, so a
     formulation that drew no emitter sample on the mirror's side would leave the others.
  c. a furnace without variance -- a glass sphere and a perfect mirror under a white sky: every sample is a product of eta_ti^2 and
     eta_it^2 factors, hence 1, or 0 if cut at max_depth.
  d. a medium behind an interface -- an absorbing slab of glass against the closed form of the incoherent sum over its internal
     reflections.
  e. index-matched -- that slab at eta = 1 with a scattering medium against the same scene with a `null` boundary: the same physics
     by two estimators (shadow rays are blocked by the one and pass the other).

Every figure printed here is measured on the device."""
import copy
import importlib

import numpy as np
import pytest

import tests.bsdf_tree_ref as R
import tests.kernel_rows as kr
import tests.specular_ref as S
from tests.test_gpu_textures import bits, render
from tests.test_independent_surface_pin import assert_agrees, rgb_estimate
from tests.test_independent_textured_pin import hip_render

pytestmark = pytest.mark.gpu

T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f
TEXTURED = {None: 1, "backdrop": 1, "placed": 2, "mirrored": 2}             # mts_stats.textured: the TEX and the INST instantiations


def assert_pinned(pkg, name, surface, placement, integrator, mono=False):
    case = S.case_of(name, surface, placement)
    ref = S.restate(case, integrator=integrator, mono=mono)                 # decides the lanes before any device value is looked at
    kept = ref.kept
    assert 1.0 - kept.mean() <= S.MAX_DROP
    scene = pkg.load_dict(dict(case.scene, integrator=dict(case.scene["integrator"], type=integrator)))
    assert int(scene._desc.sensor.sampler_seed) == R.base_seed()
    rgb, valid = scene.integrator().sample(scene, case.origins, case.directions, seed_offset=S.SEED_OFFSET)
    err = S.scaled_error(rgb, ref.value)
    print("%s %s %s %s%s: kept %d of %d, max scaled error %.3g (bound %.3g), max |difference| %.3g"
          % (name, surface, placement, integrator, " mono" if mono else "", kept.sum(), len(kept), err[kept].max(), S.device_bound(), np.abs(rgb - ref.value)[kept].max()))
    assert valid.all()
    assert np.array_equal(rgb[kept] == 0, ref.value[kept] == 0)
    assert not (err.max(axis=1) > S.device_bound())[kept].any()


# ================================================================ a. the float64 pin
@pytest.mark.parametrize("name,surface,placement", S.CASES)
def test_path_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    assert_pinned(gpu_rgb, name, surface, placement, "path")


@pytest.mark.parametrize("name,surface,placement", S.VOLPATH_CASES)
def test_volpath_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    assert_pinned(gpu_rgb, name, surface, placement, "volpath")


@pytest.mark.parametrize("name,surface,placement", S.MONO_CASES)
def test_volpath_mono_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    gpu_rgb.set_variant("gpu_mono")
    try:
        assert_pinned(gpu_rgb, name, surface, placement, "volpath", mono=True)
    finally:
        gpu_rgb.set_variant("gpu_rgb")


# ================================================================ b. the rows
def film_of(pkg, monkeypatch, d, kernel, row, textured):
    if kernel:
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
    else:
        monkeypatch.delenv("MTSAMD_KERNEL", raising=False)
    film, st = render(pkg.load_dict(d))
    assert st["textured"] == textured, (kernel, st["textured"], st["kernel_variant"])             # no silent fallback
    if row is not None:
        assert st["kernel_variant"] == row, (kernel, st["textured"], st["kernel_variant"])
    return film, st["kernel_variant"]


def lamp_on_the_sheet(scene):
    """place 2 of the ring machine's SURFACE block: a specular hit that is also an emitter's shape"""
    d = copy.deepcopy(scene)
    d["sheet"]["emitter"] = {"type": "area", "radiance": {"type": "rgb", "value": [0.4, 0.2, 0.7]}}
    return d


def plate_before_the_mirror(scene):
    """a grey plate, lit from both sides, 2 above the front of the canonical rectangle: what the mirror of twosided(conductor, diffuse)
    reflects arrives there, and the plate's emitter and BSDF samples are the next draws of the stream"""
    import tests.test_gpu_textures as gt
    d = copy.deepcopy(scene)
    d["plate"] = {"type": "rectangle", "to_world": gt.RECT_XF @ T.translate([0.0, 0.0, 2.0]) @ T.scale([3.0, 3.0, 1.0]),
                  "bsdf": {"type": "twosided", "material": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}}}
    d["integrator"] = dict(d["integrator"], max_depth=4)
    return d


ROW_CASES = [("dielectric_coloured", "rectangle", None, None), ("dielectric_checker", "quad_uv", "placed", None), ("dielectric_bubble", "disk", None, None),
             ("conductor_rgb", "rectangle", "mirrored", None), ("conductor_checker", "quad_uv", None, None), ("twosided_c", "rectangle", "placed", None),
             ("twosided_c_d", "disk", None, None), ("dielectric_glass", "rectangle", "backdrop", None),
             ("dielectric_coloured", "rectangle", None, lamp_on_the_sheet), ("conductor_rgb", "disk", None, lamp_on_the_sheet),
             ("twosided_c_d", "rectangle", None, plate_before_the_mirror)]


@pytest.mark.parametrize("name,surface,placement,change", ROW_CASES)
def test_rows_agree_with_the_nested_kernel(gpu_rgb, monkeypatch, name, surface, placement, change):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    scene = S.case_of(name, surface, placement).scene
    if change is not None:
        scene = change(scene)
    textured = TEXTURED[placement]
    flat, _ = film_of(gpu_rgb, monkeypatch, scene, None, 1, textured)                          # `path`: the flat row, in its TEX / INST loop
    nested, _ = film_of(gpu_rgb, monkeypatch, scene, "nested", 0, textured)
    assert np.all(flat[..., 4] == 4.0) and flat[..., :3].std() > 0
    assert np.array_equal(bits(flat), bits(nested))
    d = R.with_thin_medium(scene)
    ring, _ = film_of(gpu_rgb, monkeypatch, d, None, 11024, textured)                          # `volpath` in the medium: the ring row
    assert ring[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        assert np.array_equal(bits(ring), bits(film_of(gpu_rgb, monkeypatch, d, kernel, row, textured)[0])), kernel
    mis = dict(d, integrator=dict(d["integrator"], type="volpathmis"))
    # `volpathmis`: the table names its ring row, and kv::textured_variant sends a textured scene's `volpathmis` to the nested TEX /
    # INST kernel whatever the row.  What is checked is that mapping -- the row's name, `textured`, a film with content -- and that
    # asking for the nested kernel outright names row 0 and changes nothing; both runs execute the same kernel, so the equality of
    # the two films says no more than that.
    own, row = film_of(gpu_rgb, monkeypatch, mis, None, None, textured)
    assert row >= 10000 and own[..., :3].std() > 0, row
    assert np.array_equal(bits(own), bits(film_of(gpu_rgb, monkeypatch, mis, "nested", 0, textured)[0]))


# ================================================================ c. furnace without variance
MAX_DEPTH = 32


def cut_share(eta=1.5, max_depth=MAX_DEPTH, n=200001):
    """S: the share of the samples on the sphere that are still inside it at max_depth, in float64 -- a path enters with 1 - r and
    must be reflected at each of its max_depth - 2 inner hits, all at the angle of entry (a sphere), r the same by reciprocity; the
    mean over impact parameters b = sin(theta_i), uniform over the disk the sphere shows (weight 2 b db)"""
    b = (np.arange(n) + 0.5) / n
    r = S.fresnel_dielectric(np.sqrt(1.0 - b * b), eta)[0]
    return float(np.sum((1.0 - r) * r ** (max_depth - 2) * 2.0 * b) / n)


def furnace(integrator, size=16, spp=16):
    return {"type": "scene", "integrator": {"type": integrator, "max_depth": MAX_DEPTH, "rr_depth": 100},
            "sensor": {"type": "perspective", "fov": 40, "to_world": T.look_at([0, -6, 1.5], [0.6, 0, 0.2], [0, 0, 1]),
                       "film": {"type": "hdrfilm", "width": size, "height": size, "rfilter": {"type": "box"}},
                       "sampler": {"type": "independent", "sample_count": spp}},
            "ball": {"type": "sphere", "center": [0, 0, 0.3], "radius": 1.0, "bsdf": {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.0}},
            "mirror": {"type": "rectangle", "to_world": T.translate([1.9, 0.2, 0.3]) @ T.rotate([0, 1, 0], -70) @ T.scale([1.0, 1.2, 1.0]), "bsdf": {"type": "conductor"}},
            "sky": {"type": "constant", "radiance": 1.0}}


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_furnace_without_variance(gpu_rgb, monkeypatch, integrator):
    """every pixel <= 1 + 1e-5 (a few fp32 roundings of two squared factors and the film's division, times a margin of about twenty);
    the image mean >= 1 - S - 1e-5, S < 1e-4 the cut share (about 4e-6 at depth 32 for eta = 1.5)"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    s = cut_share()
    assert s < 1e-4
    seen = set()
    film = hip_render(gpu_rgb, seen)([furnace(integrator)])[0]
    assert {textured for _, textured in seen} == {1}, seen
    from tests.test_independent_surface_pin import XYZ_TO_RGB
    rgb = (film[..., :3] / film[..., 4:5]).astype(np.float64) @ XYZ_TO_RGB.T
    print("furnace %s: S = %.3g, image mean %.8f, brightest pixel 1 %+.3g, darkest pixel %.6f" % (integrator, s, rgb.mean(), rgb.max() - 1.0, rgb.min()))
    assert rgb.max() <= 1.0 + 1e-5
    assert rgb.mean() >= 1.0 - s - 1e-5


# ================================================================ d. a medium behind an interface
THETA = np.radians(40.0)


def slab(integrator, eta=1.5, albedo=0.0, boundary=None, sensor=None):
    """a wide slab of unit thickness and unit extinction (optical thickness 1 along the normal) under a white sky.  One scene for the
    closed form and for the index-matched comparison, so one roulette setting: rr_depth = 100, none.  With albedo 0.8 the depth is
    unlimited instead of 64: an index-matched dielectric counts its two crossings as depth and a null boundary does not, so a cut
    would fall on different paths of the two scenes.
    Roulette must stay out of a comparison that has `volpathmis` behind a null boundary on one side: volpathmis.cpp:136-140 divides
    p_over_f by the survival probability q and leaves p_over_f_nee as it is, so the two weights of an emitter reached through a null
    crossing after a roulette step no longer sum to one.  The CPU oracle, which restates those lines, on this slab at 40 degrees
    (512 seeds x 4 096 spp): `volpathmis` 0.71210 +- 0.00020 at rr_depth = 5 against 0.71465 +- 0.00019 at rr_depth = 100, `volpath`
    0.71535 +- 0.00038 and 0.71486 +- 0.00038.  That is a property of the reference's estimator, restated bit for bit by the kernels;
    behind a dielectric boundary no emitter sample passes, nothing is weighted, and the roulette is unbiased."""
    medium = {"type": "homogeneous", "sigma_t": 1.0, "albedo": albedo, "phase": {"type": "isotropic"}}
    return {"type": "scene", "integrator": {"type": integrator, "max_depth": 64 if albedo == 0.0 else -1, "rr_depth": 100},
            "sensor": sensor or {"type": "distant", "direction": [float(np.sin(THETA)), 0.0, float(-np.cos(THETA))], "ray_target": [0.0, 0.0, 0.0],
                                 "film": {"type": "hdrfilm", "width": 1, "height": 1, "rfilter": {"type": "box"}},
                                 "sampler": {"type": "independent", "sample_count": 1024}},
            "slab": {"type": "cube", "to_world": T.scale([60.0, 60.0, 0.5]), "interior": medium,
                     "bsdf": boundary or {"type": "dielectric", "int_ior": float(eta), "ext_ior": 1.0}},
            "sky": {"type": "constant", "radiance": 1.0}}


def slab_closed_form(eta=1.5, tau=1.0, theta=THETA):
    """R + T of the incoherent sum over the internal reflections: R = r + (1 - r)^2 r a^2 / (1 - r^2 a^2), T = (1 - r)^2 a / (1 - r^2 a^2),
    a = exp(-tau / cos(theta_t)).  The eta^2 factors of radiance cancel between entry and exit."""
    r, cos_t, _, _ = S.fresnel_dielectric(np.array([np.cos(theta)]), eta)
    r, a = float(r[0]), float(np.exp(-tau / cos_t[0]))
    return r + (1 - r) ** 2 * r * a * a / (1 - r * r * a * a) + (1 - r) ** 2 * a / (1 - r * r * a * a)


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
def test_medium_behind_an_interface(gpu_rgb, monkeypatch, integrator):
    """16 seeds x 1 024 spp: |mean - closed form| <= 4 standard errors of the 16 seed means.  A medium taken on reflection, or not left
    on exit, moves the value by tens of percent"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    expected = slab_closed_form()
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), slab(integrator), 16, 1024)
    assert {textured for _, textured in seen} == {1}, seen
    for c, ch in enumerate("rgb"):
        mean, se = float(gm[..., c].mean()), float(np.sqrt(gv[..., c].sum()) / gv[..., c].size)
        print("slab %s channel %s: mean %.5f +- %.5f, closed form %.5f" % (integrator, ch, mean, se, expected))
        assert 0 < se < 0.01
        assert abs(mean - expected) <= 4 * se


# ================================================================ e. index-matched
def slab_camera():
    return {"type": "perspective", "fov": 35, "to_world": T.look_at([4.0, -9.0, 5.0], [0, 0, 0], [0, 0, 1]),
            "film": {"type": "hdrfilm", "width": 8, "height": 8, "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": 1024}}


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
def test_index_matched_boundary_equals_a_null_boundary(gpu_rgb, monkeypatch, integrator):
    """16 seeds x 1 024 spp on the 8 x 8 film, per-pixel Z-test and image mean as tests/test_independent_surface_pin.assert_agrees.
    Measured on an MI355X: `volpath` 0.655252 against the null boundary's 0.653672, +0.24 % +- 0.10 %; `volpathmis` 0.655043 against
    0.654379, +0.10 % +- 0.05 %; every pixel accepted under both.  (slab() says why the scene runs without Russian roulette.)"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), slab(integrator, eta=1.0, albedo=0.8, sensor=slab_camera()), 16, 1024)
    assert {textured for _, textured in seen} == {1}, seen
    seen = set()
    nm, nv = rgb_estimate(hip_render(gpu_rgb, seen), slab(integrator, albedo=0.8, boundary={"type": "null"}, sensor=slab_camera()), 16, 1024)
    assert {textured for _, textured in seen} == {0}, seen
    assert_agrees(nm, nv, gm, gv, "index-matched slab %s" % integrator)
