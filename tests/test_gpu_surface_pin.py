"""The HIP path itself (not via the oracle) against the fixtures of the independent surface estimator
(tests/independent/surface.py, tests/golden/indep_pin_surf_*.npz; tests/test_independent_surface_pin.py has the reasoning, the
statistics and the oracle side): 16 seeds x 1024 spp on the 16 x 16 film, per colour channel the image mean within 4 combined
standard errors (< 0.25 %) and 1 %, and the per-pixel Z-test with the Sidak correction."""
import numpy as np
import pytest

import tests.kernel_rows as kr
from tests.independent import problems_surface
from tests.test_independent_surface_pin import (assert_agrees, assert_grey_agrees, assert_point_direct, fixture_for, grey_to_uniform, load_surf_pin,
                                                 rgb_estimate, spectral_estimate)

pytestmark = pytest.mark.gpu

LEAN_P_FLAT, GENERAL_FLAT, GENERAL_NESTED = kr.stat(kr.FLAT, kr.P), kr.stat(kr.FLAT), kr.stat(kr.NESTED)      # mts_stats.kernel_variant


def hip_render(pkg, variants):
    def render(dicts):
        films = []
        for dd in dicts:
            scene = pkg.load_dict(dd)
            sensor = scene.sensors()[0]
            assert scene.integrator().render(scene, sensor)
            films.append(np.array(sensor.film().bitmap(raw=True)))
            variants.add(scene.integrator().last_stats["kernel_variant"])
        return films
    return render


# `path` in the default formulation: the lean unit p where the scene admits it (no sphere, no rpv), the general flat loop for `orbs`
@pytest.mark.parametrize("name,variant", [("box", LEAN_P_FLAT), ("box_d3", LEAN_P_FLAT), ("orbs", GENERAL_FLAT), ("canopy", LEAN_P_FLAT)])
def test_hip_path_agrees_with_the_independent_surface_estimator(gpu_rgb, monkeypatch, name, variant):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var, _ = load_surf_pin(name)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), getattr(problems_surface, name)()[0], 16, 1024)
    assert seen == {variant}, seen
    assert_agrees(mean, var, gm, gv, "hip %s path" % name)


# the cornell box once more under every other formulation that renders it
@pytest.mark.parametrize("integrator,env,variant", [("path", {"MTSAMD_KERNEL": "nested"}, GENERAL_NESTED), ("path", {"MTSAMD_LEAN": "0"}, GENERAL_FLAT),
                                                    ("volpath", {}, GENERAL_NESTED), ("volpathmis", {}, GENERAL_NESTED)])
def test_hip_box_under_the_other_formulations(gpu_rgb, monkeypatch, integrator, env, variant):
    """`nested`, the general flat loop, and `volpath` / `volpathmis`, which run per lane on a scene without a medium."""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mean, var, _ = load_surf_pin(fixture_for("box", integrator))
    d = problems_surface.box()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {variant}, seen
    assert_agrees(mean, var, gm, gv, "hip box %s %s" % (integrator, env))


def test_hip_point_emitter_against_the_quadrature(gpu_rgb, monkeypatch):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), problems_surface.point_direct()[0], 16, 1024)
    assert seen == {GENERAL_FLAT}, seen                                               # a sphere: the general flat loop
    assert_point_direct(gm, gv, "point_direct hip")


@pytest.fixture(scope="module")
def gpu_spectral(pkg):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    pkg.set_variant("gpu_spectral")
    yield pkg
    pkg.set_variant("gpu_rgb")


def test_hip_spectral_path_agrees_with_the_independent_surface_estimator(gpu_spectral, monkeypatch):
    """`orbs` with grey colours as uniform spectra in gpu_spectral: four wavelengths per sample, CIE weighting, the spectral `path`
    on spheres, a cube, rpv and two emitters; Y / W divided by the y-bar integral against the green channel of the grey twin's fixture."""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var, _ = load_surf_pin("orbs_grey")
    seen = set()
    gm, gv = spectral_estimate(hip_render(gpu_spectral, seen), grey_to_uniform(problems_surface.orbs_grey()[0]), 16, 1024)
    assert seen == {GENERAL_FLAT}, seen
    assert_grey_agrees(mean, var, gm, gv, "hip orbs spectral")
