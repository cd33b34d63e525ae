"""Full transport through cones on the device (run with -m gpu on an MI355X) against the independent float64 estimator
(tests/independent/surface.py with the `Cone` of tests/independent/problems_cone.py; fixture tests/golden/indep_pin_surf_conifers_16x16.npz
from tests/independent/make_pin_cone.py), under `path`, `volpath` and `volpathmis` in the INST kernels: 16 seeds x 1 024 spp on the 16 x 16
film, the acceptance of tests/test_gpu_surface_pin.py (every pixel inside the Sidak-corrected Z-test at significance 0.01, the image mean
within the combined standard error).  And a furnace: whatever a path does among white two-sided cones under a white sky, it returns 1."""
import os

import numpy as np
import pytest

import tests.kernel_rows as kr
from tests.independent import problems_cone, surface
from tests.test_independent_pin import GOLDEN
from tests.test_independent_surface_pin import assert_agrees, rejected, rgb_estimate
from tests.test_independent_textured_pin import hip_render

pytestmark = pytest.mark.gpu


def load_pin():
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_conifers_16x16.npz"))
    return z["mean"], z["var"]


# `path`: the flat row in its INST loop; `volpath` / `volpathmis` on a scene without a medium: the nested INST kernel
@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0), ("volpathmis", 0)])
def test_conifers_agree_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    """Three placements of a two-sided crown over a box trunk -- rotations and uneven scales: oblique elliptic cones in world space -- and
    one plain one-sided cone, against thirteen world-space primitives worked out by hand"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d, scene, cam, max_depth, vertices = problems_cone.conifers()
    assert np.all(mean > 0) and surface.remainder_bound(scene, vertices, problems_cone.MAX_ALBEDO) < 1e-4 * mean.mean()
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 2)}, seen
    assert_agrees(mean, var, gm, gv, "hip conifers %s" % integrator)


@pytest.mark.parametrize("mutation", ["upright", "order"])
def test_pin_rejects_a_wrong_cone(gpu_rgb, monkeypatch, mutation):
    """the mutations this pin must reject: the lone cone not turned, one placement with scale and rotation in the wrong order"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), problems_cone.conifers(mutation=mutation)[0], 16, 1024)
    assert rejected(mean, var, gm, gv, "hip conifers, %s" % mutation)


@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
def test_furnace(gpu_rgb, monkeypatch, integrator):
    """Sky L = 1, every surface `twosided` diffuse with rho = 1, a cone in a group (placed twice, once under an uneven scale) and a plain
    flipped cone, max_depth = -1: the image mean is 1 within 4 standard errors (from 16 seeds x 256 spp; Russian roulette is the only
    source of variance).  A wrong frame, side or pdf on the cone darkens it.  Measured: `path` 0.99928 +- 0.00022, `volpath` 0.99955 +-
    0.00022, `volpathmis` 0.99936 +- 0.00032.  With 48 seeds the mean under `path` is 1 - 8.1e-4 +- 1.3e-4 -- and 1 - 8.4e-4 +- 1.5e-4 with
    spheres in the cones' places, 1 + 2.4e-4 +- 1.1e-4 for the ground alone: the deficit of under a tenth of a percent is that of curved
    two-sided surfaces in the INST kernels as they were, not the cone's."""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), problems_cone.furnace(integrator=integrator), 16, 256)
    assert {textured for _, textured in seen} == {2}, seen
    for c, ch in enumerate("rgb"):
        mean, se = gm[..., c].mean(), np.sqrt(gv[..., c].sum()) / gv[..., c].size
        print("furnace %s channel %s: image mean %.6f, standard error %.2g, darkest pixel %.4f" % (integrator, ch, mean, se, gm[..., c].min()))
        assert se < 2.5e-3
        assert abs(mean - 1.0) <= 4 * se + 1e-6, (integrator, ch, mean, se)          # (1e-6: the fp32 film of a pixel that sees only sky)
