"""Full transport through Fresnel interfaces on the device (run with -m gpu on an MI355X) against the independent float64 estimator
(tests/independent/specular.py; problem tests/independent/problems_specular.py: the lit box with a glass sphere, a tilted coloured
conductor plate and a `twosided(conductor)` panel; fixture tests/golden/indep_pin_surf_specular_16x16.npz from make_pin_specular.py),
under `path`, `volpath` and `volpathmis` in the TEX kernels: 16 seeds x 1 024 spp on the 16 x 16 film, the acceptance of
tests/test_independent_surface_pin.assert_agrees (every pixel inside the Sidak-corrected Z-test at significance 0.01, the image mean
within the combined standard error).  tests/test_specular_pin.py shows on the CPU that the problem is well posed."""
import os

import numpy as np
import pytest

import tests.kernel_rows as kr
from tests.independent import problems_specular
from tests.test_independent_pin import GOLDEN
from tests.test_independent_surface_pin import assert_agrees, rejected, rgb_estimate
from tests.test_independent_textured_pin import hip_render

pytestmark = pytest.mark.gpu


def load_pin():
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_specular_16x16.npz"))
    return z["mean"], z["var"]


# `path`: the flat row in its TEX loop; `volpath` / `volpathmis` on a scene without a medium: the nested TEX kernel
@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0), ("volpathmis", 0)])
def test_specular_box_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = problems_specular.box_specular()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 1)}, seen
    assert_agrees(mean, var, gm, gv, "hip specular box %s" % integrator)


@pytest.mark.parametrize("mutation", ["eta_inverted", "k_zero"])
def test_pin_rejects_a_wrong_interface(gpu_rgb, monkeypatch, mutation):
    """the mutated scenes this pin must reject: the ball's indices exchanged, the plate's k = 0"""
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), problems_specular.box_specular(mutation=mutation)[0], 16, 1024)
    assert rejected(mean, var, gm, gv, "hip specular box, %s" % mutation)
