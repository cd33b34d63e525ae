"""Full transport through textures against the independent estimator: the cornell box with a `nearest` rgb bitmap on its floor and a
checkerboard on its right wall (tests/independent/problems_textured.py), which the float64 analog walk of
tests/independent/surface.py sees as tiles of constant material.  The acceptance is test_independent_surface_pin.py's own
(rgb_estimate, assert_agrees): 16 seeds x 1024 spp on the 16 x 16 film, per colour channel the image mean within 4 combined standard
errors (< 0.25 %) and 1 %, and the per-pixel Z-test with the Sidak correction.

The oracle knows no textures, so only the HIP path stands on the other side (under -m gpu); without a GPU the fixture is held
against a short live run of the estimator, as the surface fixtures are."""
import math
import os

import numpy as np
import pytest

from tests.independent import problems_textured, surface
from tests.test_independent_pin import GOLDEN, z_test
from tests.test_independent_surface_pin import assert_agrees, rejected, rgb_estimate


def load_pin():
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_textured_16x16.npz"))
    return z["mean"], z["var"]


def test_problem_is_well_posed():
    d, scene, cam, max_depth, vertices = problems_textured.box_textured()
    mean, var = load_pin()
    assert mean.shape == (16, 16, 3) and np.all(mean > 0)
    # what the walks cut after `vertices` vertices leave out is far below the pin's sensitivity
    assert surface.remainder_bound(scene, vertices) < 1e-4 * mean.mean()
    assert len(scene.prims) == 4 + 16 + 16
    # the texels and the cells differ enough for a misplaced tile to show: the floor's texels spread over more than 0.2 per channel
    assert np.all(problems_textured.FLOOR.reshape(-1, 3).std(0) > 0.1)


def test_fixture_comes_from_the_committed_estimator():
    """A short live run of the estimator agrees with its fixture (same code, other seed, 64 walks per pixel)."""
    mean, var = load_pin()
    _, scene, cam, max_depth, vertices = problems_textured.box_textured()
    m, v = surface.render(scene, cam, 64, 77, max_depth, vertices)
    for c in range(3):
        se = math.sqrt(v[..., c].sum() + var[..., c].sum()) / m[..., c].size
        assert abs(m[..., c].mean() - mean[..., c].mean()) < 4 * se
        tm, tv = m[..., c].reshape(4, 4, 4, 4).mean((1, 3)), v[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        fm, fv = mean[..., c].reshape(4, 4, 4, 4).mean((1, 3)), var[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        p, alpha, _ = z_test(tm, tv, fm, fv)
        assert (p > alpha).all()


def hip_render(pkg, stats):
    def render(dicts):
        films = []
        for dd in dicts:
            scene = pkg.load_dict(dd)
            sensor = scene.sensors()[0]
            assert scene.integrator().render(scene, sensor)
            films.append(np.array(sensor.film().bitmap(raw=True)))
            stats.add((scene.integrator().last_stats["kernel_variant"], scene.integrator().last_stats["textured"]))
        return films
    return render


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,row", [("path", 1), ("volpath", 0)])
def test_hip_agrees_with_the_independent_estimator(gpu_rgb, monkeypatch, integrator, row):
    """`path` in the flat TEX loop, `volpath` in the nested TEX kernel"""
    import tests.kernel_rows as kr
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = problems_textured.box_textured()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    seen = set()
    gm, gv = rgb_estimate(hip_render(gpu_rgb, seen), d, 16, 1024)
    assert seen == {(row, 1)}, seen
    assert_agrees(mean, var, gm, gv, "hip textured box %s" % integrator)


@pytest.mark.gpu
def test_pin_rejects_a_transposed_bitmap(gpu_rgb, monkeypatch):
    """the mutation this pin must reject: the floor's bitmap with x and y exchanged"""
    import tests.kernel_rows as kr
    for switch in kr.SWITCHES:
        monkeypatch.delenv(switch, raising=False)
    mean, var = load_pin()
    d = problems_textured.box_textured()[0]
    d["floor"]["bsdf"]["reflectance"]["data"] = np.ascontiguousarray(problems_textured.FLOOR.transpose(1, 0, 2))
    gm, gv = rgb_estimate(hip_render(gpu_rgb, set()), d, 16, 1024)
    assert rejected(mean, var, gm, gv, "hip textured box, bitmap transposed")
