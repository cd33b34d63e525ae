"""The independent float64 transport pin of `dielectric` / `conductor`, without a GPU: the analog walk with Fresnel interfaces
(tests/independent/specular.py), its problem (problems_specular.py: the lit box with a glass sphere, a tilted coloured conductor plate
and a `twosided(conductor)` panel) and its fixture tests/golden/indep_pin_surf_specular_16x16.npz (make_pin_specular.py).
tests/test_gpu_specular_pin.py holds the device against the fixture."""
import ast
import importlib
import math
import os

import numpy as np

from tests.independent import problems_specular, specular, surface
from tests.test_independent_pin import GOLDEN, z_test
from tests.test_independent_surface_pin import rejected
from tests.test_textures import desc_digest, describe

A = importlib.import_module("eradiate-kernel_amd._capi")


def load_pin():
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_specular_16x16.npz"))
    return z["mean"], z["var"], z


def test_estimator_imports_nothing_from_the_product_or_the_oracle():
    for name in ("specular.py", "problems_specular.py"):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "independent", name)
        tree = ast.parse(open(path).read())
        mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
               [(n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert not [m for m in mods if "eradiate" in m or "oracle" in m or "specular_ref" in m or m == "importlib"], mods


def test_fresnel_of_the_walk():
    """closed values: normal incidence ((n - 1) / (n + 1))^2, Brewster's angle (r_p = 0), the critical angle, reciprocity, and a
    conductor with k = 0 against the dielectric of the same index; the perfect mirror eta = 0, k = 1"""
    R, c2 = specular.dielectric_reflectance(np.array([1.0]), 1.0, 1.5)
    assert np.isclose(R[0], 0.04, rtol=1e-12) and np.isclose(c2[0], 1.0)
    brewster = math.cos(math.atan(1.5))
    R, c2 = specular.dielectric_reflectance(np.array([brewster]), 1.0, 1.5)
    r_s = (brewster - 1.5 * c2[0]) / (brewster + 1.5 * c2[0])
    assert np.isclose(R[0], 0.5 * r_s * r_s, rtol=1e-12)
    critical = math.sqrt(1.0 - (1.0 / 1.5) ** 2)
    R, c2 = specular.dielectric_reflectance(np.array([critical - 1e-9, critical + 1e-6]), 1.5, 1.0)
    assert R[0] == 1.0 and c2[0] == 0.0 and R[1] < 1.0 and c2[1] > 0.0
    c1 = np.linspace(0.05, 1.0, 20)
    R_in, c_in = specular.dielectric_reflectance(c1, 1.0, 1.5)
    R_out, c_out = specular.dielectric_reflectance(c_in, 1.5, 1.0)
    assert np.allclose(R_in, R_out, rtol=1e-10) and np.allclose(c_out, c1, rtol=1e-10)
    F = specular.conductor_reflectance(c1, np.full(3, 1.5), np.zeros(3))
    assert np.allclose(F, R_in[:, None], rtol=1e-10)
    assert np.allclose(specular.conductor_reflectance(c1, np.zeros(3), np.ones(3)), 1.0, rtol=1e-12)


def test_glass_ball_in_a_furnace():
    """a glass sphere and a perfect mirror under a sky of radiance 1: every walk returns 1 (the index factors cancel in pairs), or
    nothing if it is still inside the ball at the cut"""
    ball = surface.Sphere([0, 0, 0], 1.0, specular.Material("dielectric", rho=1.0, tau=1.0, n_int=1.5, n_ext=1.0))
    mirror = surface.Rectangle([1.9, 0, 0], [0, 0, 1.2], [0, 1.2, 0], specular.Material("conductor", rho=1.0, eta=0.0, k=1.0))
    assert mirror.n[0] < 0
    scene = surface.Scene([ball, mirror], env=1.0)
    cam = surface.Pinhole(8, 8, 40.0, [0, -6, 0.5], [0.6, 0, 0], [0, 0, 1])
    mean, var = specular.render(scene, cam, 64, 3, -1, 40)
    assert mean.max() <= 1.0 + 1e-12 and mean.mean() > 1.0 - 1e-3


def test_problem_is_well_posed():
    d, scene, cam, max_depth, vertices = problems_specular.box_specular()
    mean, var, z = load_pin()
    assert mean.shape == (16, 16, 3) and np.all(mean > 0)
    assert int(z["vertices"]) == vertices and int(z["walks"]) == int(z["per_pixel"]) * 256 and float(z["seconds"]) > 0
    se = np.sqrt(var.sum((0, 1))) / 256 / mean.mean((0, 1))
    assert se.max() < 1.5e-3
    # no pixel is nearly deterministic (the lamp's mirror image filling it: a variance of rounding size, which a Z-test cannot use);
    # the four that see the lamp itself have none at all and are held to DETERMINISTIC_TOL by the comparison
    noisy = var > 0
    assert (~noisy).all(2).sum() == 4 and (np.sqrt(var[noisy]) / mean[noisy]).min() > 2e-3
    bound, alive = specular.remainder_bound(scene, cam, vertices, problems_specular.MAX_INDEX_RATIO, walks_per_pixel=256)
    print("remainder bound %.3g of the mean %.4f (walks alive at the cut: %.3g)" % (bound, mean.mean(), alive))
    assert bound < 1e-4 * mean.mean()
    # a weight never exceeds the cap the bound assumes: colours <= 1, Fresnel <= 1, the index factor <= 1.5^2
    assert max(problems_specular.PLATE["colour"] + problems_specular.PANEL["colour"]) <= 1.0
    assert len(scene.prims) == 6 + 1 + 1 + 2 and problems_specular.sees_the_front()
    front, back = scene.prims[-2], scene.prims[-1]
    assert np.allclose(front.n, -back.n) and np.isclose((front.c - back.c) @ front.n, problems_specular.GAP, rtol=1e-6) and front.area == back.area
    # the dictionary loads, holds ONE panel rectangle with the adapter over one conductor, and the loader puts the rectangles where the
    # hand-turned corners are
    desc, keep = describe(d)
    assert all(desc_digest(desc))
    kinds = [desc.bsdfs[i].type for i in range(desc.bsdf_count)]
    assert kinds.count(A.BSDF_DIELECTRIC) == 1 and kinds.count(A.BSDF_CONDUCTOR) == 2 and kinds.count(A.BSDF_TWOSIDED) == 1
    for prim, kind in ((scene.prims[-3], A.BSDF_CONDUCTOR), (front, A.BSDF_TWOSIDED)):
        shape = desc.shapes[[s for s in range(desc.shape_count) if desc.bsdfs[desc.shapes[s].bsdf].type == kind][0]]
        m = np.array(list(shape.to_world.matrix), np.float64).reshape(4, 4)
        assert np.allclose(m[:3, 0], prim.eu, atol=1e-6) and np.allclose(m[:3, 1], prim.ev, atol=1e-6) and np.allclose(m[:3, 3], prim.c, atol=1e-6)
    # the specular objects matter to the picture: the plain box is another one
    plain = np.load(os.path.join(GOLDEN, "indep_pin_surf_box_16x16.npz"))
    assert rejected(plain["mean"], plain["var"], mean, var, "the box without its specular objects")


def test_fixture_comes_from_the_committed_estimator():
    """A short live run of the estimator agrees with its fixture (same code, other seed, 64 walks per pixel)."""
    mean, var, _ = load_pin()
    _, scene, cam, max_depth, vertices = problems_specular.box_specular()
    m, v = specular.render(scene, cam, 64, 77, max_depth, vertices)
    for c in range(3):
        se = math.sqrt(v[..., c].sum() + var[..., c].sum()) / m[..., c].size
        assert abs(m[..., c].mean() - mean[..., c].mean()) < 4 * se
        tm, tv = m[..., c].reshape(4, 4, 4, 4).mean((1, 3)), v[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        fm, fv = mean[..., c].reshape(4, 4, 4, 4).mean((1, 3)), var[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        p, alpha, _ = z_test(tm, tv, fm, fv)
        assert (p > alpha).all()
