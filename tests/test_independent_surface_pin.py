"""An independent pin for surface transport (`path`).

GPU <-> oracle equality is common mode: both follow one reading of src/integrators/path.cpp, and the reference's own fixtures
for this path are component tests plus one end-to-end render (path + directional + one diffuse bounce).  The MIS weights of
emitter and BSDF sampling, the area-to-solid-angle pdf of rectangle / disk / mesh lamps, the cone sampling of a sphere lamp, the
emitter selection probability, the `max_depth` count, the Russian-roulette weight, the back-face rule of `diffuse`, the
transmission side of `bilambertian`, `rpv` as a sampled BSDF and sphere / disk / cube as occluders had no second opinion.

tests/independent/surface.py gives one: a float64 analog walk that samples no emitter, uses no MIS and no roulette, with its own
world-space intersection and BSDFs (see its docstring).  tests/independent/make_pin.py ran it on five problems
(tests/independent/problems_surface.py) and committed mean and variance per pixel and colour channel as
tests/golden/indep_pin_surf_*.npz.  Here, with the statistics and thresholds of tests/test_independent_pin.py: (1) the estimator
against closed forms and against a second sampling density; (2) the fixtures against a live run of the committed estimator;
(3) the oracle under `path`, `volpath` and `volpathmis` against the fixtures, per channel, on the image mean and per pixel;
(4) a `point` emitter against a deterministic quadrature; (5) the pin has teeth: three deliberately wrong renders are rejected."""
import ast
import copy
import functools
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import tests.oracle_binding as ob
from tests.independent import problems_surface, surface
from tests.test_independent_pin import GOLDEN, XYZ_TO_RGB, z_test

CASES = ["box", "box_d3", "orbs", "canopy"]
FIXTURES = CASES + ["orbs_grey", "orbs_balance"]


def fixture_for(name, integrator):
    """The three integrators render a scene without media to one radiance -- except where an rpv surface is lit by an area or
    environment emitter: RPV::sample's weight lacks a factor pi (rpv.cpp:97-104), and what reaches the film then depends on the MIS
    heuristic that splits the light between emitter and BSDF sampling: the power heuristic in `path` and `volpath`, the balance
    heuristic in `volpathmis` (tests/independent/surface.py's docstring has the derivation).  Measured on `orbs`: `volpathmis` lies
    +3.7 % / +5.0 % / +7.5 % (r / g / b) above `path`.  The estimator restates both; `orbs` under `volpathmis` is held against the
    fixture of the second."""
    return "orbs_balance" if (name, integrator) == ("orbs", "volpathmis") else name


def load_surf_pin(name):
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_%s_16x16.npz" % name))
    return z["mean"], z["var"], int(z["per_pixel"])


def rgb_estimate(render, d, seeds, spp):
    """Per-pixel mean [h, w, 3] and variance of the mean of the linear RGB radiance from `seeds` renders (render(dict) -> XYZAW film)."""
    imgs = []
    for seed in range(seeds):
        dd = copy.deepcopy(d)
        dd["sensor"]["sampler"]["sample_count"] = spp
        dd["sensor"]["sampler"]["seed"] = seed
        imgs.append(dd)
    imgs = np.array([(film[..., :3] / film[..., 4:5]) @ XYZ_TO_RGB.T for film in render(imgs)], np.float64)
    return imgs.mean(0), imgs.var(0, ddof=1) / seeds


def oracle_render(dicts):
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(lambda dd: ob.OracleScene(dd).render(threads=1), dicts))


# A pixel that lies wholly on the black lamp of the cornell box (an emitting shape without a BSDF reflects nothing, shape.cpp:75-81)
# has the lamp's radiance in every sample: no variance on either side, and a Z statistic of 0 / 0 or of rounding / 0.  Such a pixel is
# deterministic and is held tighter than any Z-test would: to the fp32 error of the film.  A pixel's XYZ sums take 256 or 1024 equal
# addends per render, each sum within (n - 1) 2^-24 <= 6.1e-5 of the exact one, and XYZ -> RGB adds three products of which the
# largest is 3.24 x 0.95 of the grey result (cancellation x 5.2 in red): 5.2 x 6.1e-5 = 3.2e-4 at most.  It counts as accepted by
# the Z-test only if it passes that.
DETERMINISTIC_TOL = 3.2e-4


def compare(mean, var, gm, gv, label):
    """Per channel: relative difference of the image means, its combined standard error, share of the pixels the Z-test accepts."""
    out = []
    for c, ch in enumerate("rgb"):
        m, v, a, b = mean[..., c], var[..., c], gm[..., c], gv[..., c]
        se = math.hypot(math.sqrt(v.sum()) / v.size / m.mean(), math.sqrt(b.sum()) / b.size / a.mean())
        rel = a.mean() / m.mean() - 1.0
        fixed = v == 0.0                                                             # every walk of the fixture returned one value
        with np.errstate(divide="ignore", invalid="ignore"):
            p, alpha, z = z_test(a, b, m, v)
        ok = np.where(fixed, np.abs(a - m) <= DETERMINISTIC_TOL * np.abs(m), p > alpha)
        out.append((rel, se, float(ok.mean())))
        print("%s channel %s: image mean %.6f, independent %.6f, difference %+.3f %% +- %.3f %%, pixels accepted %.4f, max |z| %.2f, %d deterministic pixels"
              % (label, ch, a.mean(), m.mean(), 100 * rel, 100 * se, out[-1][2], z[~fixed].max(), fixed.sum()))
    return out


def assert_agrees(mean, var, gm, gv, label):
    for rel, se, accepted in compare(mean, var, gm, gv, label):
        assert se < 2.5e-3                                                           # the sensitivity this pin claims (test_independent_pin.py)
        assert abs(rel) < 4 * se and abs(rel) < 1e-2, (label, rel, se)
        assert accepted >= 0.9975, (label, accepted)


def rejected(mean, var, gm, gv, label):
    return any(abs(rel) >= 4 * se or accepted < 0.9975 for rel, se, accepted in compare(mean, var, gm, gv, label))


def test_surface_estimator_imports_nothing_from_the_product_or_the_oracle():
    src = open(surface.__file__).read()
    mods = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            mods |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods.add((node.module or "").split(".")[0])
    assert mods == {"math", "numpy"}, mods
    assert "ctypes" not in src and "oracle" not in src.replace("oracle/", "").replace("the oracle", "")


# ---- (1) the estimator itself ------------------------------------------------------------------------------------------------
def _cosine_directions(rng, n):
    u1, u2 = rng.random(n), rng.random(n)
    r, ph = np.sqrt(u1), 2.0 * math.pi * u2
    return np.stack([r * np.cos(ph), r * np.sin(ph), np.sqrt(1.0 - u1)], axis=1)


def test_estimator_reproduces_the_irradiance_below_a_disk_lamp():
    """A Lambertian disk of radius R and radiance L at height h, facing down: E = pi L R^2 / (R^2 + h^2) at the point below its
    centre.  The estimator sees E as pi x the mean radiance over cosine-distributed directions; tilted and shifted so that the
    disk is not axis-aligned."""
    L, R, h = 2.5, 1.3, 2.0
    axis = np.array([0.3, -0.5, 0.81]); axis /= np.linalg.norm(axis)
    x0 = np.array([0.7, -1.1, 0.4])
    lamp = surface.Disk(x0 + h * axis, -axis, R, surface.Material("black", Le=L))
    scene = surface.Scene([lamp])
    rng = np.random.Generator(np.random.Philox(11))
    n = 400000
    d = surface._about(np.broadcast_to(axis, (n, 3)), _cosine_directions(rng, n)[:, 2], 2.0 * math.pi * rng.random(n))
    val = math.pi * surface.radiance(scene, rng, np.broadcast_to(x0, (n, 3)).copy(), d, max_depth=1)[:, 0]
    expected = math.pi * L * R * R / (R * R + h * h)
    se = val.std() / math.sqrt(n)
    print("disk lamp: E %.5f, closed form %.5f, standard error %.5f" % (val.mean(), expected, se))
    assert se < 5e-3 * expected and abs(val.mean() - expected) < 4 * se
    behind = surface.radiance(scene, rng, np.broadcast_to(x0 + 2 * h * axis, (n, 3)).copy(), -d, max_depth=1)      # the back does not emit
    assert not behind.any()


@pytest.mark.parametrize("density", ["cosine", "uniform"])
def test_estimator_reproduces_the_surface_furnace(density):
    """Inside a closed diffuse box whose walls all emit Le and reflect rho, L = Le / (1 - rho) everywhere, whatever the shape --
    with either sampling density for the diffuse walls (cosine: every walk returns the truncated geometric series itself)."""
    Le, rho = 1.5, 0.6
    m = surface.Material("diffuse", rho, Le=Le)
    a, b, c = 1.0, 1.7, 0.6                                                          # half sizes; normals inwards
    walls = [surface.Rectangle([0, 0, -c], [a, 0, 0], [0, b, 0], m), surface.Rectangle([0, 0, c], [a, 0, 0], [0, -b, 0], m),
             surface.Rectangle([0, b, 0], [a, 0, 0], [0, 0, c], m), surface.Rectangle([0, -b, 0], [a, 0, 0], [0, 0, -c], m),
             surface.Rectangle([-a, 0, 0], [0, 0, -c], [0, b, 0], m), surface.Rectangle([a, 0, 0], [0, 0, c], [0, b, 0], m)]
    for w in walls:
        assert w.n @ w.c < 0                                                        # faces the origin
    scene = surface.Scene(walls, diffuse_density=density)
    vertices = 48
    bound = surface.remainder_bound(scene, vertices)
    assert bound < 1e-8
    rng = np.random.Generator(np.random.Philox(12))
    n = 20000
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = rng.uniform([-0.9 * a, -0.9 * b, -0.9 * c], [0.9 * a, 0.9 * b, 0.9 * c], (n, 3))
    val = surface.radiance(scene, rng, o, d, max_vertices=vertices)
    expected = Le / (1.0 - rho)
    se = val[:, 0].std() / math.sqrt(n)
    print("furnace (%s): L %.6f, closed form %.6f, standard error %.6f" % (density, val[:, 0].mean(), expected, se))
    assert se < 5e-3 * expected and abs(val[:, 0].mean() - expected) <= 4 * se + bound + 1e-12
    assert np.array_equal(val[:, 0], val[:, 2])


def test_rpv_weight_under_two_sampling_densities_and_a_quadrature():
    """The radiance of an rpv plane under a uniform sky of radiance 1 seen at max_depth = 2 is its directional albedo, the integral
    of f cos over the hemisphere.  The walk's uniform-hemisphere density (weight 2 pi f cos), its cosine density (weight pi f) and
    a midpoint quadrature of the formula must agree; with the reference's sampling rule the walk gives what `path` computes there:
    albedo x (w_e + w_b / pi) under the integral."""
    params = (0.2, 0.7, -0.1, 0.2)
    rng = np.random.Generator(np.random.Philox(13))
    n = 200000
    for cos_i in (0.95, 0.5):
        wi = np.array([math.sqrt(1 - cos_i * cos_i), 0.0, cos_i])
        o = np.broadcast_to(np.array([0.3, 0.2, 0.0]) + 3.0 * wi, (n, 3)).copy()
        d = np.broadcast_to(-wi, (n, 3)).copy()
        k = 400
        mu = (np.arange(k) + 0.5) / k                                                 # cos_o
        ph = (np.arange(k) + 0.5) / k * 2.0 * math.pi
        MU, PH = np.meshgrid(mu, ph)
        cos_io = cos_i * MU + math.sqrt(1 - cos_i * cos_i) * np.sqrt(1 - MU * MU) * np.cos(PH)
        f = surface.rpv_brdf(params, cos_i, MU, cos_io)
        albedo = float((f * MU).mean() * 2.0 * math.pi)
        # path.cpp's MIS weights for a sky sampled uniformly over the sphere by one emitter against cosine BSDF sampling
        pe, pb = 1.0 / (4.0 * math.pi), MU / math.pi
        we = pe * pe / (pe * pe + pb * pb)
        reference = float((f * MU * (we + (1.0 - we) / math.pi)).mean() * 2.0 * math.pi)
        for rule, expected in (("physical", albedo), ("reference", reference)):
            for density in ("uniform", "cosine"):
                scene = surface.Scene([surface.Disk([0, 0, 0], [0, 0, 1], 50.0, surface.Material("rpv", rpv=params))], env=1.0, n_emitters=1,
                                      rpv_rule=rule, rpv_density=density)
                val = surface.radiance(scene, rng, o, d, max_depth=2)[:, 1]
                se = val.std() / math.sqrt(n)
                print("rpv cos_i %.2f %s %s: %.6f, quadrature %.6f, standard error %.6f" % (cos_i, rule, density, val.mean(), expected, se))
                assert se < 5e-3 * expected and abs(val.mean() - expected) < 4 * se + 1e-4 * expected


@pytest.mark.parametrize("name", FIXTURES)
def test_problem_is_well_posed(name):
    """Every sensor ray meets a surface (a pixel of pure sky or of nothing has no variance on either side: nothing to test), and
    what the fixed vertex count leaves out is below 1e-5 of the image mean."""
    mean, var, _ = load_surf_pin(name)
    _, scene, cam, max_depth, vertices = getattr(problems_surface, name)()
    g = (np.arange(64) + 0.5) / 64
    sx, sy = np.meshgrid(g, g)
    _, pid = scene.intersect(*cam.rays(sx.ravel(), sy.ravel()))
    assert (pid >= 0).all()
    assert np.isfinite(mean).all()
    fixed = (var == 0).all(-1)                                                       # deterministic pixels: only the four on the box's black lamp
    assert ((var == 0).any(-1) == fixed).all() and fixed.sum() == (4 if name.startswith("box") else 0)
    assert (mean[fixed] == 3.0).all()
    if max_depth < 0:
        if name.startswith("orbs"):                                                  # emission behind an rpv vertex counts up to pi-fold (surface.py: pi w_e + w_b)
            bound = surface.remainder_bound(scene, vertices, problems_surface.ORBS_MAX_ALBEDO, emission_factor=math.pi)
        else:
            bound = surface.remainder_bound(scene, vertices)
        print("%s: remainder after %d vertices < %.2e of the image mean" % (name, vertices, bound / mean.mean((0, 1)).min()))
        assert bound < 1e-5 * mean.mean((0, 1)).min()
    se = np.sqrt(var.sum((0, 1))) / (cam.w * cam.h) / mean.mean((0, 1))
    assert (se < 2e-3).all(), se                                                     # the precision target of the fixtures


def test_rpv_albedo_bound_of_the_orbs_problem():
    """`remainder_bound` takes the largest albedo of the scene; for the rpv ground of `orbs` that is stated, not read off a
    parameter.  Under the reference's sampling rule the weight behind an rpv vertex is its directional albedo / pi: that stays below
    ORBS_MAX_ALBEDO down to grazing incidence (cos_i = 0.01), by quadrature."""
    rho0, k, g = problems_surface.ORBS["rpv"]
    n = 600
    mu = (np.arange(n) + 0.5) / n
    ph = (np.arange(n) + 0.5) / n * 2.0 * math.pi
    MU, PH = np.meshgrid(mu, ph)
    worst = 0.0
    for cos_i in np.linspace(0.01, 1.0, 34):
        cos_io = cos_i * MU + math.sqrt(1 - cos_i * cos_i) * np.sqrt(1 - MU * MU) * np.cos(PH)
        worst = max(worst, float((surface.rpv_brdf((rho0, k, g, rho0), cos_i, MU, cos_io) * MU).mean() * 2.0 * math.pi))
    print("largest directional albedo of the rpv ground: %.3f" % worst)
    assert worst / math.pi < problems_surface.ORBS_MAX_ALBEDO


# ---- (2) the fixtures come from the committed code --------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_surface_fixture_comes_from_the_committed_estimator(name):
    """A short live run of the estimator agrees with its fixture (same code, other seed, 64 walks per pixel)."""
    mean, var, _ = load_surf_pin(name)
    _, scene, cam, max_depth, vertices = getattr(problems_surface, name)()
    m, v = surface.render(scene, cam, 64, 77, max_depth, vertices)
    for c in range(3):
        se = math.sqrt(v[..., c].sum() + var[..., c].sum()) / m[..., c].size
        assert abs(m[..., c].mean() - mean[..., c].mean()) < 4 * se
        # 64 walks do not give a usable per-pixel variance: compare 4 x 4 tiles of 16 pixels instead
        tm, tv = m[..., c].reshape(4, 4, 4, 4).mean((1, 3)), v[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        fm, fv = mean[..., c].reshape(4, 4, 4, 4).mean((1, 3)), var[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        p, alpha, _ = z_test(tm, tv, fm, fv)
        assert (p > alpha).all()


# ---- (3) the oracle against the fixtures -----------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["path", "volpath", "volpathmis"])
@pytest.mark.parametrize("name", CASES)
def test_oracle_agrees_with_the_independent_surface_estimator(name, integrator):
    """`path`, and `volpath` / `volpathmis`, which must render a scene without media to the same radiance (volpath.cpp and
    volpathmis.cpp carry their own emitter sampling, MIS and roulette), 16 seeds x 256 spp, per colour channel."""
    mean, var, _ = load_surf_pin(fixture_for(name, integrator))
    d = getattr(problems_surface, name)()[0]
    d["integrator"] = dict(d["integrator"], type=integrator)
    gm, gv = rgb_estimate(oracle_render, d, 16, 256)
    assert_agrees(mean, var, gm, gv, "%s %s" % (name, integrator))


def grey_to_uniform(node):
    """grey rgb colours -> uniform spectra (the spectral variant has no sRGB upsampling model)"""
    if isinstance(node, dict):
        if node.get("type") == "rgb":
            v = np.atleast_1d(np.asarray(node["value"], np.float64))
            assert np.all(v == v[0])
            return float(v[0])
        return {k: grey_to_uniform(x) for k, x in node.items()}
    return node


def y_bar_integral():
    """Integral of the piecewise-linear y-bar table over 360 .. 830 nm (test_spectral_oracle_agrees_with_the_independent_estimator)."""
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "eradiate-kernel_amd", "csrc", "cie_tables.h")).read()
    tbl = np.array([float(x) for x in re.findall(r"([0-9.eE+-]+)f", src.split("{")[1])], np.float64).reshape(3, 95)
    y_integral = float(((tbl[1][:-1] + tbl[1][1:]) * 0.5 * 5.0).sum())
    assert abs(y_integral - 106.857) < 1e-2
    return y_integral


def spectral_estimate(render, d, seeds, spp):
    """Per-pixel mean and variance of the mean of Y / W / integral of y-bar: the radiance of a grey scene, as the rgb variant's green."""
    norm = y_bar_integral()
    dicts = []
    for seed in range(seeds):
        dd = copy.deepcopy(d)
        dd["sensor"]["sampler"]["sample_count"] = spp
        dd["sensor"]["sampler"]["seed"] = seed
        dicts.append(dd)
    imgs = np.array([film[..., 1] / film[..., 4] / norm for film in render(dicts)], np.float64)
    return imgs.mean(0), imgs.var(0, ddof=1) / seeds


def assert_grey_agrees(mean, var, gm, gv, label):
    """One channel of assert_agrees: the green channel of the grey fixture against the spectral render's luminance."""
    m, v = mean[..., 1], var[..., 1]
    se = math.hypot(math.sqrt(v.sum()) / v.size / m.mean(), math.sqrt(gv.sum()) / gv.size / gm.mean())
    rel = gm.mean() / m.mean() - 1.0
    p, alpha, z = z_test(gm, gv, m, v)
    print("%s: image mean %.6f, independent %.6f, difference %+.3f %% +- %.3f %%, pixels accepted %.4f, max |z| %.2f"
          % (label, gm.mean(), m.mean(), 100 * rel, 100 * se, (p > alpha).mean(), z.max()))
    assert se < 2.5e-3 and abs(rel) < 4 * se and abs(rel) < 1e-2, (rel, se)
    assert (p > alpha).mean() >= 0.9975


def test_spectral_oracle_agrees_with_the_independent_surface_estimator():
    """`orbs` with grey colours as uniform spectra in the spectral variant (four wavelengths per sample, CIE weighting, the
    four-wide `path`): Y / W divided by the y-bar integral against the green channel of the grey twin's fixture."""
    mean, var, _ = load_surf_pin("orbs_grey")
    def render(dicts):
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            return list(ex.map(lambda dd: ob.OracleScene(dd, spectral=True).render(threads=1), dicts))
    gm, gv = spectral_estimate(render, grey_to_uniform(problems_surface.orbs_grey()[0]), 16, 256)
    assert_grey_agrees(mean, var, gm, gv, "orbs spectral path")


# ---- (4) a point emitter against a quadrature --------------------------------------------------------------------------------
@functools.lru_cache(None)
def point_direct_expected():
    _, scene, cam, _, _ = problems_surface.point_direct()
    c = problems_surface.POINT
    expected, smooth = surface.point_direct_image(scene, cam, c["position"], c["intensity"], sub=64)
    coarse, _ = surface.point_direct_image(scene, cam, c["position"], c["intensity"], sub=32)
    # the quadrature has converged where the integrand is smooth: halving the step moves it by less than 1e-4 (midpoint rule: the
    # error falls by 4 per halving, so what is left at sub = 64 is a third of that)
    assert (np.abs(coarse - expected)[smooth] <= 1e-4 * expected[smooth]).all()
    assert smooth.mean() >= 0.75, smooth.mean()                                      # at most a quarter of the pixels straddle an edge
    lit = expected[smooth].sum(-1) > 0
    assert lit.any() and (~lit).any()                                                # lit pixels and pixels in full shadow are both held
    return expected, smooth


def assert_point_direct(gm, gv, label):
    expected, smooth = point_direct_expected()
    z = np.abs(gm - expected)[smooth] / np.maximum(np.sqrt(gv[smooth]), 1e-30)
    rel = (gm[smooth].sum() / expected[smooth].sum()) - 1.0
    print("%s: %d of %d pixels held, sum over them %+.4f %% off the quadrature, max |z| %.2f" % (label, smooth.sum(), smooth.size, 100 * rel, z[np.isfinite(z)].max()))
    # within 4 standard errors of the render; the quadrature's own error (above: < 3.4e-5) and the film's fp32 sums (4096 terms, < 1e-5) beside it
    assert (np.abs(gm - expected)[smooth] <= 4.0 * np.sqrt(gv[smooth]) + 5e-5 * expected[smooth]).all()


def test_oracle_point_emitter_against_the_quadrature():
    """`point` (point.cpp:80-107): intensity / r^2, a delta emitter that only emitter sampling can reach.  Expected pixel radiance:
    the float64 quadrature of rho / pi x I cos / r^2 x V over the pixel footprint, on the pixels no silhouette or shadow edge crosses."""
    d = problems_surface.point_direct()[0]
    gm, gv = rgb_estimate(oracle_render, d, 16, 256)
    assert_point_direct(gm, gv, "point_direct oracle")


# ---- (5) the pin has teeth ---------------------------------------------------------------------------------------------------
def test_pin_rejects_a_depth_count_off_by_one():
    mean, var, _ = load_surf_pin("box_d3")
    d = problems_surface.box(max_depth=4)[0]
    gm, gv = rgb_estimate(oracle_render, d, 16, 256)
    assert rejected(mean, var, gm, gv, "box_d3 against max_depth 4")


def test_pin_rejects_a_lamp_sphere_five_percent_larger():
    mean, var, _ = load_surf_pin("orbs")
    d = problems_surface.orbs(lamp_radius_factor=1.05)[0]
    gm, gv = rgb_estimate(oracle_render, d, 16, 256)
    assert rejected(mean, var, gm, gv, "orbs against a lamp radius x 1.05")


def test_pin_rejects_leaves_with_reflectance_and_transmittance_swapped():
    mean, var, _ = load_surf_pin("canopy")
    d = problems_surface.canopy(swap=True)[0]
    gm, gv = rgb_estimate(oracle_render, d, 16, 256)
    assert rejected(mean, var, gm, gv, "canopy against rho <-> tau")
