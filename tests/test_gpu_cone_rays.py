"""The `cone` shape per ray on the device (run with -m gpu on an MI355X): mts_ray_intersect -> intersect_kernel<true> -> inst_intersect ->
cone_intersect_v, hit_point, complete_surface (csrc/integrator_dev.h).  Inputs, reference and exclusion rules: tests/cone_ref.py; their
conditions are asserted on the CPU in tests/test_cone.py.

(a) the reference's own grid (src/shapes/tests/test_cone.py: test_ray_intersect), with the shadow query on every ray and the cone's lit
side against a closed form, through every INST kernel; (b) turned plain
cones and cones inside instances against the float64 reference within 8 x the fp32 scale of instance_rays.fp32_scale(), on lists and on
BVHs; (c) a dyadic placement bit for bit against the same cone as a plain shape; (d) flip_normals, with the reference's shift of the
point along the flipped normal."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.cone_ref as cr
import tests.instance_rays as ir
import tests.transport_cases as tc
from tests.test_gpu_textures import ATOL, bits, render

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f


def structures(scene):
    """(the scene level has a BVH, a group has one)"""
    counts, box = (C.c_int32 * 6)(), (C.c_float * 6)()
    A.check(A.lib().mts_debug_scene_geometry(C.byref(scene._desc), counts, box))
    return counts[4] > 0, counts[5] > counts[4]


# ================================================================ (a) the reference's grid
GROUND_Y, RHO, SUN = -10.5, 0.5, 2.0


def grid_scene(r, l, o, integrator="path", medium=False):
    """The cone scale(r, r, l) of the reference's test.  Behind the rays' origins (y = -10) a diffuse ground at y = -10.5 looks along +y,
    lit by a directional emitter that shines along -y.  2 n radiancemeters: the first n look at the ground from y = -10.25 at each grid
    ray's (x, z); with max_depth = 2 they see rho / pi x E x V, V the shadow query (ray_test under ShadowRay, with the emitter's finite
    maxt) along the grid ray's own line, started half a unit further back.  The second n look along -y from y = +10 at the same (x, z),
    at the cone's lit side: rho / pi x E x n_y where they hit it, the lit ground where they miss."""
    fmt = lambda a: ", ".join("%.9g" % v for v in np.asarray(a).ravel())
    near, far = o.copy(), o.copy()
    near[:, 1], far[:, 1] = GROUND_Y + 0.25, 10.0
    white = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [RHO] * 3}}
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": 2},
         "foo": {"type": "cone", "to_world": T.scale([r, r, l]), "bsdf": white},
         "ground": {"type": "rectangle", "to_world": T.translate([0, GROUND_Y, 0]) @ T.rotate([1, 0, 0], -90) @ T.scale([10, 12, 1]), "bsdf": white},
         "sun": {"type": "directional", "direction": [0, -1, 0], "irradiance": SUN},
         "sensor": {"type": "mradiancemeter", "origins": fmt(np.r_[near, far]), "directions": fmt(np.tile([0.0, -1.0, 0.0], (2 * len(o), 1))),
                    "film": {"type": "hdrfilm", "width": 2 * len(o), "height": 1, "rfilter": {"type": "box"}},
                    "sampler": {"type": "independent", "sample_count": 4}}}
    if medium:                                                          # a medium of no effect (optical depth < 1e-7) puts `volpath` on its ring row
        xf = T.translate([-16, -16, -16]) @ T.scale(32.0)
        grid = lambda v: {"type": "gridvolume", "data": np.full((2, 2, 2), v, np.float32), "to_world": xf}
        d["air"] = {"type": "cube", "to_world": T.scale(16.0), "bsdf": {"type": "null"},
                    "interior": {"type": "heterogeneous", "sigma_t": grid(1e-9), "albedo": grid(0.5), "phase": {"type": "isotropic"}}}
    return d


def grid_film(scene, r, l, o, hit):
    """the film of grid_scene against the closed forms; `hit`: the device's closest-hit answer on the grid rays (from y = -10 along +y)"""
    film, st = render(scene)
    assert st["textured"] == 2
    lit = tc.radiance_rgb(film)[0][:, 1].astype(np.float64)
    expected, n = RHO / np.pi * SUN, len(o)
    visible = lit[:n] > 0.5 * expected
    assert np.all(np.abs(lit[:n][visible] - expected) <= ATOL) and np.all(lit[:n][~visible] == 0.0)
    assert np.array_equal(~visible, hit), (r, l)                           # the shadow query agrees with the closest-hit query on EVERY ray
    # from the other side the same lines meet the cone where the grid rays do (the cone is convex across a line): its lit side
    back = o.copy()
    back[:, 1] = 10.0
    ref = cr.reference_hits([("foo", cr.Placed(cr.Cone([0, 0, 0], cr.Z, r, l)))], back, np.tile([0.0, -1.0, 0.0], (n, 1)))
    assert np.array_equal(np.isfinite(ref["t"]), hit)
    want = np.where(hit, expected * np.maximum(ref["n"][:, 1], 0.0), expected)
    print("grid r = %d, l = %d, row %d: max |L - closed form| = %.3g on the cone's lit side" % (r, l, st["kernel_variant"], np.abs(lit[n:] - want).max()))
    assert np.abs(lit[n:] - want).max() <= ATOL
    return st


@pytest.mark.parametrize("r", cr.GRID_R)
def test_reference_grid(gpu_rgb, r):
    e_t = ir.fp32_scale()[0]
    for l in cr.GRID_L:
        o, d = cr.grid_rays(r, l)
        scene = gpu_rgb.load_dict(grid_scene(r, l, o))
        got = scene.ray_intersect(o, d)
        ref = cr.reference_hits([("foo", cr.Placed(cr.Cone([0, 0, 0], cr.Z, r, l)))], o, d)
        keep, hit = cr.kept(ref, e_t), np.isfinite(got["t"])
        assert np.array_equal(hit[keep], np.isfinite(ref["t"])[keep]), (r, l)
        assert np.all(got["shape"][hit] == 0) and np.all(got["prim_index"][hit] == 0) and np.all(got["shape"][~hit] == -1)
        r_h = (l - o[:, 2].astype(np.float64)) / l * r
        on_cone = np.abs(got["p"][:, 0].astype(np.float64) ** 2 + got["p"][:, 1].astype(np.float64) ** 2 - r_h ** 2)
        assert np.all(on_cone[hit] <= 2e-2), (r, l, on_cone[hit].max())
        print("grid r = %d, l = %d: %d of %d rays hit, %d kept, max |x^2 + y^2 - r_h^2| = %.3g" % (r, l, int(hit.sum()), len(hit), int(keep.sum()), on_cone[hit].max() if hit.any() else 0.0))
        assert grid_film(scene, r, l, o, hit)["kernel_variant"] == 1                       # `path`: the flat row, in its INST loop


@pytest.mark.parametrize("how,row", [("nested", 0), ("ring", 11024), ("volpathmis", 0)])
def test_grid_film_on_the_other_rows(gpu_rgb, monkeypatch, how, row):
    """the grid's two closed forms (shadow query, the cone's lit side) through the nested INST kernel, `volpath` on the ring INST kernel
    and `volpathmis`: every INST kernel shades a cone and casts shadow rays at one"""
    r, l = 2, 5
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    o, d = cr.grid_rays(r, l)
    scene = gpu_rgb.load_dict(grid_scene(r, l, o, {"ring": "volpath", "volpathmis": "volpathmis"}.get(how, "path"), medium=how == "ring"))
    hit = np.isfinite(cr.reference_hits([("foo", cr.Placed(cr.Cone([0, 0, 0], cr.Z, r, l)))], o, d)["t"])
    assert grid_film(scene, r, l, o, hit)["kernel_variant"] == row


# ================================================================ (b) against the float64 reference
def compare(scene, which, e):
    """-> the device maxima of |t - ref|, |p - ref|, |n - ref| over the kept hits of the four sets; hit / miss, member and prim asserted"""
    d, prims = cr.scene(which)
    index = cr.shape_indices(d)
    member = np.array([index[name] for name, _ in prims] + [-1])
    worst = np.zeros(3)
    for name, rays in cr.ray_sets(which).items():
        got, ref = scene.ray_intersect(*rays), cr.reference(which, name)
        keep, hit = cr.kept(ref, e[0]), np.isfinite(ref["t"])
        assert np.array_equal(np.isfinite(got["t"])[keep], hit[keep]), name
        k = keep & hit
        assert np.array_equal(got["shape"][k], member[ref["winner"][k]]) and np.all(got["shape"][keep & ~hit] == -1), name
        assert np.all(got["prim_index"][k] == 0), name
        dn = np.abs(got["n"][k] - ref["n"][k]).max(1)
        err = [np.abs(got["t"][k] - ref["t"][k]).max(), np.abs(got["p"][k] - ref["p"][k]).max(), dn.max()]
        rho = ref["rho"][k]
        by_rho = ["%.3g" % (dn[(rho >= lo) & (rho < hi)].max() if np.any((rho >= lo) & (rho < hi)) else 0.0) for lo, hi in ((0, .05), (.05, .1), (.1, .25), (.25, .75), (.75, np.inf))]
        print("%s %s: max |t - ref| = %.3g, |p - ref| = %.3g, |n - ref| = %.3g on %d rays; |n - ref| by distance from the axis [0, .05, .1, .25, .75, inf): %s"
              % (which, name, err[0], err[1], err[2], int(k.sum()), " ".join(by_rho)))
        worst = np.maximum(worst, err)
    return worst


@pytest.mark.parametrize("threshold", [None, "0"])
@pytest.mark.parametrize("which", ["plain", "grove"])
def test_cones_against_float64(gpu_rgb, monkeypatch, which, threshold):
    """The bound and the argument of test_gpu_instance_rays.test_general_placements_against_float64: two fp32 affine transforms (the ray
    to group or object space, p back) around an otherwise exact test (the quadratic is solved in double) cost a factor 8 over the plain
    fp32 intersection.  The scale is the oracle's on meshes, rectangles, disks and spheres; the code under test is not involved."""
    if threshold is not None:
        monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", threshold)
    e = ir.fp32_scale()
    assert 8 * max(e) <= ATOL
    scene = gpu_rgb.load_dict(cr.scene(which)[0])
    assert structures(scene) == ((False, False) if threshold is None else (True, which == "grove"))
    worst = compare(scene, which, e)
    print("%s: bounds 8 E_t = %.3g, 8 E_p = %.3g, 8 E_n = %.3g; device maxima %.3g, %.3g, %.3g" % (which, 8 * e[0], 8 * e[1], 8 * e[2], *worst))
    assert worst[0] <= 8 * e[0] and worst[1] <= 8 * e[1] and worst[2] <= 8 * e[2]


# ================================================================ (c) exact
def test_dyadic_placement_equals_the_plain_cone(gpu_rgb):
    """One cone with r = 1/2, l = 1 and a dyadic base point, placed by translate(T) diag(2, 2, 1/2), against the same cone written as a
    plain shape with the composed transform: t is equal BIT FOR BIT on every ray of the four sets.  The argument: R = I and every scale
    is a power of two, so the instance's to_object takes origin and direction to group space without rounding (origins are multiples
    of 2^-8, T of 2^-3), and the member's rigid to_object subtracts a dyadic base point exactly.  The plain cone's host record recovers
    r' = 2 r, l' = l / 2 from exact column norms and the rigid translation T + S base; its object-space origin and direction are the
    instanced ones times (2, 2, 1/2), exactly.  The direction is never renormalised.  So k' = (r' / l')^2 = 2^4 k exactly, and A, B,
    C of the quadratic are the instanced ones times 2^2 -- each term is scaled by one and the same power of two, so every rounding in
    double falls the same way -- the discriminant scales by 2^4, its root by 2^2, and the roots t are equal; the heights z scale by
    1/2 like l, so the nappe tests decide alike.  p (the translation rounds at another magnitude) and n go to the bounds of (b)."""
    e = ir.fp32_scale()
    inst, plain = gpu_rgb.load_dict(cr.scene("dyadic")[0]), gpu_rgb.load_dict(cr.dyadic_plain())
    hits = 0
    for name, rays in cr.ray_sets("dyadic").items():
        a, b = inst.ray_intersect(*rays), plain.ray_intersect(*rays)
        differ = int(np.sum(bits(a["t"]) != bits(b["t"])))
        hits += int(np.isfinite(a["t"]).sum())
        print("dyadic %s: t differs on %d of %d rays, %d hit" % (name, differ, len(a["t"]), int(np.isfinite(a["t"]).sum())))
        assert differ == 0, name
        assert np.all(a["prim_index"][np.isfinite(a["t"])] == 0) and np.all(b["prim_index"][np.isfinite(b["t"])] == 0)
    assert hits >= 1024
    worst = compare(inst, "dyadic", e)
    print("dyadic: device maxima |t|, |p|, |n| = %.3g, %.3g, %.3g" % tuple(worst))
    assert worst[1] <= 8 * e[1] and worst[2] <= 8 * e[2]


# ================================================================ (d) flip_normals
FAR = 1024.0


def test_flip_normals_turns_n_and_shifts_p_the_other_way(gpu_rgb):
    """cone.cpp:378-383: the point moves along the normal by s = r (l - z) / l - |xy|, what the object-space point lacks to lie on the
    cone, AFTER flip_normals has turned the normal.  An unflipped cone's point so moves towards the surface; a flipped cone's point moves
    the same distance AWAY from it.  Restated: with p_u and p_f the device's points of the two twins on
    one ray, their midpoint m is the raw point ray(t), and (p_u - p_f) / 2 = n s(m) with n and s from cone_ref in float64.  The rays
    start 1 024 units away, so that s (the fp32 error of ray(t), ~ 2^-24 x 1024) stands well above the tolerance: the rounding of the
    sums at the cone's own coordinates (<= 4) and of s itself, 16 x 2^-24 x 4."""
    base, axis, angle, r, l = [0.5, -0.25, 0.25], [1.0, 0.5, 0.25], 40.0, 1.5, 2.0
    scenes = []
    for flip in (False, True):
        name, cd, cone = cr._cone_pair("foo", base, axis, angle, r, l, flip)
        d = cr._base()
        d[name] = cd
        scenes.append((gpu_rgb.load_dict(d), cone))
    rng = np.random.default_rng(700)
    target = np.array([scenes[0][1].point(rng, 0.8) for _ in range(cr.N_RAYS)])
    w = cr._unit(rng, cr.N_RAYS)
    o = (target - FAR * w).astype(np.float32)
    w = w.astype(np.float32)
    u, f = scenes[0][0].ray_intersect(o, w), scenes[1][0].ray_intersect(o, w)
    hit = np.isfinite(u["t"])
    assert hit.sum() >= 0.9 * cr.N_RAYS
    assert np.array_equal(bits(u["t"]), bits(f["t"]))
    assert np.array_equal(bits(f["n"][hit]), bits(-u["n"][hit]))                        # turned, bit for bit
    cone = scenes[0][1]
    pu, pf = u["p"][hit].astype(np.float64), f["p"][hit].astype(np.float64)
    m = 0.5 * (pu + pf)
    s = cone.off_surface(m)
    tol = 16 * 2.0 ** -24 * 4.0
    ref = cr.reference_hits([("foo", cr.Placed(cone))], o[hit], w[hit])
    facing = np.abs(ref["cos"]) >= cr.MIN_COS                                            # (the normal at m is the hit's: away from grazing rays)
    n = cone.normal(m)
    half = 0.5 * (pu - pf)
    err = np.abs(half - n * s[:, None]).max(1)
    print("flip: max |s| = %.3g, max |(p_u - p_f) / 2 - n s| = %.3g (tolerance %.3g) on %d rays" % (np.abs(s[facing]).max(), err[facing].max(), tol, int(facing.sum())))
    assert np.abs(s[facing]).max() > 4 * tol                                             # the rays do show the shift
    assert err[facing].max() <= tol
    # (a step s along the normal closes s h / l of the gap across the axis, h = sqrt(l^2 + r^2): the unflipped point keeps s (1 - h / l))
    left = s * (1.0 - np.hypot(l, r) / l)
    assert np.abs(cone.off_surface(pu) - left)[facing].max() <= tol
