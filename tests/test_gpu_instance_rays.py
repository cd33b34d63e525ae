"""Instanced intersection per ray on the device (run with -m gpu on an MI355X); the inputs and their conditions: tests/instance_rays.py,
tests/test_instance_rays.py.

(a) exact: on dyadic placements the device's t, member and primitive (mts_ray_intersect: intersect_kernel<true>, inst_intersect,
hit_point) are the oracle's on the expanded plain scene, bit for bit, on every ray of the four sets; (b) general placements against
the float64 restatement within 8 x the fp32 scale measured on the dyadic scene; (c) the four list / BVH combinations of the two
levels; (d) shadow rays with a finite maxt (ray_test<true>) through every kernel row, against a closed form."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.instance_rays as ir
import tests.transport_cases as tc
from tests.test_gpu_textures import ATOL, bits, render

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")


def structures(scene):
    """(the scene level has a BVH, a group has one)"""
    counts, box = (C.c_int32 * 6)(), (C.c_float * 6)()
    A.check(A.lib().mts_debug_scene_geometry(C.byref(scene._desc), counts, box))
    return counts[4] > 0, counts[5] > counts[4]


def assert_exact(scene, which):
    results, where = ir.expanded_oracle(which)
    for name, rays in ir.ray_sets(which).items():
        got, want = scene.ray_intersect(*rays), results[name]
        hit = np.isfinite(want["t"])
        print("%s %s: t differs on %d of %d rays, %d hit" % (which, name, int(np.sum(bits(got["t"]) != bits(want["t"]))), len(hit), int(hit.sum())))
        assert np.array_equal(bits(got["t"]), bits(want["t"])), name
        assert np.array_equal(got["shape"][hit], where[want["shape"][hit], 1]) and np.all(got["shape"][~hit] == -1), name
        assert np.array_equal(got["prim_index"], want["prim_index"]), name


def test_dyadic_placements_equal_the_expanded_oracle(gpu_rgb):
    scene = gpu_rgb.load_dict(ir.dyadic_grove())
    assert structures(scene) == (False, False)                             # 26 and 34 primitives: lists at the default threshold
    assert_exact(scene, "dyadic")


@pytest.mark.parametrize("which,threshold,want", [("dyadic", "100", (False, False)), ("dyadic", "30", (False, True)), ("dyadic", "0", (True, True)),
                                                  ("dyadic_wide", "34", (True, False))])
def test_structures(gpu_rgb, monkeypatch, which, threshold, want):
    """list / list, list / BVH, BVH / BVH; BVH / list needs a scene level above the larger group's 34 primitives: 17 placements of group B"""
    monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", threshold)
    scene = gpu_rgb.load_dict(ir.GROVES[which]())
    assert structures(scene) == want
    assert_exact(scene, which)


@pytest.mark.parametrize("threshold", [None, "0"])
def test_general_placements_against_float64(gpu_rgb, monkeypatch, threshold):
    """Each instanced path adds two fp32 affine transforms (the ray to group space, p back to world), a few roundings of
    eps x |coordinate| x |scale| each: a factor 8 over the plain fp32 intersection (E_t, E_p, E_n of instance_rays.fp32_scale).  The
    ABI does not return the instance: p tells two instances of one group apart."""
    if threshold is not None:
        monkeypatch.setenv("MTSAMD_BVH_THRESHOLD", threshold)
    e_t, e_p, e_n = ir.fp32_scale()
    assert 8 * max(e_t, e_p, e_n) <= ATOL
    scene = gpu_rgb.load_dict(ir.general_grove())
    assert structures(scene) == ((False, False) if threshold is None else (True, True))
    worst = np.zeros(3)
    for name, rays in ir.ray_sets("general").items():
        got, ref = scene.ray_intersect(*rays), ir.reference("general", name)
        keep = ir.kept(ref, e_t)
        hit = np.isfinite(ref["t"])
        assert np.array_equal(np.isfinite(got["t"])[keep], hit[keep]), name
        k = keep & hit
        assert np.array_equal(got["shape"][k], ref["member"][k]) and np.all(got["shape"][keep & ~hit] == -1), name
        assert np.array_equal(got["prim_index"][k], ref["prim"][k]), name
        err = [np.abs(got["t"][k] - ref["t"][k]).max(), np.abs(got["p"][k] - ref["p"][k]).max(), np.abs(got["n"][k] - ref["n"][k]).max()]
        print("general %s: max |t - ref| = %.3g, |p - ref| = %.3g, |n - ref| = %.3g on %d rays" % (name, err[0], err[1], err[2], int(k.sum())))
        worst = np.maximum(worst, err)
    print("bounds 8 E_t = %.3g, 8 E_p = %.3g, 8 E_n = %.3g; device maxima %.3g, %.3g, %.3g" % (8 * e_t, 8 * e_p, 8 * e_n, *worst))
    assert worst[0] <= 8 * e_t and worst[1] <= 8 * e_p and worst[2] <= 8 * e_n


def test_dyadic_points_and_normals_against_float64(gpu_rgb):
    """p and n of the dyadic scene, which the exactness argument does not cover: the bounds of the general placements"""
    e_t, e_p, e_n = ir.fp32_scale()
    scene = gpu_rgb.load_dict(ir.dyadic_grove())
    for name, rays in ir.ray_sets("dyadic").items():
        got, ref = scene.ray_intersect(*rays), ir.reference("dyadic", name)
        k = ir.kept(ref, e_t) & np.isfinite(ref["t"])
        err = [np.abs(got["p"][k] - ref["p"][k]).max(), np.abs(got["n"][k] - ref["n"][k]).max()]
        print("dyadic %s: max |p - ref| = %.3g, |n - ref| = %.3g" % (name, err[0], err[1]))
        assert err[0] <= 8 * e_p and err[1] <= 8 * e_n, name


@pytest.mark.parametrize("how,row", [("path", 1), ("nested", 0), ("ring", 11024), ("volpathmis", 0), ("sample", None)])
def test_shadow_rays(gpu_rgb, monkeypatch, how, row):
    """ray_test<true> with a finite maxt: occluders between the ground and the lamp shadow it, occluders beyond the lamp on the same
    line do not"""
    integrator = {"ring": "volpath", "volpathmis": "volpathmis"}.get(how, "path")
    d, o, w, expected, keep, visible, beyond = ir.shadow_case(integrator, medium=how == "ring")
    assert (visible & beyond & keep).sum() >= 16                           # lit points with an occluder behind the lamp
    if how == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    scene = gpu_rgb.load_dict(d)
    if how == "sample":
        rgb, valid = scene.integrator().sample(scene, o, w)
        assert valid.all()
        got = rgb.astype(np.float64)
    else:
        film, st = render(scene)
        assert st["textured"] == 2 and st["kernel_variant"] == row
        assert np.all(np.asarray(film)[0][:, 4] == 4.0)
        got = tc.radiance_rgb(film)[0]
    print("%s: max |L - expected| = %.3g on %d segments, %d of them occluded" % (how, np.abs(got - expected)[keep].max(), int(keep.sum()), int((~visible & keep).sum())))
    assert np.abs(got - expected)[keep].max() <= ATOL
