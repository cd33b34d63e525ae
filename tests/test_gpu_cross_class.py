"""The ring kernels' class for null-boundary crossings (csrc/volpath_flat.h: B_CROSS), film and loop counters against the oracle bit for bit.

A main path that hits a shape with a null BSDF and no emitter (the slab cube of the benchmark scenes) waits in a ring of its own and
runs the surface blocks with those facts as constants; DScene::cross_mask (scene_host.cpp) says which shapes these are.  Sending such
a hit to the general class is always right, sending anything else to the new one is a bug, so there is one small scene per way that
could happen: the common scene, with roulette acting at crossings as early as the loader lets it (rr_depth 1: it refuses 0, as the
reference does) and with the depth limit in reach of one
(max_depth 2); a null-BSDF shape that is an area emitter (general unit: no bit); a null-BSDF rectangle that switches no medium; a
camera inside the medium (the first surface event is an exit); a camera that sees past the scene (no hit: the general class); a
boundary behind 64 other shapes (no bit in the mask; its 77 primitives are walked, as unit a wants them, by raising the host's BVH
threshold for that scene) and the most shapes unit a takes as it is; a ragged film; gpu_mono; units b and h; volpathmis, which never names the class.
One 32 x 32 block (a 1024-path workgroup) or less, 4 - 16 spp, 8^3 grids; every case renders with and without loop counters.
The oracle alone would not notice a class that is never used (the general class serves every hit correctly), so the render with
counters also says how many lane-visits the class served (mts_debug_cross_visits): at least one per sample on units a and b,
whose every camera ray enters the medium through the boundary, none where the kernel has no such class or the boundary has no bit.

Without a GPU: the oracle finishes every scene and the cases differ where they are meant to, and the mask is pinned on six hand-built
shape lists through the host scene (mts_debug_cross_mask)."""
import ctypes as C
import importlib
import os
import threading

import numpy as np
import pytest

import tests.oracle_binding as ob

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

RES = 8
LEAN_A_RING_1024, LEAN_B_RING_1024, LEAN_H_RING_1024 = 111024, 211024, 611024          # mts_stats.kernel_variant


def diffuse(rgb):
    return {"type": "diffuse", "reflectance": {"type": "rgb", "value": rgb}}


def common(width=32, height=32, spp=8, **kw):
    """the ground (diffuse) under the slab cube (null BSDF, the medium inside), seen from z = 20.  The loader takes a scene's entries in
    the order of their names, so the ground is shape 0 and the slab shape 1"""
    return scenes.c3_heterogeneous(width, height, spp, res=RES, **kw)


def null_emitter():
    d = common()
    d["lamp"] = {"type": "rectangle", "to_world": T.translate([1, -1, 4]) @ T.rotate([1, 0, 0], 180) @ T.scale(2.0), "bsdf": {"type": "null"},
                 "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [2.0, 1.5, 1.0]}}}
    return d


def null_veil():
    d = common()
    d["veil"] = {"type": "rectangle", "to_world": T.translate([0.5, 0.5, 3]) @ T.rotate([0, 1, 0], 10) @ T.scale(3.0), "bsdf": {"type": "null"}}
    return d


def camera_inside():
    d = common(spp=8)
    d["sensor"]["to_world"] = T.look_at([0.3, 0.2, 1.5], [1.0, 0.5, 0], [0, 1, 0])
    d["sensor"]["medium"] = d["slab"]["interior"]
    return d


def sees_past():
    d = common()
    d["sensor"]["to_world"] = T.look_at([0, -150, 12], [0, 0, 6], [0, 0, 1])       # the upper rows look over the slab into nothing
    return d


def boundary_beyond_the_mask(tiles=32):
    """`tiles` small diffuse tiles above the slab, whose names sort in front of the others: with 64 of them the ground is shape 64, the slab shape 65"""
    d = common(spp=4)
    for k in range(tiles):
        x, y = -7.0 + 2.0 * (k % 8), -7.0 + 2.0 * (k // 8)
        d["a_tile_%02d" % k] = {"type": "rectangle", "to_world": T.translate([x, y, 2.5 + 0.01 * k]) @ T.scale(0.3), "bsdf": diffuse([0.1 + 0.01 * k, 0.5, 0.9 - 0.01 * k])}
    return d


def case_scene(case):
    """-> (scene dict, oracle keywords, package variant, expected kernel_variant or None)"""
    if case == "common":
        return common(), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "roulette_at_crossings":
        return common(rr_depth=1), {}, "gpu_rgb", LEAN_A_RING_1024      # the smallest value the loader takes
    if case == "depth_limit_at_a_crossing":
        return common(spp=16, max_depth=2), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "null_emitter":
        return null_emitter(), {}, "gpu_rgb", None
    if case == "null_veil":
        return null_veil(), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "camera_inside":
        return camera_inside(), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "sees_past":
        return sees_past(), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "boundary_beyond_the_mask":
        return boundary_beyond_the_mask(64), {}, "gpu_rgb", LEAN_A_RING_1024      # under WALKED (below)
    if case == "boundary_at_the_mask_end":
        return boundary_beyond_the_mask(27), {}, "gpu_rgb", LEAN_A_RING_1024      # 27 tiles + 12 triangles + the ground: 40 primitives, the most without a BVH
    if case == "ragged_film":
        return common(20, 12), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "mono":
        return common(spp=4), {"mono": True}, "gpu_mono", LEAN_A_RING_1024
    if case == "unit_b":
        return scenes.c4_atmosphere(32, 32, 4, layers=8), {}, "gpu_rgb", LEAN_B_RING_1024
    if case == "unit_h":
        return scenes.c2_homogeneous_slab(32, 32, 4), {}, "gpu_rgb", LEAN_H_RING_1024
    if case == "volpathmis":
        d = common()
        d["integrator"]["type"] = "volpathmis"
        return d, {}, "gpu_rgb", None
    raise KeyError(case)


CASES = ["common", "roulette_at_crossings", "depth_limit_at_a_crossing", "null_emitter", "null_veil", "camera_inside", "sees_past",
         "boundary_beyond_the_mask", "boundary_at_the_mask_end", "ragged_film", "mono", "unit_b", "unit_h", "volpathmis"]
# cases whose kernel sorts crossings AND whose boundary has a bit in the mask; every other case must report no visit of the class
FILLS_THE_RING = ("common", "roulette_at_crossings", "depth_limit_at_a_crossing", "null_veil", "camera_inside",
                  "boundary_at_the_mask_end", "ragged_film", "mono", "unit_b")
NO_COUNT_ASSERTED = ("sees_past",)     # its subject is the ray without a hit; how few of its rays meet the slab at all is not pinned
WALKED = {"boundary_beyond_the_mask": {"MTSAMD_BVH_THRESHOLD": "100"}}      # environment of the host scene's construction, per case
_oracle = {}


class environment:
    """the process environment with `values` set, for the time a scene is built"""
    def __init__(self, values):
        self.values, self.saved = values, {}

    def __enter__(self):
        for k, v in self.values.items():
            self.saved[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def oracle(case):
    """film and (n_iter, n_lookup, n_nee_step) of the oracle, rendered once per case"""
    if case not in _oracle:
        d, kw, _, _ = case_scene(case)
        o = ob.OracleScene(d, **kw)
        ref = o.render(threads=16)
        ref.setflags(write=False)
        _oracle[case] = (ref, (o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"]))
    return _oracle[case]


def test_cases_finish_on_the_oracle_and_their_conditions_hold():
    for c in CASES:
        ref, counters = oracle(c)
        assert np.isfinite(ref).all() and ref[..., 4].max() > 0 and counters[0] > 0, (c, counters)
    common_film = oracle("common")[0]
    assert oracle("ragged_film")[0].shape[:2] == (12, 20)
    # roulette from depth 2 on and the depth limit both change the film: they act where the common case (rr_depth 5) does not
    assert not np.array_equal(oracle("roulette_at_crossings")[0], common_film)
    assert oracle("depth_limit_at_a_crossing")[1][0] / 16 < oracle("common")[1][0] / 8      # iterations per sample: 16 spp at max_depth 2, 8 spp without a limit
    # the emitting null shape is seen; the veil draws three more samples per crossing, so the film differs although nothing shades it
    assert not np.array_equal(oracle("null_emitter")[0], common_film)
    assert not np.array_equal(oracle("null_veil")[0], common_film)
    # a camera that looks past the scene has pixels without a single valid sample (alpha 0), the common one has none
    assert (oracle("sees_past")[0][..., 3] == 0).any() and not (common_film[..., 3] == 0).any()
    assert not np.array_equal(oracle("camera_inside")[0], common_film)


def lib():
    A = importlib.import_module("eradiate-kernel_amd._capi")
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    L = A.lib()
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    L.mts_debug_cross_mask.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_uint64)]
    L.mts_debug_cross_visits.argtypes = [C.POINTER(C.c_uint64)]
    return A, L


def test_cases_choose_the_kernels_they_are_meant_for():
    A, L = lib()
    SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
    for case in CASES:
        d, _, _, expect = case_scene(case)
        desc, keep = SD.build_scene_desc(d)
        v = C.c_int32(-1)
        with environment(WALKED.get(case, {})):
            assert L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)) == 0, L.mts_last_error()
        if expect is not None:
            assert v.value == expect, (case, v.value)
        else:
            assert v.value not in (LEAN_A_RING_1024, LEAN_B_RING_1024), (case, v.value)     # the units that sort crossings


def cross_mask_of(d):
    A, L = lib()
    SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
    desc, keep = SD.build_scene_desc(d)
    m = C.c_uint64(~0 & 0xFFFFFFFFFFFFFFFF)
    assert L.mts_debug_cross_mask(C.byref(desc), C.byref(m)) == 0, L.mts_last_error()
    return m.value


def test_cross_mask_of_hand_built_shape_lists():
    """bit i: shape i has a null BSDF and no emitter, i < 64 -- six lists, shape indices in the order of the entries' names"""
    assert cross_mask_of(common()) == 0b10                                       # ground, slab
    d = common()
    d["a_slab"] = d.pop("slab")
    assert cross_mask_of(d) == 0b01                                              # slab, ground
    assert cross_mask_of(null_emitter()) == 0b100                                # ground, a null shape that emits (lamp), slab
    assert cross_mask_of(null_veil()) == 0b110                                   # ground, slab, a null shape that switches no medium (veil)
    d = common()
    d["slab"]["bsdf"] = diffuse([0.5, 0.5, 0.5])
    assert cross_mask_of(d) == 0                                                 # no null BSDF anywhere
    far = boundary_beyond_the_mask(64)                                           # 64 tiles, ground (64), slab (65)
    far["veil"] = null_veil()["veil"]                                            # ... and a null shape at 66
    assert cross_mask_of(far) == 0
    near = boundary_beyond_the_mask(62)                                          # 62 tiles, ground (62), slab (63): the last bit
    assert cross_mask_of(near) == 1 << 63


def render_and_compare(pkg, case):
    d, _, variant, expect = case_scene(case)
    ref, counters = oracle(case)
    pkg.set_variant(variant)
    try:
        for collect in (True, False):                            # the instantiations with and without loop counters
            with environment(WALKED.get(case, {})):
                scene = pkg.load_dict(d)
            sensor = scene.sensors()[0]
            assert scene.integrator().render(scene, sensor, collect_counters=collect)
            st = scene.integrator().last_stats
            film = np.array(sensor.film().bitmap(raw=True))
            if expect is not None:
                assert st["kernel_variant"] == expect, (case, collect, st["kernel_variant"])
            assert np.array_equal(film, ref), (case, collect, float(np.abs(film - ref).max()), int((film != ref).sum()))
            if collect:
                assert (st["n_iter"], st["n_lookup"], st["n_nee_step"]) == counters, (case, st, counters)
                visits = C.c_uint64(0)
                assert lib()[1].mts_debug_cross_visits(C.byref(visits)) == 0
                samples = film.shape[0] * film.shape[1] * int(d["sensor"]["sampler"]["sample_count"])
                if case in FILLS_THE_RING:                      # the ninth ring is in use: the class is not merely correct by never running
                    # one crossing per camera ray at least where every ray enters through the boundary; a camera inside leaves through it
                    # unless the path ends first
                    floor = {"camera_inside": samples // 8}.get(case, samples)
                    assert visits.value >= floor, (case, visits.value, samples)
                elif case not in NO_COUNT_ASSERTED:
                    assert visits.value == 0, (case, visits.value)
    finally:
        pkg.set_variant("gpu_rgb")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_cross_class_matches_the_oracle(gpu_rgb, case):
    render_and_compare(gpu_rgb, case)


@pytest.mark.gpu
def test_cancel_in_flight_leaves_the_finished_samples(gpu_rgb):
    """Integrator::cancel while paths wait in every ring, B_CROSS among them: what wg_flush_unfinished promises -- the film is finite,
    W counts the finished samples of each pixel (whole numbers, fewer than were asked for) and alpha never exceeds it.  A cancel that
    arrives ahead of the launch stops the render before it has a kernel in flight: the next attempt waits a little longer for the
    render thread before it cancels (its waits end with the thread, none is a fixed sleep)."""
    spp = 32768                                                   # one workgroup: seconds of kernel time if nothing stopped it
    scene = gpu_rgb.load_dict(common(spp=spp))
    integ, sensor = scene.integrator(), scene.sensors()[0]
    for attempt in range(8):
        result = {}

        def run():
            result["ok"] = integ.render(scene, sensor)
        th = threading.Thread(target=run)
        th.start()
        th.join(0.02 * attempt)                                   # returns at once when the render is over
        for _ in range(3000):                                     # cancel until the render has returned: a cancel ahead of its start is reset by it
            integ.cancel()
            th.join(0.01)
            if not th.is_alive():
                break
        assert not th.is_alive() and result["ok"] is False        # render() returns !m_stop
        st = integ.last_stats
        assert st["kernel_variant"] == LEAN_A_RING_1024 and st["cancelled"] == 1, st
        if st["kernel_launches"] == 1:
            break
    assert st["kernel_launches"] == 1, st                         # the cancel met a kernel in flight
    film = np.array(sensor.film().bitmap(raw=True))
    w = film[..., 4]
    assert np.isfinite(film).all()
    assert np.array_equal(w, np.round(w)) and w.min() >= 0 and w.max() < spp, (float(w.min()), float(w.max()))
    assert (film[..., 3] <= w).all() and (film[..., :3] >= 0).all()
