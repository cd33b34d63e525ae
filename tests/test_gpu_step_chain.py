"""The tracking step with its voxel-independent half under the grid gathers: film and loop counters against the oracle bit for bit.

VolpathMachine::step_fast (csrc/volpath_flat.h, lean units a / b / c) issues the four gathers of a lookup and forms, before it waits
for them, everything of the step that reads no voxel: the distance, its transmittance and sampling weight, the walk's bound, the main
path's draws.  That code stands inside the waterfall over the lanes' media, so it runs once per medium of a wave, on that medium's
lanes alone, and a rare lane must still leave with the state it came with.  One small scene per way through it:

  c3             the metric scene in miniature
  spike          the same with one voxel fifty times the rest: a majorant far above the typical density, long runs of null collisions,
                 in-place repeats up to the cap of 16 rounds
  two_media      two heterogeneous media of different majorants side by side in the view: a wave's waterfall runs two iterations
  depth_rr       max_depth 3, rr_depth 1: the depth limit at a real collision (a rare lane), the roulette draw at every null collision
  plain_division a majorant with an all-ones significand (inv_max_density == 0): the whole step goes rare by value
  point_light    a point emitter inside the slab: NEE walks end by their remaining distance, not at the boundary
  c4             the atmosphere in miniature on unit b: a profile in z, two gathers per lookup
  canopy         the C3 miniature over 45 leaves, more primitives than a walked list holds: a BVH, unit c

One 32 x 32 block (a 1024-path workgroup) each, 4 - 8 spp, grids of 16^3 or smaller; every case is rendered with and without loop
counters and asserts the unit that served it.  Without a GPU: the oracle finishes every scene and the host-side kernel table chooses
the unit the GPU cases assert."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.kernel_rows as kr
import tests.oracle_binding as ob

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

RES = 16
RING_1024 = kr.ring(1024)


def grid_medium(data, xf=None, albedo=0.9):
    xf = xf if xf is not None else T.translate([-50, -50, 0]) @ T.scale([100, 100, 2])
    return {"type": "heterogeneous",
            "sigma_t": {"type": "gridvolume", "data": np.ascontiguousarray(data, np.float32), "to_world": xf},
            "albedo": {"type": "gridvolume", "data": np.full(data.shape, albedo, np.float32), "to_world": xf},
            "scale": 1.0, "phase": {"type": "hg", "g": 0.8}}


def slab(data, spp=8):
    return scenes._slab_scene(grid_medium(data), 32, 32, spp, -1, 5)


def spike():
    g = scenes.c3_sigma_t_grid(RES)
    g[RES // 2, RES // 2, RES // 2] *= np.float32(50.0)
    return slab(g, spp=4)


def two_media():
    """The slab cut in two along x = 0, a gap of one unit between the halves; the right half ten times as dense as the left one."""
    d = scenes._slab_scene(None, 32, 32, 8, -1, 5)
    del d["slab"]
    base = scenes.c3_sigma_t_grid(8)
    for name, x0, factor in (("slab_left", -50.0, 1.0), ("slab_right", 0.5, 10.0)):
        xf = T.translate([x0, -50, 0]) @ T.scale([49.5, 100, 2])
        d[name] = {"type": "cube", "to_world": T.translate([x0 + 24.75, 0, 1]) @ T.scale([24.75, 50, 1]), "bsdf": {"type": "null"},
                   "interior": grid_medium(base * np.float32(factor), xf)}
    return d


def all_ones_majorant():
    g = np.random.default_rng(5).uniform(0.1, 1.9, (RES, RES, RES)).astype(np.float32)
    g[3, 4, 5] = np.nextafter(np.float32(2.0), np.float32(0.0))     # 0x3fffffff: pm_invariant_rcp gives 0
    return slab(g)


def point_light():
    d = scenes.c3_heterogeneous(32, 32, 8, res=RES)
    del d["sun"]
    d["lamp"] = {"type": "point", "position": [0.5, -0.25, 1.0], "intensity": {"type": "rgb", "value": [30.0, 25.0, 20.0]}}
    return d


def canopy():
    d = scenes.c3_heterogeneous(32, 32, 4, res=RES)
    rng = np.random.default_rng(11)
    for k in range(45):
        c = rng.uniform([-3, -3, 0.2], [3, 3, 1.5])
        d["leaf%02d" % k] = {"type": "rectangle", "to_world": T.translate(c) @ T.rotate(rng.normal(size=3), float(rng.uniform(0, 180))) @ T.scale(0.4),
                             "bsdf": {"type": "bilambertian", "reflectance": {"type": "rgb", "value": [0.1, 0.45, 0.08]},
                                      "transmittance": {"type": "rgb", "value": [0.05, 0.4, 0.04]}}}
    return d


# case -> (scene, the units that may serve it)
CASES = {
    "c3": (lambda: scenes.c3_heterogeneous(32, 32, 8, res=RES), (kr.A,)),
    "spike": (spike, (kr.A,)),
    "two_media": (two_media, (kr.A,)),
    "depth_rr": (lambda: scenes.c3_heterogeneous(32, 32, 8, res=RES, max_depth=3, rr_depth=1), (kr.A,)),
    "plain_division": (all_ones_majorant, (kr.A,)),
    "point_light": (point_light, (kr.A, kr.B, kr.C)),
    "c4": (lambda: scenes.c4_atmosphere(32, 32, 4, layers=8), (kr.B,)),
    "canopy": (canopy, (kr.C,)),
}
_oracle = {}


def oracle(case):
    """film and (n_iter, n_lookup, n_nee_step) of the oracle, rendered once per case"""
    if case not in _oracle:
        o = ob.OracleScene(CASES[case][0]())
        ref = o.render(threads=16)
        ref.setflags(write=False)
        _oracle[case] = (ref, (o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"]))
    return _oracle[case]


def test_cases_reach_their_paths_on_the_oracle():
    films = {c: oracle(c) for c in CASES}
    for c, (ref, counters) in films.items():
        assert np.isfinite(ref).all() and ref[..., 4].max() > 0 and ref[..., :3].max() > 0 and min(counters) > 0, (c, counters)
    samples = 32 * 32 * 8
    # the spike (a mid-height voxel of about 0.3, times fifty) lifts the majorant from about 2 to about 16 over the same densities
    # elsewhere: the lookups per sample, nearly all of them null collisions, grow by nearly that factor -- at least fourfold
    assert films["spike"][1][1] / (samples // 2) > 4 * films["c3"][1][1] / samples, (films["spike"][1], films["c3"][1])
    # a depth limit of three cuts every path of the plain scene short: fewer iterations and walk steps
    assert films["depth_rr"][1][0] < films["c3"][1][0] and films["depth_rr"][1][2] < films["c3"][1][2]


def test_cases_choose_their_units():
    A = importlib.import_module("eradiate-kernel_amd._capi")
    SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    L = A.lib()
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    for case, (make, units) in CASES.items():
        desc, keep = SD.build_scene_desc(make())
        v = C.c_int32(-1)
        assert L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)) == 0, L.mts_last_error()
        assert kr.stat_unit(v.value) in units and kr.stat_variant(v.value) == RING_1024, (case, v.value)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_under_the_gathers_matches_the_oracle(gpu_rgb, case):
    make, units = CASES[case]
    d = make()
    ref, counters = oracle(case)
    for collect in (True, False):                                # the instantiations with and without loop counters
        scene = gpu_rgb.load_dict(d)
        sensor = scene.sensors()[0]
        assert scene.integrator().render(scene, sensor, collect_counters=collect)
        st = scene.integrator().last_stats
        film = np.array(sensor.film().bitmap(raw=True))
        assert st["kernel_variant"] // 100000 in units and st["kernel_variant"] % 100000 == RING_1024, (case, collect, st["kernel_variant"])
        assert np.array_equal(film, ref), (case, collect, float(np.abs(film - ref).max()), int((film != ref).sum()))
        if collect:
            assert (st["n_iter"], st["n_lookup"], st["n_nee_step"]) == counters, (case, st, counters)
