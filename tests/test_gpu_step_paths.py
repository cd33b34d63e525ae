"""Every way through the ring machines' tracking step, film and loop counters against the oracle bit for bit.

The lean units a / b / c run the tracking step as straight-line code (csrc/volpath_flat.h: VolpathMachine::step_fast) and send a lane
through the general step (blk_med + top) only when it meets one of that step's uncommon paths.  One small scene per path: the common
one; a majorant without an invariant reciprocal (the scalar branch around the whole form); a medium whose sigma_n is zero (every walk
dies at its first collision, every collision of the main path is real); a depth limit that real collisions reach; voxels of 1e-30
(dividends outside the window of pm_div_by_invariant: the per-lane guard); a ragged film (idle paths in the workgroup); gpu_mono; and
the spectral variant and 16 x 16 blocks, whose units keep the general step.  One 32 x 32 block (a 1024-path workgroup) or one
16 x 16 block (256 paths) each, 4 - 8 spp; every case is rendered with and without loop counters (the COUNT = true / false
instantiations) and asserts the kernel that served it, so that no case silently runs per lane.

Without a GPU: the oracle finishes every scene, its counters show that the scene reaches the path it is named after where they can,
and the host-side kernel table chooses the kernel the GPU cases assert."""
import ctypes as C
import importlib

import numpy as np
import pytest

import tests.oracle_binding as ob

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

RES = 8
LEAN_A_RING_1024, GENERAL_RING_256 = 111024, 10256          # mts_stats.kernel_variant


def f32(bits):
    return float(np.uint32(bits).view(np.float32))


def grid_medium(data, albedo=0.9):
    xf = T.translate([-50, -50, 0]) @ T.scale([100, 100, 2])
    return {"type": "heterogeneous",
            "sigma_t": {"type": "gridvolume", "data": np.ascontiguousarray(data, np.float32), "to_world": xf},
            "albedo": {"type": "gridvolume", "data": np.full(data.shape, albedo, np.float32), "to_world": xf},
            "scale": 1.0, "phase": {"type": "hg", "g": 0.8}}


def slab(data, width=32, height=32, spp=8, max_depth=-1):
    return scenes._slab_scene(grid_medium(data), width, height, spp, max_depth, 5)


def all_ones_majorant():
    g = np.random.default_rng(5).uniform(0.1, 1.9, (RES, RES, RES)).astype(np.float32)
    g[3, 4, 5] = f32(0x3fffffff)                             # 1.99999988: an all-ones significand, pm_invariant_rcp gives 0
    return g


def tiny_voxels():
    """The lower half of the slab 1e-30 (trilinear lookups there give 1e-30: below 2^-62), the upper half O(1), majorant 2."""
    g = np.random.default_rng(6).choice(np.float32([0.5, 1.25, 2.0]), (RES, RES, RES)).astype(np.float32)
    g[:RES // 2] = np.float32(1e-30)
    g[RES - 1, 0, 0] = 2.0
    return g


def case_scene(case):
    """-> (scene dict, oracle keywords, package variant, expected kernel_variant)"""
    if case == "common":
        return scenes.c3_heterogeneous(32, 32, 8, res=RES), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "plain_division":
        return slab(all_ones_majorant()), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "dead_walks":
        return slab(np.ones((RES, RES, RES), np.float32)), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "depth_limit":
        return scenes.c3_heterogeneous(32, 32, 8, res=RES, max_depth=2), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "tiny_dividends":
        return slab(tiny_voxels()), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "ragged_film":
        return scenes.c3_heterogeneous(20, 12, 8, res=RES), {}, "gpu_rgb", LEAN_A_RING_1024
    if case == "mono":
        return scenes.c3_heterogeneous(32, 32, 4, res=RES), {"mono": True}, "gpu_mono", LEAN_A_RING_1024
    if case == "blocks_16":
        d = scenes.c3_heterogeneous(16, 16, 8, res=RES)
        d["integrator"]["block_size"] = 16
        return d, {}, "gpu_rgb", GENERAL_RING_256
    if case == "spectral_16":
        d = scenes.c3_heterogeneous(16, 16, 4, res=RES)
        d["integrator"]["block_size"] = 16
        d["ground"] = dict(d["ground"], bsdf={"type": "diffuse", "reflectance": {"type": "uniform", "value": 0.5}})   # no rgb in spectral
        return d, {"spectral": True}, "gpu_spectral", GENERAL_RING_256
    raise KeyError(case)


CASES = ["common", "plain_division", "dead_walks", "depth_limit", "tiny_dividends", "ragged_film", "mono", "blocks_16", "spectral_16"]
_oracle = {}


def oracle(case):
    """film and (n_iter, n_lookup, n_nee_step) of the oracle, rendered once per case"""
    if case not in _oracle:
        d, kw, _, _ = case_scene(case)
        o = ob.OracleScene(d, **kw)
        ref = o.render(threads=16)
        ref.setflags(write=False)
        _oracle[case] = (ref, (o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"]))
    return _oracle[case]


def test_cases_reach_their_paths_on_the_oracle():
    films = {c: oracle(c) for c in CASES}
    for c, (ref, counters) in films.items():
        assert np.isfinite(ref).all() and ref[..., 4].max() > 0 and min(counters) > 0, (c, counters)
    # Dead walks.  sigma_t equals the majorant everywhere (trilerp of a constant 1 is exactly 1), so sigma_n = 0: every collision of the
    # main path is real and starts one NEE walk (directional sun, no depth limit), and the first collision of a walk kills it.  The sun
    # stands above the slab, the ground 0.01 below it, so a walk is one of
    #   started at a collision:  one step in the medium that collides and dies (1 step, 1 lookup), or one that leaves through the top
    #                            face and a step outside that finds nothing (2 steps, 0 lookups) -- with the lookup of the collision
    #                            that started it: 3;
    #   started at the ground:   a step to the bottom face, then the same two cases (2 steps + 1 lookup, or 3 steps): 3.
    # Hence n_nee_step + n_lookup = 3 x walks, and walks <= n_iter (an iteration starts at most one).  A null collision of a walk adds
    # a step and a lookup, one of the main path adds a lookup to the iteration it adds: with sigma_n > 0 the sum outgrows 3 n_iter --
    # shown on the neighbouring scene below, the same slab at half the density under the same majorant.
    it, look, nee = films["dead_walks"][1]
    samples = 32 * 32 * 8
    assert (nee + look) % 3 == 0 and (nee + look) // 3 <= it, (it, look, nee)
    # ... and walks did collide: a path's first iteration crosses the top face without a lookup, so the main path made at most
    # n_iter - samples lookups; the rest were made by walks, each of which died there
    assert look - (it - samples) > 0, (it, look, nee)
    half = np.full((RES, RES, RES), 0.5, np.float32); half[0, 0, 0] = 1.0
    o = ob.OracleScene(slab(half))
    o.render(threads=16)
    it1, look1, nee1 = o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"]
    assert nee1 + look1 > 3 * it1, (it1, look1, nee1)
    it0, nee0 = films["common"][1][0], films["common"][1][2]
    # a depth limit of two cuts every path of the common scene short: the same streams, so a prefix of its iterations and walks
    assert films["depth_limit"][1][0] < it0 and films["depth_limit"][1][2] < nee0
    # the ragged film is the corner of the full block: same streams, fewer pixels
    assert films["ragged_film"][0].shape[:2] == (12, 20)


def test_cases_choose_the_ring_kernels():
    A = importlib.import_module("eradiate-kernel_amd._capi")
    SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    L = A.lib()
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    for case in CASES:
        d, kw, _, expect = case_scene(case)
        desc, keep = SD.build_scene_desc(d, spectral=bool(kw.get("spectral")))
        v = C.c_int32(-1)
        assert L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)) == 0, L.mts_last_error()
        assert v.value == expect, (case, v.value)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_step_paths_match_the_oracle(gpu_rgb, case):
    d, _, variant, expect = case_scene(case)
    ref, counters = oracle(case)
    gpu_rgb.set_variant(variant)
    try:
        for collect in (True, False):                            # the instantiations with and without loop counters
            scene = gpu_rgb.load_dict(d)
            sensor = scene.sensors()[0]
            assert scene.integrator().render(scene, sensor, collect_counters=collect)
            st = scene.integrator().last_stats
            film = np.array(sensor.film().bitmap(raw=True))
            assert st["kernel_variant"] == expect, (case, collect, st["kernel_variant"])
            assert np.array_equal(film, ref), (case, collect, float(np.abs(film - ref).max()), int((film != ref).sum()))
            if collect:
                assert (st["n_iter"], st["n_lookup"], st["n_nee_step"]) == counters, (case, st, counters)
    finally:
        gpu_rgb.set_variant("gpu_rgb")
