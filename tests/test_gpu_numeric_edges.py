"""Media at the numeric edges of the majorant division, film against the oracle bit for bit.

The fuzzer's media are O(1) (tests/test_gpu_fuzz.py: densities in [0.1, 2.5] x [0.5, 1.5]), so no film comparison reaches the edges of
pm_div_by_invariant (csrc/pmath.h), the division by the majorant in every tracking step: the plain-division fallback (rd == 0: a majorant
with an all-ones significand, or outside the admitted exponents 67..187), dividends outside its window (exact zeros, FLT_MIN and 1e-30
voxels), a chromatic homogeneous medium with a zero channel.  Each scene is rendered by the oracle first under a wall-clock bound (a
huge majorant can stall a path: t stops advancing in fp32) -- that part runs without a GPU -- and only a scene the oracle finishes goes
to the GPU, under the integrator's timeout: volpath and volpathmis, on the lean unit and on the general kernel (MTSAMD_LEAN=0), one case
each in gpu_mono and gpu_spectral.  Film and loop counters must be the oracle's."""
import importlib
import threading

import numpy as np
import pytest

import tests.oracle_binding as ob

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

ORACLE_WALL_S = 60.0
GPU_TIMEOUT_S = 60.0
RES = 8


def f32(bits):
    return float(np.uint32(bits).view(np.float32))


def grid_medium(data, scale=1.0, filter_type="trilinear", albedo=0.8):
    xf = T.translate([-50, -50, 0]) @ T.scale([100, 100, 2])
    return {"type": "heterogeneous",
            "sigma_t": {"type": "gridvolume", "data": np.ascontiguousarray(data, np.float32), "to_world": xf, "filter_type": filter_type},
            "albedo": {"type": "gridvolume", "data": np.full(data.shape, albedo, np.float32), "to_world": xf, "filter_type": filter_type},
            "scale": scale, "phase": {"type": "hg", "g": 0.5}}


def all_ones_grid():
    """O(1) voxels whose maximum 1.99999988 (0x3fffffff) has an all-ones significand: the majorant has no admitted reciprocal."""
    g = np.random.default_rng(5).uniform(0.1, 1.9, (RES, RES, RES)).astype(np.float32)
    g[3, 4, 5] = f32(0x3fffffff)
    return g


def mixed_grid():
    """Exact zeros, FLT_MIN, ~1e-30 and O(1) voxels side by side (max 2.0: an admitted majorant, tiny dividends)."""
    rng = np.random.default_rng(6)
    g = rng.choice(np.float32([0.0, f32(0x00800000), 1e-30, 0.5, 1.25, 2.0]), (RES, RES, RES)).astype(np.float32)
    g[0, 0, 0] = 2.0
    return g


# majorant = scale x 1.0 on a constant grid (nearest filter: every collision real) at both ends of the admitted exponent range
EXTREME = {"exp66": f32((66 << 23) | 0x400000), "exp67": f32(67 << 23), "exp187": f32(187 << 23), "exp188": f32(188 << 23)}


def edge_scene(case, integrator="volpath"):
    if case == "all_ones_max":
        medium, depth = grid_medium(all_ones_grid()), -1
    elif case.startswith("mixed_"):
        medium, depth = grid_medium(mixed_grid(), filter_type=case[len("mixed_"):]), -1
    elif case in EXTREME:
        medium, depth = grid_medium(np.ones((RES, RES, RES), np.float32), scale=EXTREME[case], filter_type="nearest"), 4
    elif case == "chromatic_zero_channel":
        medium, depth = {"type": "homogeneous", "sigma_t": {"type": "rgb", "value": [0.6, 0.0, 1.2]},
                         "albedo": {"type": "rgb", "value": [0.9, 0.7, 0.5]}, "phase": {"type": "hg", "g": 0.5}}, -1
    else:
        raise KeyError(case)
    d = scenes._slab_scene(medium, 24, 24, 8, depth, 5)
    d["integrator"] = dict(d["integrator"], type=integrator, timeout=GPU_TIMEOUT_S)
    return d


CASES = ["all_ones_max", "mixed_trilinear", "mixed_nearest", "exp66", "exp67", "exp187", "exp188", "chromatic_zero_channel"]


def bounded_oracle(d, **kw):
    """The oracle's film and counters; fails (and the scene never reaches the GPU) if it does not finish within ORACLE_WALL_S."""
    o = ob.OracleScene(d, **kw)
    timer = threading.Timer(ORACLE_WALL_S, lambda: o.L.oracle_cancel(o.h))
    timer.start()
    try:
        ref = o.render(threads=16)
    finally:
        timer.cancel()
    assert not o.last_stats["cancelled"], "the oracle did not finish the scene within %.0f s" % ORACLE_WALL_S
    return ref, (o.last_stats["n_iter"], o.last_stats["n_lookup"], o.last_stats["n_nee_step"])


def gpu_render(pkg, d):
    scene = pkg.load_dict(d)
    sensor = scene.sensors()[0]
    assert scene.integrator().render(scene, sensor, collect_counters=True)
    st = scene.integrator().last_stats
    assert not st.get("cancelled", 0), "the GPU render hit the integrator's timeout"
    return np.array(sensor.film().bitmap(raw=True)), (st["n_iter"], st["n_lookup"], st["n_nee_step"])


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("case", CASES)
def test_edge_media_terminate_on_the_oracle(case, integrator):
    """CPU: every edge scene finishes on the oracle within the wall-clock bound and renders something finite."""
    ref, counters = bounded_oracle(edge_scene(case, integrator))
    assert np.isfinite(ref).all() and ref[..., 4].min() > 0 and counters[0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("case", CASES)
def test_edge_media_match_the_oracle(gpu_rgb, monkeypatch, case, integrator):
    d = edge_scene(case, integrator)
    ref, counters = bounded_oracle(d)
    for lean in (None, "0"):
        if lean is None:
            monkeypatch.delenv("MTSAMD_LEAN", raising=False)
        else:
            monkeypatch.setenv("MTSAMD_LEAN", lean)
        gpu, c = gpu_render(gpu_rgb, d)
        assert np.array_equal(gpu, ref), (case, integrator, lean, float(np.abs(gpu - ref).max()), int((gpu != ref).sum()))
        assert c == counters, (case, integrator, lean, c, counters)
    monkeypatch.delenv("MTSAMD_LEAN", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed_trilinear", "all_ones_max"])
def test_edge_media_match_the_oracle_in_gpu_mono(gpu_rgb, case):
    d = edge_scene(case, "volpathmis" if case == "all_ones_max" else "volpath")
    ref, counters = bounded_oracle(d, mono=True)
    gpu_rgb.set_variant("gpu_mono")
    try:
        gpu, c = gpu_render(gpu_rgb, d)
    finally:
        gpu_rgb.set_variant("gpu_rgb")
    assert np.array_equal(gpu, ref) and c == counters, (case, float(np.abs(gpu - ref).max()), c, counters)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mixed_nearest", "exp67"])
def test_edge_media_match_the_oracle_in_gpu_spectral(gpu_rgb, case):
    d = edge_scene(case, "volpath")
    d["ground"] = dict(d["ground"], bsdf={"type": "diffuse", "reflectance": {"type": "uniform", "value": 0.5}})   # no rgb in spectral
    ref, counters = bounded_oracle(d, spectral=True)
    gpu_rgb.set_variant("gpu_spectral")
    try:
        gpu, c = gpu_render(gpu_rgb, d)
    finally:
        gpu_rgb.set_variant("gpu_rgb")
    assert np.array_equal(gpu, ref) and c == counters, (case, float(np.abs(gpu - ref).max()), c, counters)
