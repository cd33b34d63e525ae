"""Several sensors on one uploaded scene (run with -m gpu on an MI355X).  The reference of every multi-sensor render is existing
behaviour: the film, kernel_variant and `textured` of a FRESH SINGLE-SENSOR scene built from the same dictionary with only that
sensor left in, and where the CPU restatement handles the scene, its film as well -- bit for bit (box filter), or within the
tolerance of tests/test_gpu_moment.py::test_gaussian_filter for the filtered film."""
import copy
import importlib

import numpy as np
import pytest

import tests.oracle_binding as ob
from tests import sensor_cases
from tests.independent import problems_instance
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")

SEED = 7


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def film(w, h, rfilter="box", **more):
    return dict({"type": "hdrfilm", "width": w, "height": h, "rfilter": {"type": rfilter}}, **more)


def sampler(spp, **more):
    return dict({"type": "independent", "sample_count": spp, "seed": SEED}, **more)


def six_sensors():
    """scenes.c3_heterogeneous(res=16) under `volpath` with S0 ... S5 of the module's specification; the keys sort in that order."""
    d = scenes.c3_heterogeneous(40, 24, 4, res=16)
    cam = d.pop("sensor")
    d["s0"] = dict(cam, film=film(40, 24), sampler=sampler(4))
    d["s1"] = dict(cam, film=film(72, 40, crop_offset_x=9, crop_offset_y=5, crop_width=35, crop_height=33), sampler=sampler(2))
    d["s2"] = {"type": "distant", "direction": [0.25, 0.0, 1.0], "ray_target": {"type": "sphere", "center": [0, 0, 1], "radius": 2.0},
               "film": film(16, 1), "sampler": sampler(4)}
    d["s3"] = {"type": "mdistant", "directions": "0, 0, -1, 0.5, 0, -1, 0, -0.5, -1, 0.3, 0.3, -1, -0.6, 0.1, -1", "target": [0.0, 0.0, 1.0],
               "film": film(5, 1), "sampler": sampler(4)}
    d["s4"] = {"type": "distantflux", "film": film(8, 8), "sampler": sampler(4)}
    d["s5"] = dict(cam, film=film(40, 24, rfilter="gaussian"), sampler=sampler(4))
    return d


KEYS = ["s0", "s1", "s2", "s3", "s4", "s5"]
SHAPES = [(24, 40), (33, 35), (1, 16), (1, 5), (8, 8), (24, 40)]


def sensor_keys(d):
    return [k for k, v in SD.sorted_items(d) if isinstance(v, dict) and v.get("type") in SD.SENSOR_PLUGINS]


def with_only(d, key):
    drop = set(sensor_keys(d)) - {key}
    return {k: v for k, v in d.items() if k not in drop}


def render(scene, k, **kw):
    sensor = scene.sensors()[k]
    assert scene.integrator().render(scene, sensor, **kw)
    st = scene.integrator().last_stats
    return np.array(sensor.film().bitmap(raw=True)), (st["kernel_variant"], st["textured"]), st


def lone_render(pkg, d, key, **kw):
    """the reference: a fresh scene with sensor `key` alone"""
    scene = pkg.load_dict(with_only(d, key))
    assert len(scene.sensors()) == 1
    return render(scene, 0, **kw)


_LONE = {}


def lone_six(pkg, k):
    """films of the six single-sensor scenes, computed once per module; read-only"""
    if k not in _LONE:
        f, kernel, st = lone_render(pkg, six_sensors(), KEYS[k])
        f.setflags(write=False)
        _LONE[k] = (f, kernel)
    return _LONE[k]


def assert_is_lone(pkg, d, variant="gpu_rgb", channels=5):
    """every sensor of `d` on one handle against its own single-sensor scene: film bits, kernel_variant, textured"""
    pkg.set_variant(variant)
    try:
        keys = sensor_keys(d)
        scene = pkg.load_dict(d)
        assert len(scene.sensors()) == len(keys) >= 2
        out = []
        for k, key in enumerate(keys):
            f, kernel, st = render(scene, k)
            g, lone_kernel, _ = lone_render(pkg, d, key)
            assert f.shape[2] == channels and np.isfinite(f).all() and f[..., 4].max() > 0, key
            assert kernel == lone_kernel, key
            assert same_bits(f, g), (key, int(np.sum(f.view(np.uint32) != g.view(np.uint32))))
            out.append((f, kernel, st))
        return out
    finally:
        pkg.set_variant("gpu_rgb")


# ---------------------------------------------------------------- 1: each sensor against its own scene
@pytest.mark.parametrize("k", range(6))
def test_each_sensor_against_its_own_scene(pkg, gpu_rgb, k):
    d = six_sensors()
    assert sensor_keys(d) == KEYS
    scene = pkg.load_dict(d)
    assert len(scene.sensors()) == 6
    f, kernel, st = render(scene, k)
    g, lone_kernel = lone_six(pkg, k)
    assert f.shape == SHAPES[k] + (5,) and kernel == lone_kernel
    assert f[..., :3].max() > 0                                      # the sensor does see the scene
    assert st["samples"] == SHAPES[k][0] * SHAPES[k][1] * (2 if k == 1 else 4)
    if k == 5:                                                       # filtered splats are summed with float atomics
        assert_parity(f, g, exact_fraction=0.0)
        assert np.allclose(f, g, rtol=2e-4, atol=1e-5)
        return
    assert same_bits(f, g), int(np.sum(f.view(np.uint32) != g.view(np.uint32)))
    ref = ob.OracleScene(with_only(d, KEYS[k])).render()
    assert same_bits(f, ref), int(np.sum(f.view(np.uint32) != ref.view(np.uint32)))


# ---------------------------------------------------------------- 2: order and reuse
def test_order_and_reuse(pkg, gpu_rgb):
    """3, 0, 3, 1, 0 on one handle: cache buffers regrown between film sizes and the per-sensor tables survive"""
    scene = pkg.load_dict(six_sensors())
    first = {}
    for k in (3, 0, 3, 1, 0):
        f, kernel, _ = render(scene, k)
        if k not in first:
            first[k] = (f, kernel)
            assert same_bits(f, lone_six(pkg, k)[0]) and kernel == lone_six(pkg, k)[1]
        else:
            assert same_bits(f, first[k][0]) and kernel == first[k][1], k


# ---------------------------------------------------------------- 3: the kernel choice is the sensor's, on the device
def test_per_sensor_kernel_choice(pkg, gpu_rgb):
    d = scenes.c1_cornell(48, 40, 4)
    d["sensor"]["sampler"]["seed"] = SEED
    d["z_distant"] = {"type": "distant", "direction": [0.0, -1.0, 0.2], "ray_target": {"type": "sphere", "center": [0, 0, 3.5], "radius": 1.5},
                      "film": film(16, 1), "sampler": sampler(4)}
    (_, lean, _), (_, general, _) = assert_is_lone(pkg, d)
    assert lean[0] >= 100000 and general[0] < 100000                  # the cornell box alone: a lean unit (compiled without spheres); the sphere target: never


# ---------------------------------------------------------------- 4: after an update
def test_after_an_update(pkg, gpu_rgb):
    from importlib import import_module
    traverse = import_module("eradiate-kernel_amd.params").traverse
    d = six_sensors()
    scene = pkg.load_dict(d)
    before = [render(scene, k)[0] for k in range(6)]
    sig = scenes.c3_sigma_t_grid(16, seed=99) * np.float32(1.5)
    rho = {"type": "rgb", "value": [0.9, 0.3, 0.1]}
    params = traverse(scene)
    params["slab.interior_medium.sigma_t.data"] = sig
    params["ground.bsdf.reflectance.value"] = rho
    params.update()
    e = copy.deepcopy(d)
    e["slab"]["interior"]["sigma_t"]["data"] = sig
    e["ground"]["bsdf"]["reflectance"] = rho
    for k in range(6):
        f, kernel, _ = render(scene, k)
        g, lone_kernel, _ = lone_render(pkg, e, KEYS[k])
        assert kernel == lone_kernel
        assert not same_bits(f, before[k]), k
        if k == 5:
            assert_parity(f, g, exact_fraction=0.0)
            assert np.allclose(f, g, rtol=2e-4, atol=1e-5)
        else:
            assert same_bits(f, g), (k, int(np.sum(f.view(np.uint32) != g.view(np.uint32))))


# ---------------------------------------------------------------- 5: other integrators and variants, two sensors per scene
def two_sensors(integrator=None):
    d = six_sensors()
    for key in ("s2", "s3", "s4", "s5"):
        del d[key]
    if integrator is not None:
        d["integrator"] = integrator(d["integrator"])
    return d


def test_volpathmis(pkg, gpu_rgb):
    assert_is_lone(pkg, two_sensors(lambda it: dict(it, type="volpathmis")))


def test_moment(pkg, gpu_rgb):
    d = two_sensors(lambda it: {"type": "moment", "block_size": it["block_size"], "li": dict(it)})
    for f, kernel, st in assert_is_lone(pkg, d, channels=11):
        assert same_bits(f[..., 5:8], f[..., :3])                     # a perspective's ray weight is 1


def test_mono(pkg, gpu_rgb):
    for f, kernel, st in assert_is_lone(pkg, two_sensors(), variant="gpu_mono"):
        assert same_bits(f[..., 0], f[..., 1]) and same_bits(f[..., 1], f[..., 2])


def test_spectral_bins_and_an_srf(pkg, gpu_rgb):
    d = sensor_cases.spectral(dict(sensor_cases.NBINS))
    d["sensor"]["film"] = film(12, 8); d["sensor"]["sampler"] = sampler(4)
    d["with_srf"] = dict(sensor_cases.CAMERA, srf=dict(sensor_cases.SRF_DISCRETE), film=film(9, 5), sampler=sampler(4))
    assert_is_lone(pkg, d, variant="gpu_spectral", channels=5 + 2 * 2)


def test_instanced(pkg, gpu_rgb):
    d = problems_instance.box_grove(16, 16)[0]
    keys = sensor_keys(d)
    assert len(keys) == 1
    second = copy.deepcopy(d[keys[0]])
    second["film"] = dict(second["film"], width=24, height=10)
    d["zz_second"] = second
    for f, kernel, st in assert_is_lone(pkg, d):
        assert kernel[1] == 2


def test_wavefront_beside_scalar(pkg, gpu_rgb, monkeypatch):
    monkeypatch.setenv("MTSAMD_WAVEFRONT_SPLIT", "1")                 # one entry per block: the sums are taken in sample order
    d = two_sensors()
    d["s1"] = dict(d["s1"], sampler=sampler(2, wavefront=True))
    (_, scalar, _), (_, wave, _) = assert_is_lone(pkg, d)
    assert scalar != wave


# ---------------------------------------------------------------- 6: plumbing
def test_device_film_of_sensor_1(pkg, gpu_rgb):
    import torch
    scene = pkg.load_dict(six_sensors())
    h, w = SHAPES[1]
    buf = torch.full((h, w, 5), 7.0, dtype=torch.float32, device="cuda")              # stale content must be cleared
    assert scene.integrator().render(scene, scene.sensors()[1], device_film=buf.data_ptr(), device_film_floats=h * w * 5)
    torch.cuda.synchronize()
    assert same_bits(buf.cpu().numpy(), lone_six(pkg, 1)[0])
    with pytest.raises(RuntimeError, match="this scene writes %d" % (h * w * 5)):      # sensor 1's size, not sensor 0's
        scene.integrator().render(scene, 1, device_film=buf.data_ptr(), device_film_floats=h * w * 5 - 1)
    assert scene.integrator().render(scene, 1, device_film=buf.data_ptr())             # the default capacity is that sensor's h x w x 5
    torch.cuda.synchronize()
    assert same_bits(buf.cpu().numpy(), lone_six(pkg, 1)[0])


def test_shards_of_sensor_1_sum_to_its_film(pkg, gpu_rgb):
    scene = pkg.load_dict(six_sensors())
    full, _, st = render(scene, 1)
    parts = [render(scene, 1, shard_index=i, shard_count=2) for i in range(2)]
    total = parts[0][0] + parts[1][0]
    assert sum(p[2]["samples"] for p in parts) == st["samples"] == 35 * 33 * 2
    assert all(0 < p[2]["samples"] < st["samples"] for p in parts)
    assert same_bits(total[..., 3:5], full[..., 3:5]) and np.all(full[..., 4] == 2)
    assert np.allclose(total, full, rtol=1e-6, atol=0)


def test_each_sensor_keeps_its_film(pkg, gpu_rgb):
    scene = pkg.load_dict(six_sensors())
    s0, s1 = scene.sensors()[0], scene.sensors()[1]
    with pytest.raises(RuntimeError, match="nothing has been rendered yet"):
        s1.film().bitmap()
    f0, _, _ = render(scene, 0)
    kept = s0.film().bitmap(raw=True)
    f1, _, _ = render(scene, 1)
    assert np.array(s0.film().bitmap(raw=True)).shape == (24, 40, 5) and same_bits(np.array(s0.film().bitmap(raw=True)), f0)
    assert np.array(kept) is not None and np.array(s1.film().bitmap(raw=True)).shape == (33, 35, 5)
    other = pkg.load_dict(with_only(six_sensors(), "s0"))
    with pytest.raises(RuntimeError, match="the sensor belongs to another scene"):
        scene.integrator().render(scene, other.sensors()[0])
    with pytest.raises(RuntimeError, match="out of range"):
        scene.integrator().render(scene, 6)


def test_a_dropped_scene_dies_with_its_last_reference(pkg, gpu_rgb):
    """Scene <-> Integrator must be no reference cycle: a scene left to the cyclic collector is freed whenever some thread happens to
    trigger a pass, and hipFree synchronises the device -- behind a running render of another scene that thread stalls until it ends."""
    import gc
    import weakref
    traverse = importlib.import_module("eradiate-kernel_amd.params").traverse
    gc.collect()
    gc.disable()
    try:
        scene = pkg.load_dict(six_sensors())
        params = traverse(scene)
        integ = scene.integrator()
        render(scene, 1)
        ref = weakref.ref(scene)
        del scene, params
        assert ref() is None                                          # no collector pass was needed
        with pytest.raises(RuntimeError, match="no longer exists"):
            integ.cancel()
    finally:
        gc.enable()
