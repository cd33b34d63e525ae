"""mts_scene_update on the device (run with -m gpu on an MI355X): a scene updated in place is the scene a fresh load builds -- same
film (the oracle's, bit for bit with the fresh load's), same kernel, same device contents (mts_debug_scene_digest) -- for grids given
as host arrays and as device tensors, at the grid shapes where the fused reduction / pair-grid pass can go wrong, and a refused update
leaves the scene alone.  And without a render: the uploaded copy of a fresh scene is the host scene, word for word of the digest."""
import copy
import ctypes as C
import importlib
import threading
import time

import numpy as np
import pytest

import tests.oracle_binding as ob
from tests import sensor_cases, update_cases

pytestmark = pytest.mark.gpu
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")


@pytest.fixture(params=["gpu_rgb", "gpu_mono"])
def variant(request, gpu_rgb):
    gpu_rgb.set_variant(request.param)
    yield gpu_rgb, request.param == "gpu_mono"
    gpu_rgb.set_variant("gpu_rgb")


def digest(scene):
    out = (C.c_uint64 * 8)()
    A.check(A.lib().mts_debug_scene_digest(scene._handle, out))
    return list(out)


def render(scene):
    sensor = scene.sensors()[0]
    assert scene.integrator().render(scene, sensor)
    return np.array(sensor.film().bitmap(raw=True)), scene.integrator().last_stats["kernel_variant"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_is_fresh(pkg, scene, d, ref=None):
    """`scene`, updated, against a fresh load of the dictionary it was updated to: film, kernel, device contents; and the oracle's film."""
    film, kernel = render(scene)
    fresh = pkg.load_dict(d)
    fresh_film, fresh_kernel = render(fresh)
    assert digest(scene) == digest(fresh)
    assert kernel == fresh_kernel
    assert np.array_equal(bits(film), bits(fresh_film))
    if ref is not None:
        mism = int(np.sum(bits(film) != bits(ref)))
        print("film values differing from the oracle's: %d of %d" % (mism, film.size))
        assert np.array_equal(bits(film), bits(ref))
    return film


def assign(params, sets, device=False):
    import torch
    for k, v in sets.items():
        params[k] = torch.from_numpy(np.array(v, np.float32)).cuda() if (device and k.endswith(".data")) else v
    params.update()


# ---------------------------------------------------------------- scenes A / B
def slab(sigma_t, albedo, width=16, height=16, spp=8, integrator="volpath", **grid):
    d = scenes.c3_heterogeneous(width, height, spp, res=8)
    xf = d["slab"]["interior"]["sigma_t"]["to_world"]
    med = d["slab"]["interior"]
    med["sigma_t"] = dict({"type": "gridvolume", "data": sigma_t, "to_world": xf}, **grid)
    med["albedo"] = dict({"type": "gridvolume", "data": albedo, "to_world": xf}, **grid) if isinstance(albedo, np.ndarray) else albedo
    d["integrator"]["type"] = integrator
    return d


def case_c3():
    a = scenes.c3_heterogeneous(32, 32, 16, res=16)
    sig = scenes.c3_sigma_t_grid(16, seed=99) * np.float32(1.5)
    alb = (0.5 + 0.4 * np.random.default_rng(3).random((16, 16, 16), dtype=np.float32)).astype(np.float32)
    b = copy.deepcopy(a)
    med = b["slab"]["interior"]
    med["sigma_t"]["data"], med["albedo"]["data"], med["scale"], med["phase"]["g"] = sig, alb, 0.6, -0.35
    b["ground"]["bsdf"]["reflectance"] = {"type": "rgb", "value": [0.9, 0.3, 0.1]}
    b["sun"]["irradiance"] = 2.5
    pre = "slab.interior_medium."
    sets_b = {pre + "sigma_t.data": sig, pre + "albedo.data": alb, pre + "scale": 0.6, pre + "phase_function.g": -0.35,
              "ground.bsdf.reflectance.value": {"type": "rgb", "value": [0.9, 0.3, 0.1]}, "sun.irradiance.value": 2.5}
    ma = a["slab"]["interior"]
    sets_a = {pre + "sigma_t.data": ma["sigma_t"]["data"], pre + "albedo.data": ma["albedo"]["data"], pre + "scale": 1.0, pre + "phase_function.g": 0.8,
              "ground.bsdf.reflectance.value": {"type": "rgb", "value": [0.5, 0.5, 0.5]}, "sun.irradiance.value": 1.0}
    return a, b, sets_a, sets_b


def case_c4(columns=2):
    a = scenes.c4_atmosphere(16, 16, 16, layers=8, columns=columns)
    b = copy.deepcopy(a)
    med = b["atmosphere"]["interior"]
    shape = med["sigma_t"]["data"].shape
    sig = (med["sigma_t"]["data"] * (0.5 + np.random.default_rng(7).random(shape[0], dtype=np.float32))[:, None, None]).astype(np.float32)
    alb = np.ascontiguousarray(np.broadcast_to(np.linspace(0.95, 0.6, shape[0], dtype=np.float32)[:, None, None], shape))
    med["sigma_t"]["data"], med["albedo"]["data"], med["scale"] = sig, alb, 1.75
    med["phase"]["phase_1"]["values"] = scenes.hg_table(0.55)
    b["ground"]["bsdf"].update(rho_0=0.2, k=0.8, g=-0.1)
    b["sun"]["irradiance"] = {"type": "rgb", "value": [2.0, 1.5, 0.5]}
    pre = "atmosphere.interior_medium."
    sets_b = {pre + "sigma_t.data": sig, pre + "albedo.data": alb, pre + "scale": 1.75, pre + "phase_function.phase_1.values": scenes.hg_table(0.55),
              "ground.bsdf.rho_0.value": 0.2, "ground.bsdf.k.value": 0.8, "ground.bsdf.g.value": -0.1, "sun.irradiance.value": {"type": "rgb", "value": [2.0, 1.5, 0.5]}}
    ma = a["atmosphere"]["interior"]
    sets_a = {pre + "sigma_t.data": ma["sigma_t"]["data"], pre + "albedo.data": ma["albedo"]["data"], pre + "scale": 1.0,
              pre + "phase_function.phase_1.values": scenes.hg_table(0.7), "ground.bsdf.rho_0.value": 0.1, "ground.bsdf.k.value": 0.6,
              "ground.bsdf.g.value": -0.2, "sun.irradiance.value": 1.0}
    return a, b, sets_a, sets_b


def case_rgb_grid():
    """a 3-channel nearest-filter grid of 5 x 3 x 7 voxels: no pair grid, odd sizes"""
    rng = np.random.default_rng(11)
    sa = (0.2 + rng.random((7, 3, 5, 3), dtype=np.float32)).astype(np.float32)
    sb = (0.1 + 2.0 * rng.random((7, 3, 5, 3), dtype=np.float32)).astype(np.float32)
    a = slab(sa, 0.8, filter_type="nearest")
    b = slab(sb, 0.8, filter_type="nearest")
    key = "slab.interior_medium.sigma_t.data"
    return a, b, {key: sa}, {key: sb}


CASES = {"c3": case_c3, "c4": case_c4, "c4_one_column": lambda: case_c4(columns=1), "rgb_grid_5x3x7": case_rgb_grid}


@pytest.mark.parametrize("integrator", ["volpath", "volpathmis"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_film_and_digest(variant, case, integrator):
    pkg, mono = variant
    a, b, sets_a, sets_b = CASES[case]()
    a["integrator"]["type"] = b["integrator"]["type"] = integrator
    ref_a, ref_b = ob.OracleScene(a, mono=mono).render(), ob.OracleScene(b, mono=mono).render()
    scene = pkg.load_dict(a)
    film_a, _ = render(scene)
    digest_a = digest(scene)
    params = pkg.traverse(scene)
    for device in (False, True):                                 # the grids as host arrays, then as device tensors
        if device and mono and case == "rgb_grid_5x3x7":
            # under *_mono the description holds the colour grid's luminance with the COLOUR grid's maximum as its majorant
            # (grid3d.cpp:157-160): a device tensor cannot carry that maximum, so it is refused -- and nothing has changed
            import torch
            for wrong in (torch.from_numpy(sets_b["slab.interior_medium.sigma_t.data"]).cuda(), torch.zeros((7, 3, 5, 1), device="cuda")):
                params["slab.interior_medium.sigma_t.data"] = wrong
                with pytest.raises(RuntimeError, match="a device tensor cannot update a colour grid under gpu_mono"):
                    params.update()
                assert digest(scene) == digest_a
                assert np.array_equal(bits(render(scene)[0]), bits(film_a))
            continue
        assign(params, sets_b, device)
        film_b = assert_is_fresh(pkg, scene, b, ref_b)
        assert not np.array_equal(film_b, film_a)
        assign(params, sets_a, device)
        assert digest(scene) == digest_a
        assert np.array_equal(bits(assert_is_fresh(pkg, scene, a, ref_a)), bits(film_a))


@pytest.mark.parametrize("which", ["sigma_t", "albedo"])
@pytest.mark.parametrize("columns", [1, 2])
def test_one_grid_of_a_pair(gpu_rgb, which, columns):
    """Only one of the two grids of a pair grid is dirty: the other half of every voxel comes from the scene's own device copy."""
    a, b, sets_a, sets_b = case_c4(columns)
    key = "atmosphere.interior_medium.%s.data" % which
    half = copy.deepcopy(a)
    half["atmosphere"]["interior"][which]["data"] = b["atmosphere"]["interior"][which]["data"]
    for device in (False, True):
        scene = gpu_rgb.load_dict(a)
        assign(gpu_rgb.traverse(scene), {key: sets_b[key]}, device)
        assert_is_fresh(gpu_rgb, scene, half, ob.OracleScene(half).render())


# ---------------------------------------------------------------- the reduction at the shapes where it can go wrong
SHAPES = {"2x2x2": (2, 2, 2, 1), "1x1x8": (8, 1, 1, 1), "3x5x7": (7, 5, 3, 1), "33x31x29": (29, 31, 33, 1), "17x16x16x3": (16, 16, 17, 3)}      # (nz, ny, nx, channels)


def profile(shape, seed):
    nz, ny, nx, ch = shape
    col = (0.2 + np.random.default_rng(seed).random((nz, 1, 1, ch), dtype=np.float32)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(col, shape))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reduction_shapes(gpu_rgb, shape):
    dims = SHAPES[shape]
    n = int(np.prod(dims))
    base = profile(dims, 1)
    albedo = profile(dims[:3] + (1,), 2) * np.float32(0.9) if dims[3] == 1 else 0.8      # single-channel grids sit on a pair grid
    a = slab(base, albedo, 8, 8, 4)
    scene = gpu_rgb.load_dict(a)
    params = gpu_rgb.traverse(scene)
    key = "slab.interior_medium.sigma_t.data"
    variants = {}
    for name, at in (("max_first", 0), ("max_last", n - 1), ("max_interior", n // 2 + 1)):
        g = (profile(dims, 5) * np.float32(0.5)).reshape(-1).copy()
        g[at] = np.float32(3.25)                                  # above every other value
        variants[name] = g.reshape(dims)
    variants["z_profile"] = profile(dims, 6)                     # all columns equal
    g = profile(dims, 6).copy()
    g[-1, -1, -1, -1] = np.float32(0.125)                        # the single voxel that breaks it: last column of the last slice (below the maximum)
    variants["profile_broken_at_the_end"] = g
    for device in (False, True):
        for name, g in variants.items():
            assign(params, {key: g}, device)
            b = slab(g, albedo, 8, 8, 4)
            assert_is_fresh(gpu_rgb, scene, b, ob.OracleScene(b).render())
    # the maximum alone, of data that is negative everywhere (no render: such a medium is no medium; the records carry the maximum)
    neg = -(profile(dims, 8) + np.float32(0.5))
    neg.reshape(-1)[n // 3] = np.float32(-0.015625)
    for device in (False, True):
        assign(params, {key: base}, device)
        assign(params, {key: neg}, device)
        fresh = gpu_rgb.load_dict(slab(neg, albedo, 8, 8, 4))
        assert digest(scene) == digest(fresh)


# ---------------------------------------------------------------- the kernel choice follows the update
def test_kernel_choice_follows_the_update(gpu_rgb):
    a = scenes.c4_atmosphere(16, 16, 16, layers=8)
    x = copy.deepcopy(a)
    g = x["atmosphere"]["interior"]["sigma_t"]["data"].copy()
    g[:, 1, 1] *= np.float32(1.5)                               # varies with x and y: no z profile any more
    x["atmosphere"]["interior"]["sigma_t"]["data"] = g
    key = "atmosphere.interior_medium.sigma_t.data"
    scene = gpu_rgb.load_dict(a)
    params = gpu_rgb.traverse(scene)
    digest_a = digest(scene)
    for device in (False, True):
        assign(params, {key: g}, device)
        assert digest(scene) != digest_a
        assert_is_fresh(gpu_rgb, scene, x, ob.OracleScene(x).render())
        assign(params, {key: a["atmosphere"]["interior"]["sigma_t"]["data"]}, device)
        assert digest(scene) == digest_a
        assert_is_fresh(gpu_rgb, scene, a, ob.OracleScene(a).render())


def test_grey_constvolume_becomes_coloured(gpu_rgb):
    """A homogeneous slab whose albedo stops being grey leaves the grey fast path (DMedium::grey) and comes back to it."""
    grey = scenes.c2_homogeneous_slab(24, 24, 16)
    col = copy.deepcopy(grey)
    col["slab"]["interior"]["albedo"] = {"type": "rgb", "value": [0.9, 0.5, 0.2]}
    scene = gpu_rgb.load_dict(grey)
    params = gpu_rgb.traverse(scene)
    digest_grey = digest(scene)
    params["slab.interior_medium.albedo.color.value"] = {"type": "rgb", "value": [0.9, 0.5, 0.2]}
    params.update()
    film = assert_is_fresh(gpu_rgb, scene, col, ob.OracleScene(col).render())
    assert not np.allclose(film[..., 0], film[..., 2])
    params["slab.interior_medium.albedo.color.value"] = 0.8
    params.update()
    assert digest(scene) == digest_grey
    assert_is_fresh(gpu_rgb, scene, grey, ob.OracleScene(grey).render())


# ---------------------------------------------------------------- spectral variant
def test_spectral_update(gpu_rgb):
    a, b, sets = update_cases.spectral_edit()
    gpu_rgb.set_variant("gpu_spectral")
    try:
        ref = ob.OracleScene(b, spectral=True).render()
        for device in (False, True):
            scene = gpu_rgb.load_dict(a)
            assign(gpu_rgb.traverse(scene), sets, device)
            assert_is_fresh(gpu_rgb, scene, b, ref)
    finally:
        gpu_rgb.set_variant("gpu_rgb")


# ---------------------------------------------------------------- errors
def test_refused_updates_leave_the_scene_intact(gpu_rgb):
    import torch
    a, b, sets_a, sets_b = case_c3()
    scene = gpu_rgb.load_dict(a)
    film_a, _ = render(scene)
    digest_a = digest(scene)
    params = gpu_rgb.traverse(scene)
    pre = "slab.interior_medium."
    good = torch.from_numpy(sets_b[pre + "albedo.data"]).cuda()
    bad = [(pre + "sigma_t.data", torch.zeros(16 * 16 * 15, device="cuda"), "the grid holds"),
           (pre + "sigma_t.data", torch.zeros((16, 16, 16), dtype=torch.float64, device="cuda"), "float32"),
           (pre + "sigma_t.data", torch.zeros((16, 16, 32), device="cuda")[:, :, ::2], "contiguous"),
           (pre + "sigma_t.data", np.zeros((16, 16, 8), np.float32), "'size' / 'channels' cannot change"),
           (pre + "phase_function.g", 1.0, "'g'")]
    for key, value, expect in bad:
        params[pre + "albedo.data"] = good                       # valid assignments of the same update are not applied either
        params[pre + "scale"] = 0.25
        params[key] = value
        with pytest.raises(RuntimeError, match=expect):
            params.update()
        assert digest(scene) == digest_a
        assert np.array_equal(bits(render(scene)[0]), bits(film_a))
    # ... and the scene still takes an update
    assign(params, sets_b, True)
    assert_is_fresh(gpu_rgb, scene, b)


def test_update_while_a_render_runs_and_after_destroy(gpu_rgb):
    d = scenes.c3_heterogeneous(512, 512, 8192)                  # about four seconds of kernel time (test_cancel_and_timeout's scene)
    scene = gpu_rgb.load_dict(d)
    integ, sensor = scene.integrator(), scene.sensors()[0]
    params = gpu_rgb.traverse(scene)
    result = {}
    th = threading.Thread(target=lambda: result.update(ok=integ.render(scene, sensor)))
    th.start()
    time.sleep(0.3)
    params["slab.interior_medium.scale"] = 2.0
    try:
        with pytest.raises(RuntimeError, match="a render of this scene is in flight"):
            params.update()
    finally:
        integ.cancel()
        th.join(30)
    assert not th.is_alive() and result["ok"] is False
    assert scene._desc.media[0].scale == 1.0                     # the refused update was rolled back
    params["slab.interior_medium.scale"] = 2.0
    params.update()                                              # the render is over: accepted
    scene.destroy()
    params["slab.interior_medium.scale"] = 3.0
    with pytest.raises(RuntimeError, match="the scene was destroyed"):
        params.update()


def test_description_after_a_device_update(gpu_rgb):
    """A grid that came from a device tensor: the description points at no host array any more (nothing can upload a stale one), the map
    reads the tensor back, set_dirty() sends it again, and a host array puts the pointer back."""
    import torch
    a, b, sets_a, sets_b = case_c3()
    key = "slab.interior_medium.sigma_t.data"
    scene = gpu_rgb.load_dict(a)
    params = gpu_rgb.traverse(scene)
    vol = scene._desc.volumes[scene._desc.media[0].sigma_t_volume]
    t = torch.from_numpy(sets_b[key]).cuda()
    params[key] = t
    params.update()
    assert not vol.data and params[key] is t
    want = digest(scene)
    raw = (A.Dirty * 1)()
    raw[0].object, raw[0].index = A.OBJ_VOLUME, scene._desc.media[0].sigma_t_volume
    assert A.lib().mts_scene_update(scene._handle, C.byref(scene._desc), raw, 1, None) != 0 and b"missing data" in A.lib().mts_last_error()
    assert digest(scene) == want
    with pytest.raises(RuntimeError, match="missing data"):
        ob.OracleScene(desc=scene._desc, keep=scene._keep)
    t.mul_(0.5)                                                  # changed in place by its producer
    params.set_dirty(key)
    params.update()
    half = copy.deepcopy(a)
    half["slab"]["interior"]["sigma_t"]["data"] = sets_b[key] * np.float32(0.5)
    assert_is_fresh(gpu_rgb, scene, half, ob.OracleScene(half).render())
    params[key] = sets_b[key]
    params.update()
    assert bool(vol.data)
    half["slab"]["interior"]["sigma_t"]["data"] = sets_b[key]
    assert_is_fresh(gpu_rgb, scene, half, ob.OracleScene(half).render())


# ---------------------------------------------------------------- the uploaded copy is the host scene
@pytest.mark.parametrize("case", sensor_cases.UPLOAD_CASES)
def test_uploaded_scene_is_the_host_scene(gpu_rgb, case):
    """upload_host_scene and the two modes of the digest walk (device memory, the host's own arrays) against each other: all eight slots.
    No render is launched."""
    builder, kw = sensor_cases.CASES[case]
    gpu_rgb.set_variant("gpu_spectral" if kw.get("spectral") else "gpu_rgb")
    try:
        scene = gpu_rgb.load_dict(builder())
        host = (C.c_uint64 * 8)()
        A.check(A.lib().mts_debug_desc_digest(C.byref(scene._desc), host))
        assert digest(scene) == list(host)
    finally:
        gpu_rgb.set_variant("gpu_rgb")
