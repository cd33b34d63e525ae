"""Eradiate's `moment` integrator (src/integrators/moment.cpp) on the GPU: the 11-channel film X, Y, Z, A, W, m1.XYZ, m2.XYZ.

Every expected value comes from PLAIN (non-moment) renders of the CPU restatement (tests/oracle_binding.OracleScene).  With a perspective
sensor the ray weight is exactly 1, so the 1-spp film of a plain render IS the per-sample raw XYZ; and a render of P passes of one
sample equals the fold, in pass order, of P plain 1-spp renders whose sampler seeds are shifted by whole passes: a pixel's stream is
seeded with seed + block_id * 1024 + i, and the spiral numbers the blocks of the FIRST pass highest (render_plan.h: Spiral::next_block).
So every channel of a multi-pass moment film has a bit-exact expectation; the single-pass films are pinned through channels 0-4 (the
plain film), channels 5-7 (bitwise the first three) and the Cauchy-Schwarz bound on the second moment."""
import importlib

import numpy as np
import pytest

import tests.oracle_binding as ob
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu
scenes = importlib.import_module("eradiate-kernel_amd.scenes")

SEED = 7
# The single-pass checks need films whose every sample stayed in its own pixel and was kept (W == spp everywhere: asserted on the
# restatement's plain films).  px + u rounds up to the next pixel about once in 10^5 samples, so among the eight 16-spp films of the
# four cases (scalar and wavefront streams) some pixel is hit under most seeds -- under seed 7 in (b); 97 is the first seed from 4 on
# under which none is.
SEED16 = 97
CASES = ("volpath", "volpathmis", "path", "volpath_mono")
RING_VOLPATH, RING_MIS, FLAT, NESTED = 11024, 10512, 1, 0          # mts_stats.kernel_variant, general unit


def plain_scene(case, spp, rfilter="box", seed=SEED):
    """The nested integrator's scene: (a) volpath / (b) volpathmis on the c3 miniature at 72 x 40 (partial 32 x 32 blocks, six of them),
    (c) path on the cornell box at 48 x 40, (d) = (a) in gpu_mono."""
    if case == "path":
        d = scenes.c1_cornell(48, 40, spp)
    else:
        d = scenes.c3_heterogeneous(72, 40, spp, res=16)
        if case == "volpathmis":
            d["integrator"] = dict(d["integrator"], type="volpathmis")
    d["sensor"]["sampler"]["seed"] = seed
    d["sensor"]["film"]["rfilter"] = {"type": rfilter}
    return d


def wrap(d, **outer):
    """`d` with its integrator inside a moment wrapper (the wrapper's block size is the render's)."""
    return dict(d, integrator=dict({"type": "moment", "block_size": d["integrator"]["block_size"], "li": dict(d["integrator"])}, **outer))


def is_mono(case):
    return case.endswith("mono")


_ORACLE = {}


def oracle_film(case, spp, seed=SEED, wavefront=False):
    """Plain render of the CPU restatement, computed once per module; returns (film, stats).  Read-only."""
    key = (case, spp, seed, wavefront)
    if key not in _ORACLE:
        d = plain_scene(case, spp, seed=seed)
        if wavefront:
            d["sensor"]["sampler"]["wavefront"] = True
        o = ob.OracleScene(d, mono=is_mono(case))
        film = o.render(); film.setflags(write=False)
        _ORACLE[key] = (film, dict(o.last_stats))
    return _ORACLE[key]


def moment_render(pkg, case, d, **kw):
    pkg.set_variant("gpu_mono" if is_mono(case) else "gpu_rgb")
    try:
        scene = pkg.load_dict(d)
        sensor = scene.sensors()[0]
        assert scene.integrator().render(scene, sensor, **kw)
        assert scene.integrator().aov_names() == ["li.X", "li.Y", "li.Z", "m2_li.X", "m2_li.Y", "m2_li.Z"]
        return np.array(sensor.film().bitmap(raw=True)), scene.integrator().last_stats, sensor
    finally:
        pkg.set_variant("gpu_rgb")


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_single_pass(raw, ref, spp):
    """Test 2 of the module: channels 0-4 the plain film's, 5-7 bitwise 0-2, the second moment within Cauchy-Schwarz."""
    assert raw.shape == ref.shape[:2] + (11,)
    assert np.all(ref[..., 4] == spp)                                  # precondition: no sample crossed a pixel edge
    assert same_bits(raw[..., :5], ref)
    assert same_bits(raw[..., 5:8], raw[..., :3])                      # ray weight 1, the same additions in the same order
    m1, m2, w = raw[..., 5:8].astype(np.float64), raw[..., 8:11].astype(np.float64), raw[..., 4:5].astype(np.float64)
    assert np.isfinite(raw).all() and (raw[..., 8:11] >= 0).all() and m2.max() > 0
    assert (w * m2 >= m1 * m1 * (1.0 - spp * 2.0 ** -23)).all()        # (sum x)^2 <= n sum x^2, with the rounding of `spp` fp32 additions


def expected_variant(case):
    return {"volpath": RING_VOLPATH, "volpath_mono": RING_VOLPATH, "volpathmis": RING_MIS, "path": FLAT}[case]


# ---------------------------------------------------------------------------------------------- 1: multi-pass, exact
@pytest.mark.parametrize("case", CASES)
def test_multi_pass_is_the_fold_of_plain_one_sample_renders(pkg, gpu_rgb, case):
    P = 3
    d = plain_scene(case, P)
    raw, st, _ = moment_render(pkg, case, wrap(d, samples_per_pass=1))
    w, h = d["sensor"]["film"]["width"], d["sensor"]["film"]["height"]
    B = ((w + 31) // 32) * ((h + 31) // 32)
    passes = [oracle_film(case, 1, seed=SEED + (P - 1 - p) * B * 32 * 32)[0] for p in range(P)]
    for R in passes:
        assert np.all(R[..., 4] == 1)                                  # precondition: every sample in its own pixel (and ray weight 1)
    exp = np.zeros((h, w, 11), np.float32)
    exp[..., :5] = passes[0]; exp[..., 5:8] = passes[0][..., :3]; exp[..., 8:11] = passes[0][..., :3] * passes[0][..., :3]
    for R in passes[1:]:                                               # fp32, in pass order
        exp[..., :5] += R; exp[..., 5:8] += R[..., :3]; exp[..., 8:11] += R[..., :3] * R[..., :3]
    assert raw.shape[2] == 11 and raw.dtype == np.float32
    assert same_bits(raw, exp), (np.argwhere(raw.view(np.uint32) != exp.view(np.uint32))[:5], st["kernel_variant"])
    assert exp[..., 8:11].max() > 0 and st["samples"] == w * h * P
    assert st["kernel_variant"] == expected_variant(case)


# ---------------------------------------------------------------------------------------------- 2 + 3: single pass, the kernels that ran
@pytest.mark.parametrize("case", CASES)
def test_single_pass(pkg, gpu_rgb, case):
    spp = 16
    raw, st, _ = moment_render(pkg, case, wrap(plain_scene(case, spp, seed=SEED16)))
    check_single_pass(raw, oracle_film(case, spp, seed=SEED16)[0], spp)
    assert st["kernel_variant"] == expected_variant(case)              # unit 0: the general kernels
    if case == "volpathmis":                                           # ... the variant the plain scene gets, lean unit aside
        pkg.set_variant("gpu_rgb")
        scene = pkg.load_dict(plain_scene(case, 1)); scene.integrator().render(scene, scene.sensors()[0])
        assert scene.integrator().last_stats["kernel_variant"] % 100000 == st["kernel_variant"]


@pytest.mark.parametrize("mode", ["nested", "counters", "wavefront"])
@pytest.mark.parametrize("case", CASES)
def test_nested_fallback(pkg, gpu_rgb, monkeypatch, case, mode):
    """Rows of the kernel table without a moment instantiation run the nested moment kernel: MTSAMD_KERNEL=nested, counters, wavefront streams."""
    spp = 16
    d = plain_scene(case, spp, seed=SEED16)
    kw = {}
    if mode == "nested":
        monkeypatch.setenv("MTSAMD_KERNEL", "nested")
    elif mode == "counters":
        kw["collect_counters"] = True
    else:
        d["sensor"]["sampler"]["wavefront"] = True
        monkeypatch.setenv("MTSAMD_WAVEFRONT_SPLIT", "1")             # one entry per block: the sums are taken in sample order
    ref, so = oracle_film(case, spp, seed=SEED16, wavefront=mode == "wavefront")
    raw, st, _ = moment_render(pkg, case, wrap(d), **kw)
    assert st["kernel_variant"] == NESTED
    check_single_pass(raw, ref, spp)
    if mode == "counters":
        assert (st["n_iter"], st["n_lookup"], st["n_nee_step"]) == (so["n_iter"], so["n_lookup"], so["n_nee_step"]) and st["n_iter"] > 0


# ---------------------------------------------------------------------------------------------- 4: before the ray weight
def test_moments_are_taken_before_the_ray_weight(pkg, gpu_rgb):
    """distantflux weighs its rays (distantflux.cpp); the first five channels carry the weight, the moments do not: moment.cpp:74-79."""
    d = scenes.c3_heterogeneous(8, 8, 1, res=16)
    d["sensor"] = {"type": "distantflux", "film": {"type": "hdrfilm", "width": 8, "height": 8, "rfilter": {"type": "box"}},
                   "sampler": {"type": "independent", "sample_count": 1, "seed": SEED}}
    raw, st, _ = moment_render(pkg, "volpath_mono", wrap(d))
    # each pixel's first two 2-D draws: film position, aperture sample (the sensor needs one); one 32 x 32 block, id 0, Morton order
    o = ob.OracleScene(d, mono=True)
    fs = np.zeros((8, 8, 2), np.float32); ap = np.zeros((8, 8, 2), np.float32)
    for y in range(8):
        for x in range(8):
            i = sum(((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1) for b in range(3))
            u = np.zeros(4, np.float32)
            ob.lib().oracle_sampler_stream(SEED, i, 4, u.ctypes.data_as(ob.fp))
            fs[y, x] = (np.float32(x) + u[0]) / np.float32(8), (np.float32(y) + u[1]) / np.float32(8)
            ap[y, x] = u[2], u[3]
    w = o.sensor_sample_ray(fs.reshape(-1, 2), ap.reshape(-1, 2))[2][:, 0].reshape(8, 8).astype(np.float32)
    assert (w != 1).any() and np.all(raw[..., 4] == 1) and raw[..., 5].max() > 0
    assert same_bits(raw[..., 0], w * raw[..., 5])
    assert same_bits(raw[..., 8], raw[..., 5] * raw[..., 5])
    assert same_bits(raw[..., :5], o.render())


# ---------------------------------------------------------------------------------------------- 5: wider filter
def test_gaussian_filter(pkg, gpu_rgb):
    """Every channel is splatted with the same filter weights.  Filtered splats are summed with float atomics (their order differs from
    the CPU block accumulation): the tolerance of tests/test_gpu_parity.py for such films, no bitwise fraction."""
    d = plain_scene("volpath", 4, rfilter="gaussian")
    raw, st, _ = moment_render(pkg, "volpath", wrap(d))
    ref = ob.OracleScene(d).render()
    assert raw.shape == (40, 72, 11)
    for got, want in ((raw[..., :5], ref), (raw[..., 5:8], raw[..., :3])):
        assert_parity(got, want, exact_fraction=0.0)
        assert np.allclose(got, want, rtol=2e-4, atol=1e-5)            # test_crop_window_and_gaussian_filter's
    assert (raw[..., 8:11] >= 0).all() and raw[..., 8:11].max() > 0


# ---------------------------------------------------------------------------------------------- 6: plumbing
def test_device_film_and_capacity(pkg, gpu_rgb):
    import torch
    d = wrap(plain_scene("volpath", 4))
    host, _, _ = moment_render(pkg, "volpath", d)
    scene = pkg.load_dict(d)
    sensor = scene.sensors()[0]
    h, w = 40, 72
    film = torch.full((h, w, 11), 7.0, dtype=torch.float32, device="cuda")         # stale content must be cleared
    assert scene.integrator().render(scene, sensor, device_film=film.data_ptr(), device_film_floats=h * w * 11)
    torch.cuda.synchronize()
    assert same_bits(film.cpu().numpy(), host)
    with pytest.raises(RuntimeError, match="11 channels"):
        scene.integrator().render(scene, sensor, device_film=film.data_ptr(), device_film_floats=h * w * 5)


def test_shards_sum_to_the_full_film(pkg, gpu_rgb):
    d = wrap(plain_scene("volpath", 4), samples_per_pass=2)
    full, st, _ = moment_render(pkg, "volpath", d)
    parts = [moment_render(pkg, "volpath", d, shard_index=i, shard_count=2) for i in range(2)]
    total = parts[0][0] + parts[1][0]
    assert sum(p[1]["samples"] for p in parts) == st["samples"] == 72 * 40 * 4
    assert same_bits(total[..., 3:5], full[..., 3:5]) and np.all(full[..., 4] == 4)
    assert np.allclose(total, full, rtol=1e-6, atol=0)


def test_bitmap_develops_the_aov_channels(pkg, gpu_rgb):
    raw, _, sensor = moment_render(pkg, "path", wrap(plain_scene("path", 4)))
    dev = np.array(sensor.film().bitmap())
    assert dev.shape == (40, 48, 4 + 6)
    assert same_bits(dev[..., 4:], (raw[..., 5:] / raw[..., 4:5]).astype(np.float32))
    plain = pkg.load_dict(plain_scene("path", 4)); ps = plain.sensors()[0]
    assert plain.integrator().render(plain, ps)
    assert same_bits(dev[..., :4], np.array(ps.film().bitmap()))


def test_crop_window(pkg, gpu_rgb):
    """Case (c) through a crop window with an offset: the plain render of the same window (the spiral, and with it every pixel's stream,
    follows the window) in channels 0-4, and the first moment bitwise next to it."""
    spp = 4
    d = plain_scene("path", spp)
    d["sensor"]["film"] = dict(d["sensor"]["film"], crop_offset_x=9, crop_offset_y=5, crop_width=35, crop_height=33)
    raw, st, _ = moment_render(pkg, "path", wrap(d))
    ref = ob.OracleScene(d).render()
    assert raw.shape == (33, 35, 11) and np.all(ref[..., 4] == spp)
    assert same_bits(raw[..., :5], ref) and same_bits(raw[..., 5:8], raw[..., :3])
    assert st["kernel_variant"] == FLAT
