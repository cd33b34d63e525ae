"""Timing-only probe of textured and blended grounds under the C4 atmosphere (diagnostic).
usage: gpu_blend_time.py GROUND [REPEATS]   GROUND: a = 64x64 bilinear bitmap reflectance (a diffuse ground: what the TEX kernels rendered
before blends), b = blendbsdf(diffuse, rpv) under a 64x64 `nearest` weight bitmap, c = the same blend under the constant weight 0.3."""
import importlib, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("eradiate-kernel_amd"); scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f
pkg.set_variant("gpu_rgb")
ground, repeats = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 5
w, h, spp = 512, 512, 64                                                  # the size of tests/gpu_canopy_ab.py
d = scenes.c4_atmosphere(w, h, spp)
rng = np.random.default_rng(64)
to_uv = T.scale([37.0, 41.0, 1.0])                                        # many texels across the footprint of the sensor's target
children = {"background": {"type": "diffuse", "reflectance": [0.35, 0.3, 0.2]}, "target": {"type": "rpv", "rho_0": 0.1, "k": 0.6, "g": -0.2}}
if ground == "a":
    d["ground"]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": rng.random((64, 64, 3), dtype=np.float32), "to_uv": to_uv}}
elif ground == "b":
    mask = (rng.random((64, 64), dtype=np.float32) > 0.5).astype(np.float32)
    d["ground"]["bsdf"] = dict({"type": "blendbsdf", "weight": {"type": "bitmap", "data": mask, "filter_type": "nearest", "to_uv": to_uv}}, **children)
elif ground == "c":
    d["ground"]["bsdf"] = dict({"type": "blendbsdf", "weight": 0.3}, **children)
else:
    sys.exit("GROUND must be a, b or c")
scene = pkg.load_dict(d); sensor = scene.sensors()[0]
scene.integrator().render(scene, sensor)                                  # warm-up: code objects, the block calibration
for rep in range(repeats):
    scene.integrator().render(scene, sensor); st = scene.integrator().last_stats
    print("%s C4 ground %s %dx%dx%d rep %d: kernel %.2f ms -> %.1f Msamples/s (row %d, textured %d)"
          % (os.environ.get("TAG", ""), ground, w, h, spp, rep, st["kernel_ms"], st["samples"] / st["kernel_ms"] / 1e3, st["kernel_variant"], st["textured"]), flush=True)
