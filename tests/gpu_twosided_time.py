"""Timing-only probe of a scene that uses the `twosided` adapter (diagnostic): ground b of tests/gpu_blend_time.py
-- blendbsdf(diffuse, rpv) under a 64x64 `nearest` weight bitmap, beneath the C4 atmosphere -- wrapped in a twosided.
usage: gpu_twosided_time.py [REPEATS]"""
import importlib, sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("eradiate-kernel_amd"); scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f
pkg.set_variant("gpu_rgb")
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
w, h, spp = 512, 512, 64                                                  # the size of tests/gpu_blend_time.py
d = scenes.c4_atmosphere(w, h, spp)
rng = np.random.default_rng(64)
to_uv = T.scale([37.0, 41.0, 1.0])
mask = (rng.random((64, 64), dtype=np.float32) > 0.5).astype(np.float32)
blend = {"type": "blendbsdf", "weight": {"type": "bitmap", "data": mask, "filter_type": "nearest", "to_uv": to_uv},
         "background": {"type": "diffuse", "reflectance": [0.35, 0.3, 0.2]}, "target": {"type": "rpv", "rho_0": 0.1, "k": 0.6, "g": -0.2}}
d["ground"]["bsdf"] = {"type": "twosided", "bsdf": blend}
scene = pkg.load_dict(d); sensor = scene.sensors()[0]
scene.integrator().render(scene, sensor)                                  # warm-up: code objects, the block calibration
for rep in range(repeats):
    scene.integrator().render(scene, sensor); st = scene.integrator().last_stats
    print("%s C4 ground twosided(b) %dx%dx%d rep %d: kernel %.2f ms -> %.1f Msamples/s (row %d, textured %d)"
          % (os.environ.get("TAG", ""), w, h, spp, rep, st["kernel_ms"], st["samples"] / st["kernel_ms"] / 1e3, st["kernel_variant"], st["textured"]), flush=True)
