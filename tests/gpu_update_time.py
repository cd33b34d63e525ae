"""Timing-only probe of the wavelength loop of the *_mono variants (diagnostic, not a test): bench.py's C5 job -- the C4 atmosphere
as monochromatic batches, Rayleigh extinction ~ lambda^-4 -- written the two ways a caller can write it.

    python tests/gpu_update_time.py WIDTH HEIGHT SPP LAYERS BATCHES [create|update] [columns=N]

  create          load_dict + render per batch: every batch builds, validates, allocates and uploads a whole scene
  update          one load_dict, then traverse() + update() + render per batch, with the new grids as host arrays ("update/host") and
                  as float32 tensors already on the device ("update/device")
`columns=N` makes the three grids LAYERS x N x N voxels (default 2: the plane-parallel atmosphere of bench.py).
Prints the wall time per batch of each way (after one batch of warm-up each).  `create` alone also runs on a tree without
traverse(), which is how the figures of the commit before it were taken (TAG names the tree in the output).
"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

columns = ([int(x[8:]) for x in sys.argv[6:] if x.startswith("columns=")] + [2])[0]
ways = [x for x in sys.argv[6:] if not x.startswith("columns=")] or ["create", "update"]
if "update" in ways:                                                         # torch opens the device first, as in bench.py and the test-suite
    import torch
    torch.cuda.init()
pkg = importlib.import_module("eradiate-kernel_amd")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
pkg.set_variant("gpu_mono")
w, h, spp, layers, batches = [int(x) for x in sys.argv[1:6]]
PRE = "atmosphere.interior_medium."


def scene_dict(k):
    return scenes.c4_atmosphere(w, h, spp, layers=layers, columns=columns, rayleigh_scale=(550.0 / (400.0 + 40.0 * (k % 16))) ** 4)


def grids(d):
    med = d["atmosphere"]["interior"]
    return {PRE + "sigma_t.data": med["sigma_t"]["data"], PRE + "albedo.data": med["albedo"]["data"],
            PRE + "phase_function.weight.data": med["phase"]["weight"]["data"]}


def render(scene):
    assert scene.integrator().render(scene, scene.sensors()[0])
    return scene.integrator().last_stats["kernel_ms"]


def report(name, wall, kernel, update=None):
    print("%s %-13s %dx%dx%d, grids %dx%dx%d: %.2f ms per batch (kernel %.2f ms, everything else %.2f ms%s)"
          % (os.environ.get("TAG", ""), name, w, h, spp, layers, columns, columns, 1e3 * wall / batches, kernel / batches, 1e3 * wall / batches - kernel / batches,
             "" if update is None else ", of which assignments + update() %.2f ms" % (1e3 * update / batches)), flush=True)


dicts = [scene_dict(k) for k in range(batches + 1)]                          # the inputs of the loop exist before it starts, in both ways
if "create" in ways:
    render(pkg.load_dict(dicts[0]))
    t0, kernel = time.perf_counter(), 0.0
    for d in dicts[1:]:
        kernel += render(pkg.load_dict(d))
    report("create", time.perf_counter() - t0, kernel)
if "update" in ways:
    for name in ("update/host", "update/device"):
        values = [grids(d) for d in dicts]
        if name == "update/device":
            values = [{k: torch.from_numpy(v).cuda() for k, v in g.items()} for g in values]
            torch.cuda.synchronize()
        scene = pkg.load_dict(dicts[0])
        params = pkg.traverse(scene)
        render(scene)
        for k, v in values[0].items():                                       # warm-up of the update path (first use allocates the scratch words)
            params[k] = v
        params.update()
        t0, kernel, update = time.perf_counter(), 0.0, 0.0
        for g in values[1:]:
            t1 = time.perf_counter()
            for k, v in g.items():
                params[k] = v
            params.update()
            update += time.perf_counter() - t1
            kernel += render(scene)
        report(name, time.perf_counter() - t0, kernel, update)
