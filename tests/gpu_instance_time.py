"""Timing-only probe of instanced geometry (diagnostic): a grove of K instances of one mesh group over a diffuse
ground under a directional sun, `path`, and the same grove expanded into K plain meshes (every vertex carried through the instance's
transform on the host).  Reports, for both, the free device memory load_dict consumed and the rate of the render.
usage: gpu_instance_time.py [K] [CELLS] [REPEATS]     (K instances of a CELLS x CELLS grid of two-triangle cells; 256, 32, 3)"""
import importlib, sys, os
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("eradiate-kernel_amd"); scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f
pkg.set_variant("gpu_rgb")
count = int(sys.argv[1]) if len(sys.argv) > 1 else 256
cells = int(sys.argv[2]) if len(sys.argv) > 2 else 32
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
w, h, spp = 256, 256, 16
g = np.linspace(-0.5, 0.5, cells + 1)
x, y = np.meshgrid(g, g)
pos = np.c_[x.ravel(), y.ravel(), (0.2 * np.sin(6 * x) * np.cos(5 * y)).ravel()].astype(np.float32)
faces = np.array([f for j in range(cells) for i in range(cells) for f in ([j * (cells + 1) + i, j * (cells + 1) + i + 1, (j + 1) * (cells + 1) + i + 1],
                                                                            [j * (cells + 1) + i, (j + 1) * (cells + 1) + i + 1, (j + 1) * (cells + 1) + i])], np.uint32)
rng = np.random.default_rng(7)
side = int(np.ceil(np.sqrt(count)))
places = [T.translate([-8 + 16 * ((k % side) + 0.5) / side, -8 + 16 * ((k // side) + 0.5) / side, float(rng.uniform(0.5, 2.5))])
          @ T.rotate(rng.normal(size=3).tolist(), float(rng.uniform(0, 360))) @ T.scale([float(rng.uniform(0.8, 1.6)), float(rng.uniform(0.8, 1.6)), 1.0]) for k in range(count)]
leaf = {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.6, 0.1]}}


def base():
    return {"type": "scene", "integrator": {"type": "path", "max_depth": 6},
            "sensor": {"type": "perspective", "to_world": T.look_at([0, -22, 14], [0, 0, 1], [0, 0, 1]), "fov": 40.0,
                       "film": {"type": "hdrfilm", "width": w, "height": h, "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": spp}},
            "ground": {"type": "rectangle", "to_world": T.scale(12.0), "bsdf": {"type": "diffuse", "reflectance": 0.4}},
            "sun": {"type": "directional", "direction": [0.3, 0.2, -1.0], "irradiance": 3.0}}


def instanced():
    d = base()
    d["a_group"] = {"type": "shapegroup", "id": "tree", "mesh": {"type": "mesh", "vertex_positions": pos, "faces": faces, "bsdf": leaf}}
    for k, xf in enumerate(places):
        d["tree_%04d" % k] = {"type": "instance", "to_world": xf, "group": {"type": "ref", "id": "tree"}}
    return d


def expanded():
    d = base()
    for k, xf in enumerate(places):
        m = np.asarray(xf.matrix, np.float64).reshape(4, 4)
        d["tree_%04d" % k] = {"type": "mesh", "vertex_positions": (pos.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32), "faces": faces, "bsdf": leaf}
    return d


warm = pkg.load_dict(base()); warm.integrator().render(warm, warm.sensors()[0])       # the context, the code objects, the library's buffers
for name, build in (("instanced", instanced), ("expanded", expanded)):
    torch.cuda.synchronize(); free = torch.cuda.mem_get_info()[0]
    scene = pkg.load_dict(build()); sensor = scene.sensors()[0]
    torch.cuda.synchronize(); used = free - torch.cuda.mem_get_info()[0]
    scene.integrator().render(scene, sensor)                                          # warm-up
    for rep in range(repeats):
        scene.integrator().render(scene, sensor); st = scene.integrator().last_stats
        print("%s grove %s: %d x %d triangles, load %.1f MB of device memory, %dx%dx%d rep %d: kernel %.2f ms -> %.1f Msamples/s (row %d, textured %d)"
              % (os.environ.get("TAG", ""), name, count, len(faces), used / 2 ** 20, w, h, spp, rep, st["kernel_ms"], st["samples"] / st["kernel_ms"] / 1e3,
                 st["kernel_variant"], st["textured"]), flush=True)
    del scene, sensor
