"""Timing-only probe of several sensors on one upload (diagnostic): the C3 scene (128^3 grids) seen by N
perspective sensors at 16 spp.  Reports the wall time of N x (load_dict + render) of single-sensor scenes, of one load_dict + N renders,
and the summed kernel time of both, which must agree: the kernels are the same.  No threshold is asserted.
usage: gpu_sensors_time.py [N] [SIZE] [REPEATS]     (N sensors on a ring around the slab, SIZE x SIZE films; 8, 256, 3)"""
import importlib, math, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("eradiate-kernel_amd"); scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f
pkg.set_variant("gpu_rgb")
count = int(sys.argv[1]) if len(sys.argv) > 1 else 8
size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
spp = 16
base = scenes.c3_heterogeneous(size, size, spp, res=128)
camera = base.pop("sensor")


def sensor(k):
    a = 2.0 * math.pi * k / count
    return dict(camera, to_world=T.look_at([12.0 * math.cos(a), 12.0 * math.sin(a), 16.0], [0, 0, 0], [0, 0, 1]),
                sampler={"type": "independent", "sample_count": spp, "seed": k})


def wall(f):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = f(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def one_by_one():
    kernel = 0.0
    for k in range(count):
        scene = pkg.load_dict(dict(base, sensor=sensor(k)))
        scene.integrator().render(scene, scene.sensors()[0]); kernel += scene.integrator().last_stats["kernel_ms"]
        scene.destroy()
    return kernel


def one_upload():
    scene = pkg.load_dict(dict(base, **{"sensor_%d" % k: sensor(k) for k in range(count)}))
    kernel = 0.0
    for s in scene.sensors():
        scene.integrator().render(scene, s); kernel += scene.integrator().last_stats["kernel_ms"]
    scene.destroy()
    return kernel


warm = pkg.load_dict(dict(base, sensor=sensor(0))); warm.integrator().render(warm, warm.sensors()[0]); warm.destroy()       # the context, the code objects
for rep in range(repeats):
    (wa, ka), (wb, kb) = wall(one_by_one), wall(one_upload)
    print("%s C3 128^3, %d sensors %dx%dx%d, rep %d: %d x (load_dict + render) %.1f ms wall, kernels %.2f ms | one load_dict + %d renders %.1f ms wall, kernels %.2f ms | saved %.1f ms (%.1f %%)"
          % (os.environ.get("TAG", ""), count, size, size, spp, rep, count, wa, ka, count, wb, kb, wa - wb, 100.0 * (wa - wb) / wa), flush=True)
