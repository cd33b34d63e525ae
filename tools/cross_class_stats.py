"""Diagnostic: block statistics of the ring kernel with the null-boundary crossings told apart (needs a -DMTSAMD_BLOCKSTATS build).

    MTSAMD_LIB=<diagnostic library> python tools/cross_class_stats.py WIDTH HEIGHT SPP [C3|C4|C2]

Per class: executions per 64 pixels and sample, lanes per execution, lane-visits per sample, cycles per execution and the share of a
wave's cycles.  CROSS is the class of the main path's crossings of a null-BSDF boundary (a tree without the class leaves its row empty);
the last lines give the share of SURF's lane-visits that ARE such crossings, counted in the SURF block itself (g_blockstats[9]), and the
share of all crossings that the CROSS class carries."""
import ctypes as C
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("eradiate-kernel_amd")
A = importlib.import_module("eradiate-kernel_amd._capi")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")

NAMES = ["INT", "MED", "SCATTER", "WSURF", "SURF", "PHASE", "NEW", "MEDW", "CROSS"]


def main():
    w, h, spp = [int(x) for x in sys.argv[1:4]]
    cfg = sys.argv[4] if len(sys.argv) > 4 else "C3"
    pkg.set_variant("gpu_rgb")
    make = {"C3": scenes.c3_heterogeneous, "C4": scenes.c4_atmosphere, "C2": scenes.c2_homogeneous_slab}[cfg]
    scene = pkg.load_dict(make(w, h, spp))
    sensor = scene.sensors()[0]
    out = (C.c_ulonglong * 48)()
    read = A.lib().mts_debug_blockstats
    read(out, 1)
    scene.integrator().render(scene, sensor, collect_counters=True)
    st = scene.integrator().last_stats
    read(out, 0)
    waves = w * h / 64.0           # normalisation unit: one 64-pixel group
    total = sum(out[24:36]) + out[42] + out[43] + out[44]
    print("%s %dx%dx%d  kernel %.1f ms  total cycles/wave/sample %.0f" % (cfg, w, h, spp, st["kernel_ms"], total / waves / spp))
    for i, n in enumerate(NAMES):
        ex, lanes, cyc = out[i], out[12 + i], out[24 + i]
        print("%-7s executions/wave/sample %7.2f  lanes/execution %6.2f  lane-visits/sample %6.3f  cycles/execution %8.1f  share %5.1f %%" % (
            n, ex / waves / spp, lanes / max(ex, 1), lanes / (w * h * spp), cyc / max(ex, 1), 100.0 * cyc / max(total, 1)))
    print("claim / vote %5.1f %%   idle %5.1f %%   push %5.1f %%" % (
        100.0 * out[44] / max(total, 1), 100.0 * out[42] / max(total, 1), 100.0 * out[43] / max(total, 1)))
    surf, in_surf, cross = out[12 + 4], out[9], out[12 + 8]
    print("crossings among SURF lane-visits: %d of %d = %.1f %%" % (in_surf, surf, 100.0 * in_surf / max(surf, 1)))
    print("crossings carried by CROSS: %d of %d = %.1f %%" % (cross, cross + in_surf, 100.0 * cross / max(cross + in_surf, 1)))


if __name__ == "__main__":
    main()
