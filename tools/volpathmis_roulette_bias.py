"""`volpath` and `volpathmis` on a scattering slab inside a `null` boundary, with and without Russian roulette, on the CPU oracle.

    python tools/volpathmis_roulette_bias.py [SEEDS] [SPP]        (512 and 4096: a few seconds)

The scene is the slab of tests/test_gpu_specular.py (unit thickness, sigma_t = 1, albedo 0.8, a white sky, a `distant` sensor at 40
degrees) with a `null` BSDF on the boundary.  Prints the mean of SEEDS renders and its standard error for rr_depth = 5 and 100 under both
integrators.  volpathmis.cpp:136-140 divides p_over_f by the roulette's survival probability and leaves p_over_f_nee as it is; the
oracle restates those lines, and `volpathmis` comes out about 0.4 % low at rr_depth = 5 (the index-matched check
of `dielectric`): 0.71210 +- 0.00020 against 0.71465 +- 0.00019 at rr_depth = 100, `volpath` 0.71535 / 0.71486 +- 0.00038."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tests.test_gpu_specular as G                                    # noqa: E402  (the slab's dictionary)
from tests.test_independent_pin import XYZ_TO_RGB                      # noqa: E402
from tests.test_independent_surface_pin import oracle_render           # noqa: E402


def estimate(d, seeds):
    dicts = []
    for seed in range(seeds):
        dd = copy.deepcopy(d)
        dd["sensor"]["sampler"]["seed"] = seed
        dicts.append(dd)
    means = np.array([((film[..., :3] / film[..., 4:5]) @ XYZ_TO_RGB.T)[..., 1].mean() for film in oracle_render(dicts)])
    return means.mean(), means.std(ddof=1) / np.sqrt(seeds)


if __name__ == "__main__":
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    spp = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    for rr_depth in (5, 100):
        for integrator in ("volpath", "volpathmis"):
            d = G.slab(integrator, albedo=0.8, boundary={"type": "null"})
            d["integrator"]["rr_depth"] = rr_depth
            d["sensor"]["sampler"]["sample_count"] = spp
            print("%-10s rr_depth %3d: %.5f +- %.5f" % ((integrator, rr_depth) + estimate(d, seeds)), flush=True)
