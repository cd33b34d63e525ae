"""Generates tests/golden/indep_pin_surf_instance_16x16.npz: per-pixel mean radiance (linear RGB) and variance of that mean from the
analog walks of tests/independent/surface.py on the cornell box with the five placed sprigs of problems_instance.py, which the walk
sees as twenty world-space primitives worked out by hand (an ellipse and an ellipsoid among them).

    python -m tests.independent.make_pin_instance

Same scheme as make_pin_twosided.py: walks per pixel in chunks of 64 on Philox streams (seed, chunk), summed in chunk order, so the
result does not depend on the number of cores.  Twenty-six primitives; 24 576 walks per pixel (6.3e6 walks, 80 vertices), as the
box's own fixture has (DESIGN.md section 2 has the standard errors)."""
import os
import time

import numpy as np

from . import problems_instance, surface

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAME, PER_PIXEL, SEED, CHUNK = "instance", 24576, 20261021, 64


def _chunk(chunk):
    _, scene, cam, max_depth, vertices = problems_instance.box_grove()
    return surface.render_chunk(scene, cam, CHUNK, SEED, chunk, max_depth, vertices)


def main():
    from multiprocessing import Pool
    _, scene, cam, max_depth, vertices = problems_instance.box_grove()
    t0 = time.time()
    s1 = s2 = 0.0
    with Pool(os.cpu_count() or 1) as pool:
        for a, b in pool.imap(_chunk, range(PER_PIXEL // CHUNK), chunksize=4):
            s1, s2 = s1 + a, s2 + b
    mean, var = surface.finish(s1, s2, PER_PIXEL, cam)
    se = np.sqrt(var.sum((0, 1))) / (cam.w * cam.h) / mean.mean((0, 1))
    print("%s: image mean %s, standard error %s %%, %.0f s" % (NAME, mean.mean((0, 1)), np.round(100 * se, 3), time.time() - t0))
    np.savez_compressed(os.path.join(OUT, "indep_pin_surf_%s_%dx%d.npz" % (NAME, cam.w, cam.h)), mean=mean, var=var, per_pixel=PER_PIXEL, seed=SEED,
                        vertices=vertices)


if __name__ == "__main__":
    main()
