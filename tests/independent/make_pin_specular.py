"""Generates tests/golden/indep_pin_surf_specular_16x16.npz: per-pixel mean radiance (linear RGB) and variance of that mean from the
analog walks of tests/independent/specular.py on the `box_specular` problem of problems_specular.py: the lit box with a glass sphere,
a tilted coloured conductor plate and a `twosided(conductor)` panel, ten world-space primitives.

    python -m tests.independent.make_pin_specular

Same scheme as make_pin_cone.py: walks per pixel in chunks of 64 on Philox streams (seed, chunk), summed in chunk order, so the
result does not depend on the number of cores.  The walk count brings the standard error of the image mean below 0.15 % per channel;
the file keeps the walk count and the run time."""
import os
import time

import numpy as np

from . import problems_specular, specular, surface

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAME, PER_PIXEL, SEED, CHUNK = "specular", 24576, 20261121, 64


def _chunk(chunk):
    _, scene, cam, max_depth, vertices = problems_specular.box_specular()
    return specular.render_chunk(scene, cam, CHUNK, SEED, chunk, max_depth, vertices)


def main():
    from multiprocessing import Pool
    _, scene, cam, max_depth, vertices = problems_specular.box_specular()
    t0 = time.time()
    s1 = s2 = 0.0
    with Pool(os.cpu_count() or 1) as pool:
        for a, b in pool.imap(_chunk, range(PER_PIXEL // CHUNK), chunksize=4):
            s1, s2 = s1 + a, s2 + b
    mean, var = surface.finish(s1, s2, PER_PIXEL, cam)
    se = np.sqrt(var.sum((0, 1))) / (cam.w * cam.h) / mean.mean((0, 1))
    seconds = time.time() - t0
    print("%s: image mean %s, standard error %s %%, %.0f s" % (NAME, mean.mean((0, 1)), np.round(100 * se, 3), seconds))
    assert se.max() < 1.5e-3
    path = os.path.join(OUT, "indep_pin_surf_%s_%dx%d.npz" % (NAME, cam.w, cam.h))
    np.savez_compressed(path, mean=mean, var=var, per_pixel=PER_PIXEL, seed=SEED, vertices=vertices, walks=PER_PIXEL * cam.w * cam.h, seconds=seconds)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
