"""Generates tests/golden/indep_pin_surf_textured_16x16.npz: per-pixel mean radiance (linear RGB) and variance of that mean from the
analog walks of tests/independent/surface.py on the textured cornell box of problems_textured.py, whose textures the walk sees as
tiles of constant material.

    python -m tests.independent.make_pin_textured

Same scheme as make_pin.py's surface fixtures: walks per pixel in chunks of 64 on Philox streams (seed, chunk), summed in chunk order,
so the result does not depend on the number of cores.  38 rectangles instead of the box's 6: an analog walk costs about four times the
box's; 24 576 walks per pixel (6.3e6 walks, 80 vertices), as the box's own fixture has.  A first fixture of 12 288 walks (seed 20261101:
0.16 % per channel) put `volpath` 2.6 standard errors below it in all three channels; this one was drawn finer on another seed to see
whether that was the fixture's own error (DESIGN.md section 2 has both sets of figures)."""
import os
import time

import numpy as np

from . import problems_textured, surface

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAME, PER_PIXEL, SEED, CHUNK = "textured", 24576, 20261102, 64


def _chunk(chunk):
    _, scene, cam, max_depth, vertices = problems_textured.box_textured()
    return surface.render_chunk(scene, cam, CHUNK, SEED, chunk, max_depth, vertices)


def main():
    from multiprocessing import Pool
    _, scene, cam, max_depth, vertices = problems_textured.box_textured()
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
