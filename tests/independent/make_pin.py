"""Generates the fixtures tests/golden/indep_pin_*.npz: per-pixel mean radiance and variance of that mean from the
independent estimators: tests/independent/walk.py on the C3 / C4 miniatures, tests/independent/surface.py on the surface
problems (fixtures indep_pin_surf_*.npz, linear RGB).

    python -m tests.independent.make_pin [c3] [c4] [surf_box] ...

Takes a few minutes on one core; tests/test_independent_pin.py Z-tests the oracle (and, under -m gpu, the HIP path)
against these numbers and re-runs the estimator at a small sample count to show that the fixtures come from this code."""
import os
import sys
import time

import numpy as np

from . import problems, problems_surface, surface, walk

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
CASES = {   # name: (problem factory, width, height, walks per pixel, seed)
    "c3": (lambda: problems.c3(16, 16, res=16), 16, 16, 3000, 20261004),
    "c4": (lambda: problems.c4(16, 16), 16, 16, 1600, 20261005),
    "c4x3": (lambda: problems.c4x3(16, 16), 16, 16, 1600, 20261006),          # three species: a blendphase nested in a blendphase (round 3)
    # a chromatic slab, one monochromatic run per colour channel (round 3): what spectral MIS is for
    "chroma_r": (lambda: problems.c2_chroma(0), 16, 16, 2000, 20261007),
    "chroma_g": (lambda: problems.c2_chroma(1), 16, 16, 2000, 20261008),
    "chroma_b": (lambda: problems.c2_chroma(2), 16, 16, 2000, 20261009),
}
STEPS, REFINE = 96, 16
# The analog surface walks (surface.py).  Walks per pixel in chunks of 64 on Philox streams (seed, chunk), spread over the machine's
# cores; the result does not depend on that spread.  Measured on 8 cores (an analog walk costs 3 .. 14 us on one of them: the
# target of 0.2 % is reached several times over in seconds, so the fixtures are drawn finer than it):
#
#   name           walks per pixel   walks    vertices   standard error of the image mean (r / g / b)   run time
#   box            24 576            6.3e6    80         0.114 % / 0.114 % / 0.124 %                     13 s
#   box_d3         24 576            6.3e6    3          0.129 % / 0.129 % / 0.131 %                     3 s
#   orbs           16 384            4.2e6    56         0.090 % / 0.081 % / 0.062 %                     3 s
#   orbs_grey      16 384            4.2e6    56         0.080 % (grey)                                  2 s
#   orbs_balance   65 536            1.7e7    56         0.043 % / 0.038 % / 0.029 %                     7 s
#   canopy         49 152            1.3e7    180        0.130 % / 0.127 % / 0.125 %                     16 s
#
# orbs_balance is `orbs` as `volpathmis` renders it (surface.py: rpv_rule="reference_balance"); it was first drawn with 16 384 walks
# and redrawn finer after one pixel failed the Z-test by chance (DESIGN.md section 2 has the figures).
SURF_CASES = {   # name: (problem factory, walks per pixel, seed)
    "surf_box": (problems_surface.box, 24576, 20261019),
    "surf_box_d3": (problems_surface.box_d3, 24576, 20261020),
    "surf_orbs": (problems_surface.orbs, 16384, 20261021),
    "surf_orbs_grey": (problems_surface.orbs_grey, 16384, 20261022),
    "surf_canopy": (problems_surface.canopy, 49152, 20261023),
    "surf_orbs_balance": (problems_surface.orbs_balance, 65536, 20261024),
}
CHUNK = 64


def _surf_chunk(args):
    name, chunk = args
    mk, _, seed = SURF_CASES[name]
    _, scene, cam, max_depth, vertices = mk()
    return surface.render_chunk(scene, cam, CHUNK, seed, chunk, max_depth, vertices)


def surf_main(name):
    from multiprocessing import Pool
    mk, per_pixel, seed = SURF_CASES[name]
    _, scene, cam, max_depth, vertices = mk()
    t0 = time.time()
    s1 = s2 = 0.0
    with Pool(os.cpu_count() or 1) as pool:                                       # sums in chunk order: the same bits on any number of cores
        for a, b in pool.imap(_surf_chunk, [(name, c) for c in range(per_pixel // CHUNK)], chunksize=4):
            s1, s2 = s1 + a, s2 + b
    mean, var = surface.finish(s1, s2, per_pixel, cam)
    se = np.sqrt(var.sum((0, 1))) / (cam.w * cam.h) / mean.mean((0, 1))
    print("%s: image mean %s, standard error %s %%, %.0f s" % (name, mean.mean((0, 1)), np.round(100 * se, 3), time.time() - t0))
    np.savez_compressed(os.path.join(OUT, "indep_pin_%s_%dx%d.npz" % (name, cam.w, cam.h)), mean=mean, var=var, per_pixel=per_pixel, seed=seed,
                        vertices=vertices)


def main(names):
    for name in names:
        if name in SURF_CASES:
            surf_main(name)
            continue
        mk, w, h, per_pixel, seed = CASES[name]
        _, prob, sensor = mk()
        t0 = time.time()
        def progress(done, total):
            if done % 200000 < 20000:
                print("  %s: %d / %d walks, %.0f s" % (name, done, total, time.time() - t0), flush=True)
        mean, var = walk.render(prob, sensor, w, h, per_pixel, seed=seed, steps=STEPS, refine=REFINE, progress=progress)
        se = np.sqrt(var.sum()) / var.size
        print("%s: image mean %.6f, standard error %.2e (%.3f %%), %.0f s" % (name, mean.mean(), se, 100 * se / mean.mean(), time.time() - t0))
        np.savez_compressed(os.path.join(OUT, "indep_pin_%s_%dx%d.npz" % (name, w, h)), mean=mean, var=var,
                            per_pixel=per_pixel, seed=seed, steps=STEPS, refine=REFINE)


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES) + list(SURF_CASES))
