"""The textured surface-transport problem of tests/test_independent_textured_pin.py, stated twice as problems_surface.py states its
own: as a scene dictionary with textures for the HIP path, and in the terms of tests/independent/surface.py, which knows no textures.

The second statement models a texture exactly, as tiles of constant Material: a `nearest` bitmap is constant on every texel, a
checkerboard on every cell.  The tiles are written out in world space by hand -- centres and half edges of the rectangles a texel or
a cell covers on its wall -- and never pass through the loader's transforms, `to_uv`, the wrap rule or the lookup, so a mistake in
any of those (a transposed bitmap, a flipped v, a cell off by half a period, a wall's u and v exchanged) shows up as a disagreement."""
import numpy as np

from . import problems_surface
from . import surface as S

# 4 x 4 rgb texels of the floor, row y first (y grows with v, i.e. with world y); values within the box's range of albedos
FLOOR = np.round(0.15 + 0.65 * np.random.default_rng(20261101).random((4, 4, 3)), 3).astype(np.float32)     # <= 0.8, the box's largest albedo
CHECKER = {"color0": [0.75, 0.6, 0.2], "color1": [0.1, 0.25, 0.6], "scale": 2.0}        # on the right wall: 4 x 4 cells


def box_textured(width=16, height=16):
    """The cornell box of problems_surface.box with the floor carrying a 4 x 4 `nearest` rgb bitmap and the right wall a checkerboard."""
    d, scene, cam, max_depth, vertices = problems_surface.box(width, height)
    T = problems_surface.T
    d["floor"]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "bitmap", "data": FLOOR, "filter_type": "nearest"}}
    d["right"]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "checkerboard", "color0": CHECKER["color0"], "color1": CHECKER["color1"],
                                                             "to_uv": T.scale([CHECKER["scale"], CHECKER["scale"], 1.0])}}
    floor, ceiling, back, left, right, lamp = scene.prims
    prims = [ceiling, back, left, lamp]
    # The floor spans [-5, 5]^2 at z = 0 with u along +x and v along +y (rectangle.cpp:205 on scale(5, 5, 1)): texel (ix, iy) covers
    # x in -5 + 2.5 ix + [0, 2.5], y in -5 + 2.5 iy + [0, 2.5]
    for iy in range(4):
        for ix in range(4):
            prims.append(S.Rectangle([-5 + 2.5 * ix + 1.25, -5 + 2.5 * iy + 1.25, 0], [1.25, 0, 0], [0, 1.25, 0], S.Material("diffuse", FLOOR[iy, ix])))
    # The right wall (x = 5, normal -x) has its local x along +z over z in [0, 7] and its local y along +y over [-5, 5]
    # (problems_surface.box: eu = (0, 0, 3.5), ev = (0, 5, 0)), so u = z / 7 and v = (y + 5) / 10.  With to_uv = scale(2) a cell is a
    # quarter of each: cell (a, b) covers z in 1.75 a + [0, 1.75], y in -5 + 2.5 b + [0, 2.5]; frac(2u) > .5 on odd a, frac(2v) > .5 on odd
    # b, and color0 goes where the two agree (checkerboard.cpp:50-59): a + b even
    for a in range(4):
        for b in range(4):
            colour = CHECKER["color0"] if (a + b) % 2 == 0 else CHECKER["color1"]
            prims.append(S.Rectangle([5, -5 + 2.5 * b + 1.25, 1.75 * a + 0.875], [0, 0, 0.875], [0, 1.25, 0], S.Material("diffuse", colour)))
    for p in prims[4:20]:
        assert np.allclose(p.n, floor.n)
    for p in prims[20:]:
        assert np.allclose(p.n, right.n)
    assert np.isclose(sum(p.area for p in prims[4:20]), floor.area) and np.isclose(sum(p.area for p in prims[20:]), right.area)
    return d, S.Scene(prims), cam, max_depth, vertices
