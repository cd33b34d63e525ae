"""The `twosided` surface-transport problem of tests/test_twosided.py and tests/test_gpu_twosided.py, stated twice as
problems_surface.py states its own: as a scene dictionary with ONE rectangle that carries a `twosided` BSDF for the HIP path, and in
the terms of tests/independent/surface.py, which knows no adapter and whose one-sided materials absorb from behind.

The second statement models the panel as two one-sided rectangles back to back, 1e-9 apart: the front one carries brdf_0 and looks
along the panel's normal, the back one carries brdf_1 and looks the other way.  Their corners are written out by hand in world space
and never pass through the loader's transforms or through the adapter's choice of a side and its flips of wi and wo, so a mistake
in any of those (the children exchanged, the back side black, a direction sampled into the panel) shows up as a disagreement."""
from . import problems_surface
from . import surface as S

# brdf_0 (front) and brdf_1 (back): one colour channel dominant each, none above the box's largest albedo 0.8
FRONT, BACK = [0.1, 0.2, 0.8], [0.8, 0.3, 0.05]
CENTRE, HALF, ANGLE = [0.5, 0.0, 3.0], 2.0, 30.0           # a 4 x 4 panel upright in the middle of the room, turned about z
GAP = 1e-9


def box_panel(width=16, height=16, exchanged=False):
    """The cornell box of problems_surface.box with a free-standing panel inside.  A rectangle lies in z = 0 and looks along +z;
    turned about x by 90 degrees it stands upright and looks along -y, at the camera; turned about z by 30 degrees its normal is
    (sin 30, -cos 30, 0): the camera still sees the front, the back looks at the back wall and the left (red) wall, and the lamp
    overhead lights both sides.  `exchanged`: the two children exchanged (the mutation the pin must reject)."""
    d, scene, cam, max_depth, vertices = problems_surface.box(width, height)
    T = problems_surface.T
    front, back = (BACK, FRONT) if exchanged else (FRONT, BACK)
    # name order decides: "a_front" is brdf_0, "b_back" is brdf_1
    d["panel"] = {"type": "rectangle", "to_world": T.translate(CENTRE) @ T.rotate([0, 0, 1], ANGLE) @ T.rotate([1, 0, 0], 90) @ T.scale([HALF, HALF, 1.0]),
                  "bsdf": {"type": "twosided", "a_front": problems_surface._diffuse(front), "b_back": problems_surface._diffuse(back)}}
    # by hand: the local x edge (2, 0, 0) stays in the xy plane and turns by 30 degrees, 2 (cos 30, sin 30, 0); the local y edge
    # (0, 2, 0) stands up, (0, 0, 2); their cross product is 4 (sin 30, -cos 30, 0)
    eu, ev, n = [1.7320508075688772, 1.0, 0.0], [0.0, 0.0, 2.0], [0.5, -0.8660254037844386, 0.0]
    up = [CENTRE[i] + 0.5 * GAP * n[i] for i in range(3)]
    down = [CENTRE[i] - 0.5 * GAP * n[i] for i in range(3)]
    prims = list(scene.prims) + [S.Rectangle(up, eu, ev, S.Material("diffuse", front)),
                                 S.Rectangle(down, eu, [-x for x in ev], S.Material("diffuse", back))]
    assert abs(prims[-2].n[0] - n[0]) < 1e-12 and abs(prims[-2].n[1] - n[1]) < 1e-12 and abs(prims[-1].n[0] + n[0]) < 1e-12
    assert check_turn(n)
    return d, S.Scene(prims), cam, max_depth, vertices


def check_turn(n):
    """the hand-written normal against the Rodrigues formula of problems_surface (not against the loader's transform)"""
    import numpy as np
    return np.allclose(problems_surface.rodrigues([0, 0, 1], ANGLE, problems_surface.rodrigues([1, 0, 0], 90, [0, 0, 1])), n, atol=1e-12)
