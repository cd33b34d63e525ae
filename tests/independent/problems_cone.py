"""The `cone` surface-transport problem of tests/test_gpu_cone_pin.py, stated twice as problems_surface.py states its own: as a scene
dictionary for the HIP path -- a `shapegroup` of one `twosided`-diffuse cone crown over a thin diffuse box trunk, placed three times by
`instance` under different rotations and uneven scales, one plain one-sided cone, a diffuse ground disk, a grey constant sky and a disk
lamp -- and in the terms of tests/independent/surface.py, which knows neither cones, groups, instances nor two-sided materials.

The second statement:

  cone      `Cone` below, with surface.py's interface (hit, normal, material).  It holds the cone as the image of a right circular cone
            under x -> t + A x: the cone itself is a base point, a unit axis, a base radius and a length, and a ray is intersected from
            the apex, the axis and the half-angle -- ((P - apex) . a)^2 = cos^2(theta) |P - apex|^2, the nappe between base and tip --
            not from the object-space quadratic of the shape plugin (src/shapes/cone.cpp:245-294).  Under an uneven scale the image is
            an oblique elliptic cone; the ray goes to the cone's own space in float64 (t keeps its meaning) and the normal comes back
            through the inverse transpose.  A is R diag(s) column by column from the Rodrigues formula of problems_surface; nothing passes
            through the loader's transforms, the traversal's ray transform or the device's frame code.
  crown     `twosided` with one diffuse child reflects on both sides.  surface.py's diffuse material absorbs from behind, so the crown is
            TWO cones: the outer one looks outwards, the inner one -- the same cone shrunk about its base centre by 1e-9 -- looks inwards.
  trunk     a box: the image of the axis-aligned box under R diag(s) still has orthogonal half-axes, R (s_i h_i e_i).
  the lone cone is one-sided: lit from outside, black seen from inside (through its open base).

`mutation`: the same problem with one thing wrong -- what the pin must reject."""
import math

import numpy as np

from . import problems_surface
from . import surface as S
from .problems_instance import linear_part
from .problems_surface import rodrigues

T = problems_surface.T


class Cone:
    """The image under x -> t + A x of the right circular cone (base centre, unit axis base -> tip, base radius r, length l); the normal
    points outwards, or inwards (`inward`)."""

    def __init__(self, base, axis, r, l, material, inward=False, A=None, t=None):
        self.base, self.u = np.asarray(base, np.float64), S._unit(axis)
        self.r, self.l, self.inward = float(r), float(l), bool(inward)
        self.apex, self.a = self.base + self.l * self.u, -self.u
        self.cos2 = self.l * self.l / (self.l * self.l + self.r * self.r)
        self.A = np.eye(3) if A is None else np.asarray(A, np.float64)
        self.t = np.zeros(3) if t is None else np.asarray(t, np.float64)
        self.Ai = np.linalg.inv(self.A)
        self.material = material
        self.sample_area = self.area = float("nan")                                   # never an emitter here

    def hit(self, o, d):
        o, d = (o - self.t) @ self.Ai.T, d @ self.Ai.T                                # the cone's own space; t keeps its meaning
        w = o - self.apex
        wa, da = w @ self.a, d @ self.a
        qa = da * da - self.cos2 * (d * d).sum(1)
        qb = wa * da - self.cos2 * (w * d).sum(1)                                     # half of the linear coefficient
        qc = wa * wa - self.cos2 * (w * w).sum(1)
        disc = qb * qb - qa * qc
        with np.errstate(divide="ignore", invalid="ignore"):
            root = np.sqrt(np.maximum(disc, 0.0))
            q = -(qb + np.where(qb >= 0.0, root, -root))
            ta, tb = q / qa, qc / q
        best = np.full(o.shape[0], np.inf)
        for t in (ta, tb):
            h = (o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - self.base) @ self.u
            ok = np.isfinite(t) & (disc >= 0.0) & (t > S.T_MIN) & (h >= 0.0) & (h < self.l)
            best = np.where(ok & (t < best), t, best)
        return best

    def normal(self, p):
        q = (p - self.t) @ self.Ai.T - self.base
        e = q - (q @ self.u)[:, None] * self.u
        n = e / np.linalg.norm(e, axis=1, keepdims=True) * self.l + self.u * self.r
        n = n @ self.Ai                                                               # A^-T n
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        return -n if self.inward else n


# ---- the group, in its own space: the crown over the trunk -----------------------------------------------------------------------
CROWN = {"base": [0.0, 0.0, 0.8], "r": 0.8, "l": 1.6, "rho": [0.15, 0.6, 0.2]}
TRUNK = {"centre": [0.0, 0.0, 0.5], "half": [0.12, 0.12, 0.5], "rho": [0.5, 0.3, 0.15]}
# ---- the three placements: translation, rotation axis and angle (degrees), scale: x -> t + R diag(s) x -----------------------------
PLACES = [([-1.9, 0.6, 0.0], [0.0, 0.0, 1.0], 30.0, [1.0, 1.4, 1.2]),
          ([1.8, 1.4, 0.0], [1.0, 1.0, 0.0], 12.0, [1.3, 0.8, 1.0]),
          ([0.3, -1.6, 0.0], [0.3, -0.5, 0.8], 100.0, [0.8, 1.1, 1.5])]
LONE = {"base": [-0.4, 2.6, 0.0], "r": 0.9, "l": 2.2, "rho": [0.6, 0.55, 0.5]}
LONE_TURN = ([1.0, 0.5, 0.0], 15.0)                                                    # the lone cone's axis: z turned about this axis by this angle
SCENE = {"sky": 0.4, "ground": [0.3, 0.25, 0.2], "ground_radius": 14.0,
         "lamp_centre": [0.5, -0.5, 5.0], "lamp_radius": 1.5, "lamp_radiance": [6.0, 5.0, 4.0], "lamp_reflectance": 0.2,
         "origin": [0.0, -6.5, 7.0], "target": [0.0, 0.0, 0.8], "fov": 36.0}
GAP = 1e-9


def placed(place):
    """the group's members under one placement, as world-space primitives"""
    t, axis, angle, scale = place
    t, s = np.asarray(t, np.float64), np.asarray(scale, np.float64)
    A = linear_part(axis, angle, s)
    crown, trunk = S.Material("diffuse", CROWN["rho"]), S.Material("diffuse", TRUNK["rho"])
    prims = [Cone(CROWN["base"], [0, 0, 1], CROWN["r"], CROWN["l"], crown, False, A, t),
             Cone(CROWN["base"], [0, 0, 1], CROWN["r"] * (1.0 - GAP), CROWN["l"] * (1.0 - GAP), crown, True, A, t)]
    h = TRUNK["half"]
    prims.append(S.Box(t + A @ np.asarray(TRUNK["centre"], np.float64), A @ [h[0], 0, 0], A @ [0, h[1], 0], A @ [0, 0, h[2]], trunk))
    return prims


def conifers(width=16, height=16, mutation=None):
    """mutation "upright": the lone cone not turned (in both statements); "order": the third placement with scale and rotation in the
    wrong order, in the dictionary alone.  (The crowns' inner sides are too little of the picture for the pin to tell a one-sided crown:
    measured -0.27 % +- 0.12 % in the green channel.)"""
    assert mutation in (None, "upright", "order")
    c = SCENE
    diffuse, rgb = problems_surface._diffuse, problems_surface._rgb
    turn_axis, turn_angle = LONE_TURN
    lone_angle = 0.0 if mutation == "upright" else turn_angle
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": -1, "rr_depth": 5, "block_size": 32},
         "sensor": problems_surface._sensor(c["origin"], c["target"], [0, 0, 1], c["fov"], width, height),
         "ground": {"type": "disk", "to_world": T.scale(c["ground_radius"]), "bsdf": diffuse(c["ground"])},
         "lamp": {"type": "disk", "to_world": T.translate(c["lamp_centre"]) @ T.rotate([1, 0, 0], 180) @ T.scale(c["lamp_radius"]),
                  "bsdf": diffuse([c["lamp_reflectance"]] * 3), "emitter": {"type": "area", "radiance": rgb(c["lamp_radiance"])}},
         "sky": {"type": "constant", "radiance": rgb([c["sky"]] * 3)},
         "a_group": {"type": "shapegroup", "id": "conifer",
                     "crown": {"type": "cone", "to_world": T.translate(CROWN["base"]) @ T.scale([CROWN["r"], CROWN["r"], CROWN["l"]]),
                               "bsdf": {"type": "twosided", "bsdf": diffuse(CROWN["rho"])}},
                     "trunk": {"type": "cube", "to_world": T.translate(TRUNK["centre"]) @ T.scale(TRUNK["half"]), "bsdf": diffuse(TRUNK["rho"])}},
         "lone": {"type": "cone", "to_world": T.translate(LONE["base"]) @ T.rotate(turn_axis, lone_angle) @ T.scale([LONE["r"], LONE["r"], LONE["l"]]),
                  "bsdf": diffuse(LONE["rho"])}}
    for k, (t, axis, angle, scale) in enumerate(PLACES):
        turn, size = T.rotate(list(axis), angle), T.scale(list(scale))
        d["conifer_%d" % k] = {"type": "instance", "to_world": T.translate(list(t)) @ (size @ turn if (mutation == "order" and k == 2) else turn @ size),
                               "group": {"type": "ref", "id": "conifer"}}
    prims = [S.Disk([0, 0, 0], [0, 0, 1], c["ground_radius"], S.Material("diffuse", c["ground"])),
             S.Disk(c["lamp_centre"], [0, 0, -1], c["lamp_radius"], S.Material("diffuse", c["lamp_reflectance"], Le=c["lamp_radiance"]))]
    for place in PLACES:
        prims += placed(place)
    prims.append(Cone(LONE["base"], rodrigues(turn_axis, lone_angle, [0, 0, 1]), LONE["r"], LONE["l"], S.Material("diffuse", LONE["rho"])))
    cam = S.Pinhole(width, height, c["fov"], c["origin"], c["target"], [0, 0, 1])
    return d, S.Scene(prims, env=[c["sky"]] * 3, n_emitters=2), cam, -1, 56


MAX_ALBEDO = 0.6        # the largest reflectance of the scene


def furnace(width=16, height=16, integrator="path"):
    """Sky L = 1 and every surface `twosided` diffuse with rho = 1: a cone in a group, placed twice (once under an uneven scale), a plain
    cone and a ground disk.  Whatever a path does it returns 1: a wrong frame, side or pdf on the cone darkens (or brightens) it."""
    white = {"type": "twosided", "bsdf": problems_surface._diffuse([1.0, 1.0, 1.0])}
    d = {"type": "scene", "integrator": {"type": integrator, "max_depth": -1, "rr_depth": 5, "block_size": 32},
         "sensor": problems_surface._sensor([0.0, -5.0, 3.0], [0.0, 0.0, 0.8], [0, 0, 1], 40.0, width, height),
         "ground": {"type": "disk", "to_world": T.scale(3.0), "bsdf": white},
         "sky": {"type": "constant", "radiance": problems_surface._rgb([1.0, 1.0, 1.0])},
         "a_group": {"type": "shapegroup", "id": "conifer",
                     "crown": {"type": "cone", "to_world": T.translate([0, 0, 0.25]) @ T.rotate([1, 0.5, 0], 20) @ T.scale([0.75, 0.75, 1.5]), "bsdf": white}},
         "lone": {"type": "cone", "to_world": T.translate([0.25, 1.0, 0.25]) @ T.rotate([0.5, 1, 0.25], 160) @ T.scale([1.0, 1.0, 1.25]), "bsdf": white,
                  "flip_normals": True}}
    for k, (t, axis, angle, scale) in enumerate([([-1.25, 0.0, 0.0], [0, 0, 1], 30.0, [1.0, 1.0, 1.0]), ([1.25, -0.25, 0.0], [1, 1, 0], 15.0, [1.25, 0.75, 1.5])]):
        d["conifer_%d" % k] = {"type": "instance", "to_world": T.translate(t) @ T.rotate(axis, angle) @ T.scale(scale), "group": {"type": "ref", "id": "conifer"}}
    return d
