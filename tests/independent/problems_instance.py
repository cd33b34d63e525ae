"""The instanced surface-transport problem of tests/test_instance.py and tests/test_gpu_instance.py, stated twice as
problems_surface.py states its own: as a scene dictionary with ONE `shapegroup` -- a two-triangle leaf, a disk and a sphere, all
diffuse -- placed five times by `instance` inside the cornell box for the HIP path, and in the terms of
tests/independent/surface.py, which knows neither groups nor instances.

The second statement is twenty world-space primitives.  Every vertex, centre, axis and normal is worked out here in float64 from
the numbers of PLACES with the Rodrigues formula of problems_surface -- the linear part of a placement is A = R diag(s), applied
column by column -- and never passes through the loader's transforms, the ray transform of the traversal or the inverse transpose
of the device code, so a mistake in any of those (a transform applied in the wrong order, a scale left out, a normal carried over
as a vector, a mirror that turns a surface inside out) shows up as a disagreement.  What a placement does to each member:

  leaf    its four corners go through A and the translation.  `diffuse` reflects on the side of the geometric normal only, and the
          reference carries that normal over as a normal (instance.cpp:134): a placement that mirrors keeps the lit side on the
          image of the lit side, while the cross product of the image's edges points the other way -- so the mirrored leaf lists
          its corners in the other order.
  disk    under a rotation and an even scale s it is a disk of radius s r about the image of its centre, with the normal R z;
          under the mirror diag(1, 1, -1) the normal is -R z; under the uneven scale it is an ELLIPSE with the half-axes
          A (r, 0, 0) and A (0, r, 0), and its normal A^-T z is R z again, because z is an axis of the scale.
  sphere  even scale: a sphere of radius s r; mirror: the same sphere; uneven scale: an ELLIPSOID whose half-axes are the columns
          of A r.

The estimator has neither ellipse nor ellipsoid: the two are defined below with surface.py's interface (hit, normal, material).
`mutation`: the same problem with one placement wrong -- what the pin must reject."""
import math

import numpy as np

from . import problems_surface
from . import surface as S
from .problems_surface import rodrigues

# ---- the group, in its own space ------------------------------------------------------------------------------------------
LEAF = [[-0.8, -0.5, 0.0], [0.8, -0.5, 0.0], [0.8, 0.5, 0.25], [-0.8, 0.5, 0.25]]        # two triangles: (0, 1, 2), (0, 2, 3); lit side up
LEAF_RHO, DISK_RHO, BALL_RHO = [0.15, 0.7, 0.1], [0.7, 0.5, 0.15], [0.2, 0.3, 0.75]
DISK_CENTRE, DISK_RADIUS = [0.0, 0.0, -0.45], 0.7                                          # looks along +z
BALL_CENTRE, BALL_RADIUS = [0.0, 0.0, 0.8], 0.4
# ---- the five placements: translation, rotation axis and angle (degrees), scale: x -> t + R diag(s) x ----------------------
PLACES = [
    ([-2.6, -0.5, 1.6], [0.0, 0.0, 1.0], 30.0, [1.0, 1.0, 1.0]),          # a turn about the vertical
    ([2.6, 0.8, 2.2], [1.0, 1.0, 0.0], 50.0, [1.0, 1.0, 1.0]),            # tipped about a horizontal diagonal
    ([0.0, -1.8, 4.4], [1.0, 0.0, 0.0], 65.0, [1.9, 0.7, 1.3]),           # the uneven scale, facing the camera
    ([-2.3, 2.4, 4.9], [0.0, 1.0, 0.0], 25.0, [1.0, 1.0, -1.0]),          # the mirror
    ([2.4, -2.2, 5.0], [0.3, -0.5, 0.8], 110.0, [1.3, 1.3, 1.3]),         # a skew axis and an even scale
]
UNEVEN, MIRROR = 2, 3


class Ellipse:
    """centre + s a + t b with s^2 + t^2 <= 1 (a, b: conjugate half-axes, not necessarily orthogonal); front normal `normal`."""

    def __init__(self, centre, a, b, normal, material):
        self.c, self.a, self.b = (np.asarray(x, np.float64) for x in (centre, a, b))
        self.n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        assert abs(self.n @ self.a) < 1e-12 and abs(self.n @ self.b) < 1e-12
        self.material = material
        self.sample_area = self.area = math.pi * float(np.linalg.norm(np.cross(self.a, self.b)))

    def hit(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - o) @ self.n) / (d @ self.n)
        t = np.where(np.isfinite(t) & (t > S.T_MIN), t, np.inf)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - self.c
        aa, ab, bb = self.a @ self.a, self.a @ self.b, self.b @ self.b
        qa, qb = q @ self.a, q @ self.b
        det = aa * bb - ab * ab
        s, u = (bb * qa - ab * qb) / det, (aa * qb - ab * qa) / det
        return np.where(s * s + u * u <= 1.0, t, np.inf)

    def normal(self, p):
        return np.broadcast_to(self.n, p.shape)


class Ellipsoid:
    """centre + B u, |u| = 1 (the columns of B: conjugate half-axes); the normal points outwards."""

    def __init__(self, centre, B, material):
        self.c, self.B = np.asarray(centre, np.float64), np.asarray(B, np.float64)
        self.Bi = np.linalg.inv(self.B)
        self.material = material
        self.sample_area = self.area = float("nan")                                   # never an emitter here

    def hit(self, o, d):
        q, e = (o - self.c) @ self.Bi.T, d @ self.Bi.T                               # the unit sphere's problem; t keeps its meaning
        a, b, c = (e * e).sum(1), (q * e).sum(1), (q * q).sum(1) - 1.0
        disc = b * b - a * c
        root = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = (-b - root) / a, (-b + root) / a
        t = np.where(t0 > S.T_MIN, t0, np.where(t1 > S.T_MIN, t1, np.inf))
        return np.where(disc >= 0.0, t, np.inf)

    def normal(self, p):
        n = ((p - self.c) @ self.Bi.T) @ self.Bi                                      # B^-T B^-1 (p - c): the gradient of |B^-1 (p - c)|^2
        return n / np.linalg.norm(n, axis=1, keepdims=True)


def linear_part(axis, angle, scale):
    """A = R diag(s), column by column: the images of the scaled basis vectors under the Rodrigues formula"""
    return np.stack([rodrigues(axis, angle, np.eye(3)[k] * scale[k]) for k in range(3)], axis=1)


def placed(place):
    """the group's three members under one placement, as world-space primitives"""
    t, axis, angle, scale = place
    t, s = np.asarray(t, np.float64), np.asarray(scale, np.float64)
    A = linear_part(axis, angle, s)
    at = lambda x: t + A @ np.asarray(x, np.float64)
    leaf, disk, ball = S.Material("diffuse", LEAF_RHO), S.Material("diffuse", DISK_RHO), S.Material("diffuse", BALL_RHO)
    v = [at(x) for x in LEAF]
    mirrors = np.prod(s) < 0
    tris = [(v[0], v[2], v[1]), (v[0], v[3], v[2])] if mirrors else [(v[0], v[1], v[2]), (v[0], v[2], v[3])]
    prims = [S.Triangle(a, b, c, leaf) for a, b, c in tris]
    up = rodrigues(axis, angle, [0.0, 0.0, 1.0]) * (1.0 if s[2] > 0 else -1.0)         # A^-T z = R z / s_z
    even = abs(abs(s[0]) - abs(s[1])) < 1e-15 and abs(abs(s[1]) - abs(s[2])) < 1e-15
    if even:
        prims.append(S.Disk(at(DISK_CENTRE), up, abs(s[0]) * DISK_RADIUS, disk))
        prims.append(S.Sphere(at(BALL_CENTRE), abs(s[0]) * BALL_RADIUS, ball))
    else:
        prims.append(Ellipse(at(DISK_CENTRE), A @ [DISK_RADIUS, 0.0, 0.0], A @ [0.0, DISK_RADIUS, 0.0], up, disk))
        prims.append(Ellipsoid(at(BALL_CENTRE), A * BALL_RADIUS, ball))
    return prims


def box_grove(width=16, height=16, mutation=None):
    """The cornell box of problems_surface.box with the five placements inside.  mutation "unscaled": the third instance without
    its uneven scale; "unmirrored": the fourth without its mirror; "order": the third with scale and rotation in the wrong
    order (diag(s) R instead of R diag(s)) -- in the dictionary alone, which has no other way to say it."""
    d, scene, cam, max_depth, vertices = problems_surface.box(width, height)
    T = problems_surface.T
    places = [list(p) for p in PLACES]
    if mutation == "unscaled":
        places[UNEVEN][3] = [1.0, 1.0, 1.0]
    elif mutation == "unmirrored":
        places[MIRROR][3] = [1.0, 1.0, 1.0]
    else:
        assert mutation in (None, "order")
    diffuse = problems_surface._diffuse
    d["a_group"] = {"type": "shapegroup", "id": "sprig",
                    "leaf": {"type": "mesh", "vertex_positions": np.array(LEAF, np.float32), "faces": np.array([[0, 1, 2], [0, 2, 3]], np.uint32), "bsdf": diffuse(LEAF_RHO)},
                    "disk": {"type": "disk", "to_world": T.translate(DISK_CENTRE) @ T.scale(DISK_RADIUS), "bsdf": diffuse(DISK_RHO)},
                    "ball": {"type": "sphere", "center": BALL_CENTRE, "radius": BALL_RADIUS, "bsdf": diffuse(BALL_RHO)}}
    for k, (t, axis, angle, scale) in enumerate(places):
        turn, size = T.rotate(list(axis), angle), T.scale(list(scale))
        xf = T.translate(list(t)) @ (size @ turn if (mutation == "order" and k == UNEVEN) else turn @ size)
        d["sprig_%d" % k] = {"type": "instance", "to_world": xf, "group": {"type": "ref", "id": "sprig"}}
    prims = list(scene.prims)
    for place in places:
        prims += placed(place)
    return d, S.Scene(prims), cam, max_depth, vertices
