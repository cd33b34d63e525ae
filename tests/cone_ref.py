"""Per-ray pins of the `cone` shape (src/shapes/cone.cpp): a float64 reference, the scenes and the ray sets.  CPU only, numpy.

TEST INFRASTRUCTURE for tests/test_cone.py (CPU) and tests/test_gpu_cone_rays.py (device), in the manner of tests/instance_rays.py.

The reference is a closed-form closest hit of a different construction than the kernel's.  The kernel takes the ray to the cone's
object space and solves x^2 + y^2 = (r / l)^2 (z - l)^2 there.  `Cone` below never leaves the space the cone is given in: from the apex
A = base + l u, the unit axis a = -u (apex -> base) and the half-angle, cos^2(theta) = l^2 / (l^2 + r^2), it solves
    ((P - A) . a)^2 = cos^2(theta) |P - A|^2,   P = o + t d,
keeps the nappe between base and tip (0 <= (P - base) . u < l) and returns t, P and the outward normal (e l + u r) / sqrt(l^2 + r^2),
e the unit radial direction at P.  A cone inside an instance is the same cone seen through the placement x -> T + A x (A = R diag(s),
column by column from the Rodrigues formula of tests/independent/problems_surface.py): the ray goes to group space in float64 (t keeps
its meaning), the normal comes back through the inverse transpose.  Nothing passes through the loader's transforms.

Scenes (`SCENES`):
  plain    three plain cones, turned, r, l in [0.25, 2], one with flip_normals, and a rectangle behind them.
  grove    a group of one cone and one disk placed five times under rotation x uneven scale x translation, one placement mirrored, and
           one plain cone.
  dyadic   one cone with r, l powers of two and an axis-aligned, dyadic-translated to_world, placed ONCE by translate(T) diag(2^a, 2^a,
           2^c); `dyadic_plain` is the same cone written as a plain shape with the composed transform (tests/test_gpu_cone_rays.py (c)).

Ray sets (`ray_sets`, 1 024 rays each, fixed seeds): `aimed` (origins around the scene, aimed at points drawn on the primitives), `through`
(long rays across the scene), `nadir` (d = (0, 0, -1) exactly) and `inside` (mint / maxt windows that begin or end between the roots of
a cone).  Origins are multiples of 2^-8 in [-4, 4].

A ray is left out of a comparison (`kept`) when its float64 hit has any of
  * |cos| < 0.2 between the ray and the normal at the hit;
  * a height within 1e-3 l of the base or the tip -- the hit's own, or that of a root of the same quadratic in front of it inside the
    window, which the nappe test rejected: had it passed, it would have been the hit;
  * a root (of any primitive the ray meets) within 8 E_t of mint or maxt.
At most 5 % of a set may be left out (tests/test_cone.py asserts it on the CPU).  So that the reference alone stays inside that cap,
candidates whose float64 hit is met at |cos| < 0.25 are not drawn; every other rule drops what it drops (well below 1 % of a set).
Hits near the axis stay in: the normal's azimuth is that of the object-space point about the axis, so its error grows like 1 / rho
towards the tip.  `reference_hits` reports rho so that the device test can print the normal's error by distance from the axis.
"""
import functools
import importlib
import math

import numpy as np

from tests.independent.problems_instance import linear_part
from tests.independent.problems_surface import rodrigues

A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

N_RAYS = 1024
MIN_COS = 0.2
EDGE_MARGIN = 1e-3
MAX_LEFT_OUT = 0.05
MINT = 1500 * 2.0 ** -24
Z = [0.0, 0.0, 1.0]


# ---------------------------------------------------------------- primitives, float64, in the space they are given in
class Cone:
    """base centre, axis (base -> tip), base radius r, length l; the normal points outwards (inwards: flip)"""

    def __init__(self, base, axis, r, l, flip=False):
        self.base, self.u = np.asarray(base, np.float64), np.asarray(axis, np.float64) / np.linalg.norm(axis)
        self.r, self.l, self.flip = float(r), float(l), bool(flip)
        self.apex, self.a = self.base + self.l * self.u, -self.u
        self.cos2 = self.l * self.l / (self.l * self.l + self.r * self.r)

    def roots(self, o, d):
        """-> t [n, 2] ascending (nan: none), ok [n, 2] (on the nappe between base and tip), height / l [n, 2]"""
        w = o - self.apex
        wa, da = w @ self.a, d @ self.a
        qa = da * da - self.cos2 * (d * d).sum(1)
        qb = 2.0 * (wa * da - self.cos2 * (w * d).sum(1))
        qc = wa * wa - self.cos2 * (w * w).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            disc = qb * qb - 4.0 * qa * qc
            root = np.sqrt(np.where(disc >= 0.0, disc, np.nan))
            q = -0.5 * (qb + np.where(qb >= 0.0, root, -root))
            t = np.stack([q / qa, qc / q], axis=1)
            lin = qa == 0.0
            t = np.where(lin[:, None], np.stack([-qc / qb, np.full_like(qb, np.nan)], axis=1), t)
        t = np.sort(t, axis=1)                                            # nan last
        h = ((o[:, None, :] + np.nan_to_num(t)[:, :, None] * d[:, None, :] - self.base) @ self.u) / self.l
        ok = np.isfinite(t) & (h >= 0.0) & (h < 1.0)
        return t, ok, np.where(np.isfinite(t), h, np.nan)

    def radial(self, p):
        q = p - self.base
        e = q - (q @ self.u)[:, None] * self.u
        return e, np.linalg.norm(e, axis=1)

    def normal(self, p):
        e, rho = self.radial(p)
        n = (e / rho[:, None] * self.l + self.u * self.r) / math.hypot(self.l, self.r)
        return -n if self.flip else n

    def off_surface(self, p):
        """cone.cpp:383: r (l - z) / l - |xy| of the object-space point: how far p lies inside (> 0) or outside the cone, measured across the axis"""
        q = p - self.base
        return self.r * (self.l - q @ self.u) / self.l - self.radial(p)[1]

    def point(self, rng, h_max=0.9):
        h, phi = rng.uniform(0.05, h_max), rng.uniform(0.0, 2.0 * math.pi)
        e1 = np.cross(self.u, [1.0, 0.0, 0.0] if abs(self.u[0]) < 0.9 else [0.0, 1.0, 0.0])
        e1 /= np.linalg.norm(e1)
        return self.base + h * self.l * self.u + self.r * (1.0 - h) * (math.cos(phi) * e1 + math.sin(phi) * np.cross(self.u, e1))


class Flat:
    """centre + s eu + t ev: |s|, |t| <= 1 (a rectangle) or s^2 + t^2 <= 1 (a disk); front normal eu x ev"""

    def __init__(self, centre, eu, ev, disk):
        self.c, self.eu, self.ev, self.disk = np.asarray(centre, np.float64), np.asarray(eu, np.float64), np.asarray(ev, np.float64), disk
        self.n = np.cross(self.eu, self.ev) / np.linalg.norm(np.cross(self.eu, self.ev))

    def roots(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - o) @ self.n) / (d @ self.n)
        t = np.where(np.isfinite(t), t, np.nan)
        q = o + np.nan_to_num(t)[:, None] * d - self.c
        s, u = (q @ self.eu) / (self.eu @ self.eu), (q @ self.ev) / (self.ev @ self.ev)            # eu, ev are orthogonal
        ok = np.isfinite(t) & ((s * s + u * u <= 1.0) if self.disk else ((np.abs(s) <= 1.0) & (np.abs(u) <= 1.0)))
        return t[:, None], ok[:, None], np.full((len(t), 1), np.nan)

    def normal(self, p):
        return np.broadcast_to(self.n, p.shape)

    def point(self, rng, h_max=None):
        if self.disk:
            r, phi = math.sqrt(rng.random()), 2.0 * math.pi * rng.random()
            return self.c + r * math.cos(phi) * self.eu + r * math.sin(phi) * self.ev
        s = rng.uniform(-1.0, 1.0, 2)
        return self.c + s[0] * self.eu + s[1] * self.ev


class Placed:
    """`prim`, given in group space, seen through x -> t + P x (P any invertible matrix)"""

    def __init__(self, prim, P=None, t=None):
        self.prim = prim
        self.P = np.eye(3) if P is None else np.asarray(P, np.float64)
        self.t = np.zeros(3) if t is None else np.asarray(t, np.float64)
        self.Pi = np.linalg.inv(self.P)

    def roots(self, o, d):
        return self.prim.roots((o - self.t) @ self.Pi.T, d @ self.Pi.T)

    def normal(self, p):
        n = self.prim.normal((p - self.t) @ self.Pi.T) @ self.Pi                                   # P^-T n
        return n / np.linalg.norm(n, axis=1, keepdims=True)

    def point(self, rng, h_max=0.9):
        return self.t + self.P @ self.prim.point(rng, h_max)


# ---------------------------------------------------------------- the scenes
def _xf(t, axis, angle, s):
    r = T.rotate(list(axis), angle) if angle != 0.0 else T()
    return T.translate(list(t)) @ r @ T.scale(list(s))


def _diffuse(rho):
    return {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(rho)}}


def _base():
    return {"type": "scene", "integrator": {"type": "path", "max_depth": 2},
            "sensor": {"type": "perspective", "to_world": T.look_at([0, -3.9, 1], [0, 0, 0], [0, 0, 1]), "fov": 60.0,
                       "film": {"type": "hdrfilm", "width": 4, "height": 4, "rfilter": {"type": "box"}},
                       "sampler": {"type": "independent", "sample_count": 1}},
            "sun": {"type": "directional", "direction": [0.3, -0.2, -1.0], "irradiance": 3.0}}


def _cone_pair(name, base, axis, angle, r, l, flip=False):
    """a cone as the dictionary states it and as the reference holds it: base centre, axis R z, r, l"""
    d = {"type": "cone", "to_world": _xf(base, axis, angle, [r, r, l]), "bsdf": _diffuse([0.3, 0.5, 0.2])}
    if flip:
        d["flip_normals"] = True
    return name, d, Cone(base, rodrigues(axis, angle, Z) if angle != 0.0 else Z, r, l, flip)


# base centre, rotation axis, angle (degrees), r, l, flip_normals
PLAIN_CONES = [([-1.5, -0.25, -0.5], [1.0, 0.25, 0.0], 25.0, 1.0, 2.0, False),
               ([1.25, 0.5, 0.75], [0.25, 1.0, 0.5], 140.0, 2.0, 1.25, True),
               ([0.25, -1.25, 0.5], [1.0, -1.0, 0.25], 75.0, 0.25, 1.5, False)]
WALL = ([0.0, 3.5, 0.0], [1.0, 0.0, 0.0], 90.0, (3.5, 3.5))


def _wall(d, prims):
    c, axis, angle, (sx, sy) = WALL
    d["wall"] = {"type": "rectangle", "to_world": _xf(c, axis, angle, [sx, sy, 1.0]), "bsdf": _diffuse([0.5, 0.5, 0.5])}
    prims.append(("wall", Placed(Flat(c, rodrigues(axis, angle, [sx, 0, 0]), rodrigues(axis, angle, [0, sy, 0]), False))))


def plain():
    d, prims = _base(), []
    for k, spec in enumerate(PLAIN_CONES):
        name, cd, cone = _cone_pair("cone_%d" % k, *spec)
        d[name] = cd
        prims.append((name, Placed(cone)))
    _wall(d, prims)
    return d, prims


# the group: a turned cone and a disk under it; the placements: translation, axis, angle, scale (x -> t + R diag(s) x), the fourth mirrored
GROUP_CONE = ([0.0, 0.0, -0.25], [1.0, 0.5, 0.0], 20.0, 0.75, 1.0)
GROUP_DISK = ([0.0, 0.0, -0.5], 0.5)
PLACES = [([-2.0, -0.5, 0.5], [0.0, 0.0, 1.0], 30.0, [1.0, 1.5, 1.0]),
          ([1.75, 0.75, 1.0], [1.0, 1.0, 0.0], 50.0, [1.5, 1.0, 1.25]),
          ([0.0, -1.5, -1.0], [1.0, 0.0, 0.0], 65.0, [1.25, 0.75, 1.5]),
          ([-1.0, 1.5, -0.25], [0.0, 1.0, 0.0], 25.0, [1.0, 1.25, -1.5]),
          ([1.5, -1.25, -1.5], [0.25, -0.5, 0.75], 110.0, [1.5, 1.5, 0.75])]
LONE_CONE = ([0.25, 0.5, 1.5], [0.5, 1.0, 0.25], 200.0, 1.0, 1.5, False)


def grove():
    d, prims = _base(), []
    base, axis, angle, r, l = GROUP_CONE
    _, cd, cone = _cone_pair("m0_cone", base, axis, angle, r, l)
    dc, dr = GROUP_DISK
    d["a_group"] = {"type": "shapegroup", "id": "tree", "m0_cone": cd,
                    "m1_disk": {"type": "disk", "to_world": T.translate(dc) @ T.scale([dr, dr, 1.0]), "bsdf": _diffuse([0.6, 0.4, 0.2])}}
    disk = Flat(dc, [dr, 0, 0], [0, dr, 0], True)
    for k, (t, ax, ang, s) in enumerate(PLACES):
        d["inst_%d" % k] = {"type": "instance", "to_world": _xf(t, ax, ang, s), "group": {"type": "ref", "id": "tree"}}
        P = linear_part(ax, ang, np.asarray(s, np.float64))
        prims += [("m0_cone", Placed(cone, P, t)), ("m1_disk", Placed(disk, P, t))]
    name, cd, lone = _cone_pair("z_cone", *LONE_CONE)
    d[name] = cd
    prims.append((name, Placed(lone)))
    return d, prims


# r = 2^-1, l = 2^0, base at a dyadic point; placed by translate(T) diag(2^1, 2^1, 2^-1)
DYADIC = {"r": 0.5, "l": 1.0, "base": [0.25, -0.125, -0.5], "T": [-0.5, 0.25, 0.375], "s": [2.0, 2.0, 0.5]}


def dyadic():
    c = DYADIC
    d = _base()
    d["a_group"] = {"type": "shapegroup", "id": "tree",
                    "m0_cone": {"type": "cone", "to_world": T.translate(c["base"]) @ T.scale([c["r"], c["r"], c["l"]]), "bsdf": _diffuse([0.3, 0.5, 0.2])}}
    d["inst_0"] = {"type": "instance", "to_world": T.translate(c["T"]) @ T.scale(c["s"]), "group": {"type": "ref", "id": "tree"}}
    return d, [("m0_cone", Placed(Cone(c["base"], Z, c["r"], c["l"]), np.diag(c["s"]), c["T"]))]


def dyadic_plain():
    """the cone of dyadic() as a plain shape: to_world = translate(T + S base) diag(s_x r, s_x r, s_z l), every entry exact in fp32"""
    c = DYADIC
    s, base = np.asarray(c["s"]), np.asarray(c["T"]) + np.asarray(c["s"]) * np.asarray(c["base"])
    d = _base()
    d["m0_cone"] = {"type": "cone", "to_world": T.translate(base.tolist()) @ T.scale([s[0] * c["r"], s[0] * c["r"], s[2] * c["l"]]), "bsdf": _diffuse([0.3, 0.5, 0.2])}
    return d


SCENES = {"plain": plain, "grove": grove, "dyadic": dyadic}


def shape_indices(d):
    """where the loader puts each named shape in mts_scene_desc.shapes: {name: index}; a group's members by their own names"""
    desc, keep = SD.build_scene_desc(d)
    out, i = {}, 0
    names = sorted(k for k, v in d.items() if isinstance(v, dict) and v.get("type") in ("cone", "rectangle", "disk", "shapegroup", "instance"))
    for name in names:
        out[name] = i
        i += 1
        if d[name]["type"] == "shapegroup":
            assert desc.shapes[out[name]].type == A.SHAPE_SHAPEGROUP
            for m in sorted(k for k, v in d[name].items() if isinstance(v, dict) and v.get("type") in ("cone", "disk")):
                out[m] = i
                i += 1
    assert i == desc.shape_count
    for name, idx in out.items():
        node = d[name] if name in d else d["a_group"][name]
        assert desc.shapes[idx].type == {"cone": A.SHAPE_CONE, "rectangle": A.SHAPE_RECTANGLE, "disk": A.SHAPE_DISK, "shapegroup": A.SHAPE_SHAPEGROUP,
                                         "instance": A.SHAPE_INSTANCE}[node["type"]], name
    return out


# ---------------------------------------------------------------- the float64 closest hit
def reference_hits(prims, o, d_, mint=None, maxt=None):
    """prims: [(name, Placed)].  -> dict of arrays: t (inf: none), winner (index into prims, -1), p, n, cos, height (of the hit, in units
    of l; nan on a flat primitive), rim (the smallest distance from 0 or 1 of the height of a cone root in the window, in front of the
    hit or at it), window (the smallest distance of any root from mint or maxt), rho (distance of the hit from its cone's axis, in the cone's
    own space; inf on a flat primitive)."""
    o, d_ = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(d_, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(o)
    mint = np.full(n, MINT) if mint is None else np.asarray(mint, np.float32).astype(np.float64)
    maxt = np.full(n, np.inf) if maxt is None else np.asarray(maxt, np.float32).astype(np.float64)
    best, win, height = np.full(n, np.inf), np.full(n, -1), np.full(n, np.nan)
    window = np.full(n, np.inf)
    every = []
    for i, (_, prim) in enumerate(prims):
        t, ok, h = prim.roots(o, d_)
        every.append((t, h))
        for k in range(t.shape[1]):
            tk = t[:, k]
            with np.errstate(invalid="ignore"):
                window = np.minimum(window, np.where(np.isfinite(tk), np.minimum(np.abs(tk - mint), np.abs(tk - maxt)), np.inf))
                cand = np.where(ok[:, k] & (tk >= mint) & (tk <= maxt), tk, np.inf)
            closer = cand < best
            best, win, height = np.where(closer, cand, best), np.where(closer, i, win), np.where(closer, h[:, k], height)
    hit = win >= 0
    p = o + np.where(hit, best, 0.0)[:, None] * d_
    nrm, rho = np.zeros((n, 3)), np.full(n, np.inf)
    for i in np.unique(win[hit]):
        sel = win == i
        nrm[sel] = prims[i][1].normal(p[sel])
        if isinstance(prims[i][1].prim, Cone):
            pl = prims[i][1]
            rho[sel] = pl.prim.radial((p[sel] - pl.t) @ pl.Pi.T)[1]
    rim = np.full(n, np.inf)
    limit = np.where(hit, best, maxt)
    for t, h in every:
        for k in range(t.shape[1]):
            with np.errstate(invalid="ignore"):
                relevant = np.isfinite(h[:, k]) & (t[:, k] >= mint) & (t[:, k] <= limit)
                rim = np.minimum(rim, np.where(relevant, np.minimum(np.abs(h[:, k]), np.abs(h[:, k] - 1.0)), np.inf))
    return {"t": best, "winner": win, "p": p, "n": nrm, "cos": (nrm * d_).sum(1) / np.linalg.norm(d_, axis=1), "height": height, "rim": rim,
            "window": window, "rho": rho}


def kept(ref, e_t):
    """the rays the float64 reference alone keeps (the three rules of the module docstring)"""
    hit = np.isfinite(ref["t"])
    return ~((hit & (np.abs(ref["cos"]) < MIN_COS)) | (ref["rim"] < EDGE_MARGIN) | (ref["window"] < 8.0 * e_t))


# ---------------------------------------------------------------- ray sets
def _snap(x, step=2.0 ** -8):
    return np.clip(np.round(np.asarray(x) / step) * step, -4.0, 4.0)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _candidates(name, prims, rng, n):
    mint, maxt = np.full(n, MINT, np.float32), np.full(n, np.inf, np.float32)
    if name == "aimed":
        target = np.array([prims[rng.integers(len(prims))][1].point(rng) for _ in range(n)])
        o = _snap(target + _unit(rng, n) * rng.uniform(1.0, 3.5, (n, 1)))
        w = target - o
    elif name in ("through", "inside"):
        o = _snap(3.8 * _unit(rng, n))
        w = 1.5 * _unit(rng, n) * rng.random((n, 1)) ** (1.0 / 3.0) - o
    else:
        o = np.c_[(2 * rng.integers(-340, 340, n) + 1) / 256.0, (2 * rng.integers(-42, 42, n) + 1) / 32.0, np.full(n, 3.75)]
        w = np.tile([0.0, 0.0, -1.0], (n, 1))
    w = w / np.linalg.norm(w, axis=1)[:, None]
    o, w = o.astype(np.float32), w.astype(np.float32)
    if name == "inside":                                                  # windows that begin or end between the roots of a cone the ray meets
        cones = [pl for _, pl in prims if isinstance(pl.prim, Cone)]
        o64, w64 = o.astype(np.float64), w.astype(np.float64)
        roots = [c.roots(o64, w64)[0] for c in cones]
        for i in range(n):
            pairs = [r[i] for r in roots if np.all(np.isfinite(r[i])) and r[i][0] > 0.0]
            if not pairs:
                continue
            a, b = pairs[rng.integers(len(pairs))]
            within = a + rng.uniform(0.05, 0.95) * (b - a)
            how = i % 3
            if how == 0:
                mint[i] = within
            elif how == 1:
                maxt[i] = within
            else:
                mint[i], maxt[i] = max(a - 0.25 * rng.random(), MINT), b + 0.25 * rng.random()
    return o, w, mint, maxt


@functools.lru_cache(maxsize=None)
def _ray_sets(which):
    d, prims = SCENES[which]()
    sets = {}
    for seed, name in enumerate(("aimed", "through", "nadir", "inside")):
        rng = np.random.default_rng(500 + seed)
        o, w, mint, maxt = _candidates(name, prims, rng, 3 * N_RAYS)
        ref = reference_hits(prims, o, w, mint, maxt)
        ok = np.flatnonzero(~np.isfinite(ref["t"]) | (np.abs(ref["cos"]) >= 0.25))[:N_RAYS]
        assert len(ok) == N_RAYS, (which, name, len(ok))
        sets[name] = tuple(np.ascontiguousarray(a[ok]) for a in (o, w, mint, maxt))
    return d, prims, sets


def scene(which):
    """-> the dictionary and [(name, Placed)] of one of SCENES"""
    return _ray_sets(which)[:2]


def ray_sets(which):
    """which: a key of SCENES -> {name: (origins, directions, mint, maxt)}, float32, 1 024 rays each"""
    return _ray_sets(which)[2]


@functools.lru_cache(maxsize=None)
def reference(which, name):
    """reference_hits on one ray set, computed once and left unchanged"""
    d, prims, sets = _ray_sets(which)
    return reference_hits(prims, *sets[name])


# ---------------------------------------------------------------- the reference's own grid (src/shapes/tests/test_cone.py: test_ray_intersect)
GRID_R, GRID_L, GRID_N = (1, 2, 4, 8), (1, 5, 10), 10


def grid_rays(r, l):
    """10 x 10 rays from y = -10 along +y over [-1.1 r, 1.1 r] x [-1.1 l, 1.1 l] -> origins, directions (float32)"""
    g = np.linspace(-1.0, 1.0, GRID_N).astype(np.float32)
    x, z = np.meshgrid(np.float32(1.1 * r) * g, np.float32(1.1 * l) * g, indexing="ij")
    o = np.stack([x.ravel(), np.full(x.size, -10.0, np.float32), z.ravel()], axis=1).astype(np.float32)
    return o, np.tile(np.array([0.0, 1.0, 0.0], np.float32), (len(o), 1))
