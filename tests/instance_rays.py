"""Per-ray pins of instanced intersection: the scenes, their expansion, a float64 reference and the ray sets.  CPU only.

TEST INFRASTRUCTURE for tests/test_instance_rays.py (CPU) and tests/test_gpu_instance_rays.py (device).

Two scenes, each two shapegroups placed about two dozen times with heavily overlapping world boxes, plus two plain rectangles (one
between the instances, one behind them):

  dyadic_grove()   every placement is translate(T) . diag(+-2^a, +-2^b, +-2^c) with T a multiple of 2^-4, |T| <= 2; member vertices,
                   centres and radii are multiples of 2^-6 in [-1, 1] (x and y of every vertex and centre are multiples of 2^-2),
                   member transforms are dyadic diagonals plus a translation, ray origins are multiples of 2^-8 in [-4, 4].  The
                   ray transform to group space then rounds nothing, every intermediate of the triangle, rectangle and disk tests is
                   the world-space value times a power of two, and the sphere (uniform |scale| only) scales exactly in double: the
                   device's t, member and primitive must be, bit for bit, the oracle's on `expand(dyadic_grove())`, the same scene
                   written out as plain world-space shapes.  p (the translation rounds at another magnitude) and n (a mirrored mesh
                   recomputed from its vertices flips) are not covered by that argument and go to the float64 reference.
  general_grove()  Rodrigues rotation x uneven scale in [0.5, 2] x translation, a third mirrored, members rotated inside their
                   group, all coordinates <= 4: held to `reference_hits` within a bound measured on the dyadic scene.

`reference_hits` is a brute-force closest hit in world space, float64, over the primitives of tests/independent/surface.py and the
Ellipse / Ellipsoid of tests/independent/problems_instance.py, placed the way problems_instance.placed places them: A = R diag(s)
column by column from the Rodrigues formula, corners and centres through A and the translation, normals through the inverse
transpose (the lit side is carried as a normal: a mirrored triangle lists its corners in the other order).  It passes through
neither the loader's transforms nor any traversal.

Ray sets (`ray_sets`, 4 096 rays each, fixed seeds): `aimed` (origins around the grove, aimed at points drawn on the primitives),
`through` (long rays across the whole grove), `nadir` (d = (0, 0, -1) exactly, so d_rcp = +-inf on two axes) and `inside` (mint /
maxt windows that begin or end inside an instance's box or between two).  Candidates whose float64 winner is met at |cos| < 0.25 are
not drawn, so that the |cos| < 0.2 rule below drops next to nothing; every other rule drops what it drops.  Nadir origins: x is an
odd multiple of 2^-8 and y an odd multiple of 2^-5, so that in group space no origin coordinate equals a vertex coordinate and no
ray runs inside the plane of a mesh's diagonal edge (an exact tie between two faces).  An origin lying exactly on a box plane with a
ray parallel to it gives 0 x inf in the slab test; core/bbox.h then keeps or culls depending on which face it is.  That case concerns
exact-edge hits and is OUT OF SCOPE here: no ray of these sets is such a ray.
"""
import copy
import functools
import importlib
import math

import numpy as np

from tests.independent import surface as S
from tests.independent.problems_instance import Ellipse, Ellipsoid, linear_part
from tests.independent.problems_surface import rodrigues

A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

N_RAYS = 4096
EDGE_MARGIN = 1e-3                                                     # in the primitive's parameter
MIN_COS = 0.2
Z = [0.0, 0.0, 1.0]


class Grove(dict):
    """a scene dictionary that remembers the numbers it was made from (`spec`), for the float64 restatement"""
    spec = None


class Parallelogram(S.Rectangle):
    """centre + s eu + t ev, s, t in [-1, 1], eu and ev not necessarily orthogonal (a rectangle under an uneven scale); front normal `normal`."""

    def __init__(self, centre, eu, ev, normal, material):
        S.Rectangle.__init__(self, centre, eu, ev, material)
        self.n = np.asarray(normal, np.float64) / np.linalg.norm(normal)
        assert abs(self.n @ self.eu) < 1e-12 and abs(self.n @ self.ev) < 1e-12

    def hit(self, o, d):
        t, m = plane_params(self, o, d)
        return np.where(np.isfinite(t) & (t > S.T_MIN) & (m >= 0.0), t, np.inf)


# ---------------------------------------------------------------- the groups
def bumpy_grid(seed=5):
    """4 x 4 cells on [-1, 1]^2, 32 triangles, heights that are multiples of 2^-6 in [0, 1/4]"""
    g = np.linspace(-1.0, 1.0, 5)
    x, y = np.meshgrid(g, g)
    z = np.random.default_rng(seed).integers(0, 17, x.shape) / 64.0
    pos = np.c_[x.ravel(), y.ravel(), z.ravel()]
    faces = []
    for j in range(4):
        for i in range(4):
            a = j * 5 + i
            faces += [[a, a + 1, a + 6], [a, a + 6, a + 5]]
    return pos, np.array(faces, np.int64)


def octahedron():
    """8 triangles about (0, 0, -1/2), outward normals"""
    c, a, h = np.array([0.0, 0.0, -0.5]), 0.75, 0.375
    pos = c + np.array([[a, 0, 0], [0, a, 0], [-a, 0, 0], [0, -a, 0], [0, 0, h], [0, 0, -h]])
    faces = [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [1, 0, 5], [2, 1, 5], [3, 2, 5], [0, 3, 5]]
    return pos, np.array(faces, np.int64)


def _groups(rotated):
    """members: ("mesh", vertices, faces) | ("rectangle" | "disk", centre, axis, angle, (sx, sy)) | ("sphere", centre, radius)"""
    grid, faces = bumpy_grid()
    octa, ofaces = octahedron()
    if rotated:                                                         # members turned inside their group; vertices are what fp32 holds
        grid = np.array([rodrigues([1.0, 0.3, 0.2], 20.0, v) for v in grid]).astype(np.float32).astype(np.float64)
        octa = np.array([rodrigues([0.2, 1.0, 0.5], 35.0, v - [0, 0, -0.5]) + [0, 0, -0.5] for v in octa]).astype(np.float32).astype(np.float64)
        rect = ("rectangle", [0.25, 0.0, -0.25], [1.0, -1.0, 0.5], 25.0, (0.75, 0.5))
        disk = ("disk", [-0.25, 0.25, 0.5], [0.5, 1.0, 0.0], 40.0, (0.5, 0.5))
    else:
        rect = ("rectangle", [0.25, 0.0, -15.0 / 64], Z, 0.0, (0.5, 1.0))
        disk = ("disk", [-0.25, 0.25, 34.0 / 64], Z, 0.0, (0.5, 0.5))
    return {"A": [("mesh", grid, faces), rect, disk],
            "B": [("sphere", [0.0, 0.0, 0.25], 0.75), ("mesh", octa, ofaces)]}


PLAIN = [("between", [0.25, -0.25, 0.375], [1.0, 1.0, 0.0], 70.0, (1.5, 1.0)),
         ("behind", [0.0, 3.5, 0.0], [1.0, 0.0, 0.0], 90.0, (3.5, 3.5))]


def _dyadic_places(count_b=8):
    rng = np.random.default_rng(20)
    places = []
    # On this grid two instances' horizontal surfaces -- the rectangle, the disk, a level face of the mesh -- easily share a plane,
    # and every ray through both is an exact tie in t: a placement is drawn again until its levels are nobody else's.
    grid, faces = bumpy_grid()
    level = {-15.0 / 64, 34.0 / 64} | {float(grid[f[0], 2]) for f in faces if len(set(grid[f, 2])) == 1}
    taken = set()
    for k in range(16):                                                 # group A: uneven dyadic scales, six mirrors
        s = rng.choice([0.5, 1.0, 2.0], 3) * np.where(rng.random(3) < (0.5 if k % 3 == 0 else 0.0), -1.0, 1.0)
        if k % 3 == 0 and np.prod(s) > 0:
            s[int(rng.integers(0, 3))] *= -1.0
        for attempt in range(1000):
            t = np.r_[rng.integers(-20, 21, 2), rng.integers(-24, 25, 1)] / 16.0
            mine = {float(t[2] + s[2] * z) for z in level}
            if not (mine & taken):
                break
        else:
            raise RuntimeError("no free level for placement %d" % k)
        taken |= mine
        places.append(("A", t.tolist(), Z, 0.0, s.tolist()))
    for k in range(count_b):                                            # group B: uniform |scale|, mirrors allowed
        # (no 1/2: a sphere's normal is (p - c) / r, so its fp32 error is that of p over the radius -- the spheres stay large)
        s = float(rng.choice([1.0, 2.0])) * np.where(rng.random(3) < 0.4, -1.0, 1.0)
        t = np.r_[rng.integers(-24, 25, 2), rng.integers(-20, 21, 1)] / 16.0
        places.append(("B", t.tolist(), Z, 0.0, s.tolist()))
    return places


def _general_places():
    rng = np.random.default_rng(21)
    places = []
    for k in range(24):
        g = "A" if k < 16 else "B"
        s = np.round(rng.uniform(0.5 if g == "A" else 0.75, 2.0, 3) * 256) / 256      # group B: see _dyadic_places
        if k % 3 == 0:
            s[k // 3 % 3] *= -1.0
        axis = np.round(rng.normal(size=3) * 64) / 64 + [0.0, 0.0, 1.0 / 128]
        angle = float(np.round(rng.uniform(0.0, 360.0)))
        t = np.round(np.r_[rng.uniform(-1.0, 1.0, 2), rng.uniform(-0.75, 1.0)] * 1024) / 1024
        places.append((g, t.tolist(), axis.tolist(), angle, s.tolist()))
    return places


def _xf(t, axis, angle, s):
    r = T.rotate(list(axis), angle) if angle != 0.0 else T()
    return T.translate(list(t)) @ r @ T.scale(list(s))


def _diffuse(rho):
    return {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(rho)}}


def _member_dict(m):
    if m[0] == "mesh":
        return {"type": "mesh", "vertex_positions": np.asarray(m[1], np.float32), "faces": np.asarray(m[2], np.uint32), "bsdf": _diffuse([0.2, 0.6, 0.1])}
    if m[0] == "sphere":
        return {"type": "sphere", "center": list(m[1]), "radius": m[2], "bsdf": _diffuse([0.3, 0.3, 0.7])}
    return {"type": m[0], "to_world": _xf(m[1], m[2], m[3], [m[4][0], m[4][1], 1.0]), "bsdf": _diffuse([0.6, 0.4, 0.2])}


def _grove(groups, places):
    d = Grove({"type": "scene", "integrator": {"type": "path", "max_depth": 2},
               "sensor": {"type": "perspective", "to_world": T.look_at([0, -3.9, 1], [0, 0, 0], [0, 0, 1]), "fov": 60.0,
                          "film": {"type": "hdrfilm", "width": 4, "height": 4, "rfilter": {"type": "box"}},
                          "sampler": {"type": "independent", "sample_count": 1}},
               "sun": {"type": "directional", "direction": [0.3, -0.2, -1.0], "irradiance": 3.0}})
    for g in sorted(groups):
        d["a_group_%s" % g] = dict({"type": "shapegroup", "id": "group_%s" % g}, **{"m%d_%s" % (j, m[0]): _member_dict(m) for j, m in enumerate(groups[g])})
    for k, (g, t, axis, angle, s) in enumerate(places):
        d["inst_%03d" % k] = {"type": "instance", "to_world": _xf(t, axis, angle, s), "group": {"type": "ref", "id": "group_%s" % g}}
    for k, (name, c, axis, angle, (sx, sy)) in enumerate(PLAIN):
        d["wall_%d_%s" % (k, name)] = {"type": "rectangle", "to_world": _xf(c, axis, angle, [sx, sy, 1.0]), "bsdf": _diffuse([0.5, 0.5, 0.5])}
    d.spec = {"groups": groups, "places": places, "plain": PLAIN}
    return d


def dyadic_grove(count_b=8):
    """count_b: placements of group B (17 of them give the scene level 35 primitives, one more than the larger group has)"""
    return _grove(_groups(False), _dyadic_places(count_b))


def general_grove():
    return _grove(_groups(True), _general_places())


def shape_table(d):
    """where the loader puts things in mts_scene_desc.shapes: {"members": {group: [index per member]}, "instances": [index per
    placement], "plain": [index per plain rectangle]} -- read from the description's records, in the order of `spec`"""
    desc, keep = SD.build_scene_desc(d)
    kinds = [desc.shapes[i].type for i in range(desc.shape_count)]
    groups = [i for i, k in enumerate(kinds) if k == A.SHAPE_SHAPEGROUP]
    names = sorted(d.spec["groups"])
    assert len(groups) == len(names)
    members, inside = {}, set()
    for g, name in zip(groups, names):
        n = desc.shapes[g].face_count
        assert n == len(d.spec["groups"][name])
        members[name] = list(range(g + 1, g + 1 + n))
        inside |= set(members[name])
        want = {"mesh": A.SHAPE_MESH, "rectangle": A.SHAPE_RECTANGLE, "disk": A.SHAPE_DISK, "sphere": A.SHAPE_SPHERE}
        assert [kinds[i] for i in members[name]] == [want[m[0]] for m in d.spec["groups"][name]]
    instances = [i for i, k in enumerate(kinds) if k == A.SHAPE_INSTANCE]
    assert len(instances) == len(d.spec["places"])
    for i, place in zip(instances, d.spec["places"]):
        assert desc.shapes[i].vertex_count == groups[names.index(place[0])]
    plain = [i for i, k in enumerate(kinds) if k == A.SHAPE_RECTANGLE and i not in inside]
    assert len(plain) == len(d.spec["plain"])
    return {"members": members, "instances": instances, "plain": plain}


# ---------------------------------------------------------------- expansion (dyadic placements only)
def expand(d):
    """-> (plain dictionary, [(instance, member's index in the instanced scene's shapes)] per expanded shape).  Every instance written
    out as world-space shapes, instance by instance and member by member: the transform applied in float64 and rounded once to
    fp32; meshes stay meshes with their faces, rectangles and disks keep their type under the composed to_world, a sphere gets
    the image of its centre and |scale| x radius."""
    table = shape_table(d)
    out = {k: copy.deepcopy(v) for k, v in d.items() if not (isinstance(v, dict) and v.get("type") in ("shapegroup", "instance", "rectangle"))}
    where = []
    for k, (g, t, axis, angle, s) in enumerate(d.spec["places"]):
        M = np.asarray(d["inst_%03d" % k]["to_world"].matrix, np.float64)
        L = M[:3, :3]
        if np.count_nonzero(L - np.diag(np.diag(L))):
            raise ValueError("expand(): instance %d is not placed by a diagonal matrix and a translation" % k)
        group = d["a_group_%s" % g]
        for j, m in enumerate(d.spec["groups"][g]):
            src = group["m%d_%s" % (j, m[0])]
            e = {"type": src["type"], "bsdf": copy.deepcopy(src["bsdf"])}
            if m[0] == "mesh":
                v = np.asarray(src["vertex_positions"], np.float64)
                e["vertex_positions"] = (v @ L.T + M[:3, 3]).astype(np.float32)
                e["faces"] = src["faces"].copy()
            elif m[0] == "sphere":
                if len(set(np.abs(np.diag(L)))) != 1:
                    raise ValueError("expand(): a sphere under an uneven scale (instance %d) is no sphere" % k)
                e["center"] = (L @ np.asarray(src["center"], np.float64) + M[:3, 3]).astype(np.float32).tolist()
                e["radius"] = float(np.float32(abs(L[0, 0]) * src["radius"]))
            else:
                e["to_world"] = T((M @ np.asarray(src["to_world"].matrix, np.float64)).astype(np.float32))
            out["x_%03d_%d" % (k, j)] = e
            where.append((k, table["members"][g][j]))
    for k, (name, *_) in enumerate(d.spec["plain"]):
        out["y_%d" % k] = copy.deepcopy(d["wall_%d_%s" % (k, name)])
        where.append((-1, table["plain"][k]))
    return out, where


def reversed_order(plain):
    """the expanded scene with its shapes, and every mesh's faces, listed the other way round: the oracle gives an exact tie in t to
    the later primitive, so its winner is the same in both orders iff no exact tie occurs.  -> dictionary, [index in `plain`'s order]"""
    keys = [k for k in plain if k[:2] in ("x_", "y_")]
    out = {k: v for k, v in plain.items() if k not in keys}
    for n, k in enumerate(reversed(keys)):
        e = copy.deepcopy(plain[k])
        if e["type"] == "mesh":
            e["faces"] = e["faces"][::-1].copy()
        out["z_%04d" % n] = e
    return out, list(range(len(keys)))[::-1]


# ---------------------------------------------------------------- the float64 restatement
def world_primitives(d, mutation=None):
    """-> list of (primitive, instance, member's shape index, face).  mutation ("unmirrored", k): placement k without its mirror;
    ("order", k): placement k with scale and rotation exchanged (diag(s) R instead of R diag(s))."""
    table = shape_table(d)
    mat = S.Material("diffuse", 0.5)
    out = []

    def flat(kind, c, eu, ev, n_local, place_A, at, shape, inst, radius_uv):
        """a rectangle (half-axes eu, ev) or a disk (conjugate radii eu, ev) given in group space"""
        centre, a, b = at(c), place_A @ eu, place_A @ ev
        n = np.linalg.inv(place_A).T @ n_local                           # carried as a normal
        if kind == "rectangle":
            ortho = abs(a @ b) < 1e-14 * np.linalg.norm(a) * np.linalg.norm(b)
            if ortho:
                prim = S.Rectangle(centre, a, b, mat) if np.cross(a, b) @ n > 0 else S.Rectangle(centre, b, a, mat)
            else:
                prim = Parallelogram(centre, a, b, n, mat)
        else:
            ra, rb = np.linalg.norm(a), np.linalg.norm(b)
            round_ = abs(ra - rb) < 1e-14 * ra and abs(a @ b) < 1e-14 * ra * rb
            prim = S.Disk(centre, n, ra, mat) if round_ else Ellipse(centre, a, b, n, mat)
        out.append((prim, inst, shape, 0))

    for k, (g, t, axis, angle, s) in enumerate(d.spec["places"]):
        t, s = np.asarray(t, np.float64), np.asarray(s, np.float64)
        if mutation == ("unmirrored", k):
            assert np.prod(s) < 0
            s = np.abs(s)
        P = linear_part(axis, angle, s) if angle != 0.0 else np.diag(s)
        if mutation == ("order", k):
            P = np.diag(s) @ linear_part(axis, angle, np.ones(3))
        at = lambda x, P=P, t=t: t + P @ np.asarray(x, np.float64)
        mirrors = np.linalg.det(P) < 0
        for j, m in enumerate(d.spec["groups"][g]):
            shape = table["members"][g][j]
            if m[0] == "mesh":
                v = [at(x) for x in m[1]]
                for f, (a, b, c) in enumerate(m[2]):
                    out.append((S.Triangle(v[a], v[c], v[b], mat) if mirrors else S.Triangle(v[a], v[b], v[c], mat), k, shape, f))
            elif m[0] == "sphere":
                even = abs(abs(s[0]) - abs(s[1])) < 1e-15 and abs(abs(s[1]) - abs(s[2])) < 1e-15
                out.append((S.Sphere(at(m[1]), abs(s[0]) * m[2], mat) if even else Ellipsoid(at(m[1]), P * m[2], mat), k, shape, 0))
            else:
                R = linear_part(m[2], m[3], np.ones(3)) if m[3] != 0.0 else np.eye(3)
                flat(m[0], m[1], R[:, 0] * m[4][0], R[:, 1] * m[4][1], R[:, 2], P, at, shape, k, None)
    for k, (name, c, axis, angle, (sx, sy)) in enumerate(d.spec["plain"]):
        R = linear_part(axis, angle, np.ones(3))
        flat("rectangle", np.zeros(3), R[:, 0] * sx, R[:, 1] * sy, R[:, 2], np.eye(3), lambda x, c=c: np.asarray(c, np.float64) + x, table["plain"][k], -1, None)
    return out


def _gram(q, a, b):
    aa, ab, bb = a @ a, a @ b, b @ b
    qa, qb = q @ a, q @ b
    det = aa * bb - ab * ab
    return (bb * qa - ab * qb) / det, (aa * qb - ab * qa) / det


def plane_params(prim, o, d):
    """-> t and the signed distance from the primitive's edge in its own parameter (>= 0: inside), whether or not the ray hits:
    a flat primitive at the crossing of its plane (barycentric margin of a triangle, 1 - max |s|, |t| of a rectangle, 1 - the
    relative radius of a disk or an ellipse); a sphere or an ellipsoid at the ray's closest approach, 1 - the relative distance from
    its centre."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if isinstance(prim, (S.Sphere, Ellipsoid)):
            Bi = np.eye(3) / prim.r if isinstance(prim, S.Sphere) else prim.Bi
            q, e = (o - prim.c) @ Bi.T, d @ Bi.T
            ee, qe = (e * e).sum(1), (q * e).sum(1)
            return -qe / ee, 1.0 - np.sqrt(np.maximum((q * q).sum(1) - qe * qe / ee, 0.0))
        c = prim.p0 if isinstance(prim, S.Triangle) else prim.c
        t = ((c - o) @ prim.n) / (d @ prim.n)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - c
        if isinstance(prim, S.Triangle):
            u, v = _gram(q, prim.e1, prim.e2)
            m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        elif isinstance(prim, S.Rectangle):
            u, v = _gram(q, prim.eu, prim.ev)
            m = 1.0 - np.maximum(np.abs(u), np.abs(v))
        elif isinstance(prim, S.Disk):
            m = 1.0 - np.sqrt((q * q).sum(1)) / prim.r
        else:
            u, v = _gram(q, prim.a, prim.b)
            m = 1.0 - np.sqrt(u * u + v * v)
        return t, np.where(np.isfinite(t), m, -np.inf)


def instance_boxes(d, prims=None):
    """world boxes of the instances, [k, 2, 3], from the primitives' own extents (float64)"""
    prims = prims or world_primitives(d)
    n = len(d.spec["places"])
    lo, hi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    for prim, inst, _, _ in prims:
        if inst < 0:
            continue
        if isinstance(prim, S.Triangle):
            pts = np.array([prim.p0, prim.p0 + prim.e1, prim.p0 + prim.e2])
        elif isinstance(prim, S.Rectangle):
            pts = np.array([prim.c + i * prim.eu + j * prim.ev for i in (-1, 1) for j in (-1, 1)])
        elif isinstance(prim, Ellipse):
            ext = np.sqrt(prim.a ** 2 + prim.b ** 2)
            pts = np.array([prim.c - ext, prim.c + ext])
        elif isinstance(prim, S.Disk):
            ext = prim.r * np.sqrt(np.maximum(1.0 - prim.n ** 2, 0.0))
            pts = np.array([prim.c - ext, prim.c + ext])
        elif isinstance(prim, S.Sphere):
            pts = np.array([prim.c - prim.r, prim.c + prim.r])
        else:
            ext = np.sqrt((prim.B ** 2).sum(1))
            pts = np.array([prim.c - ext, prim.c + ext])
        lo[inst], hi[inst] = np.minimum(lo[inst], pts.min(0)), np.maximum(hi[inst], pts.max(0))
    return np.stack([lo, hi], axis=1)


def box_spans(boxes, o, d):
    """[rays, boxes] entry and exit distances of the slab test in float64 (entry > exit: the ray passes the box by)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (boxes[None, :, 0] - o[:, None]) / d[:, None], (boxes[None, :, 1] - o[:, None]) / d[:, None]
    par = (d == 0.0)[:, None, :]
    inside = (o[:, None] > boxes[None, :, 0]) & (o[:, None] < boxes[None, :, 1])
    lo = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    hi = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    return np.maximum(lo.max(2), 0.0), hi.min(2)


def reference_hits(d, o, d_, mint=None, maxt=None, mutation=None, prims=None):
    """Brute-force closest hit in world space, float64.  -> dict of arrays: t (inf: none), instance (-1: the scene's own geometry),
    member (index in the instanced scene's shapes, -1: none), prim, p, n (front normal: the lit side carried as a normal), cos (n . d),
    gap (distance in t to the runner-up; the ends of the [mint, maxt] window count as runners-up for every candidate), edge (the
    smallest distance, in a primitive's parameter, at which the ray passes an edge or a limb in front of the hit or at it)."""
    o, d_ = np.asarray(o, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(d_, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(o)
    mint = np.full(n, 1500 * 2.0 ** -24) if mint is None else np.asarray(mint, np.float32).astype(np.float64)
    maxt = np.full(n, np.inf) if maxt is None else np.asarray(maxt, np.float32).astype(np.float64)
    prims = prims or world_primitives(d, mutation)
    start = o + mint[:, None] * d_                                      # a primitive's nearest hit behind mint (a sphere's far root included)
    best, second, win = np.full(n, np.inf), np.full(n, np.inf), np.full(n, -1)
    window = np.full(n, np.inf)
    planes = []
    for i, (prim, _, _, _) in enumerate(prims):
        t = prim.hit(start, d_) + mint
        with np.errstate(invalid="ignore"):
            window = np.minimum(window, np.where(np.isfinite(t), np.abs(t - maxt), np.inf))
        near = prim.hit(o, d_)                                          # ... and its nearest hit at all, against the window's start
        window = np.minimum(window, np.where(np.isfinite(near), np.abs(near - mint), np.inf))
        t = np.where(t <= maxt, t, np.inf)
        closer = t < best
        second = np.where(closer, best, np.minimum(second, t))
        win = np.where(closer, i, win)
        best = np.where(closer, t, best)
        planes.append(plane_params(prim, o, d_))
    hit = win >= 0
    p = o + np.where(hit, best, 0.0)[:, None] * d_
    nrm = np.zeros((n, 3))
    for i in np.unique(win[hit]):
        sel = win == i
        nrm[sel] = prims[i][0].normal(p[sel])
    edge = np.full(n, np.inf)
    limit = np.minimum(np.where(hit, best, np.inf), maxt) + 1e-2
    for t, m in planes:
        relevant = (t >= mint - 1e-2) & (t <= limit)
        edge = np.minimum(edge, np.where(relevant, np.abs(m), np.inf))
    meta = np.array([(inst, shape, face) for _, inst, shape, face in prims] + [(-1, -1, -1)])
    second = np.where(hit, second, np.inf)
    best_or_zero = np.where(hit, best, 0.0)
    return {"t": best, "instance": meta[win, 0], "member": meta[win, 1], "prim": meta[win, 2], "p": p, "n": nrm,
            "cos": (nrm * d_).sum(1) / np.linalg.norm(d_, axis=1), "gap": np.minimum(second - best_or_zero, window), "edge": edge, "winner": win}


def kept(ref, e_t):
    """the rays the float64 restatement alone keeps: runner-up gap >= 64 E_t, edge distance >= 1e-3, |cos| >= 0.2 at the hit"""
    hit = np.isfinite(ref["t"])
    return ~((ref["gap"] < 64.0 * e_t) | (ref["edge"] < EDGE_MARGIN) | (hit & (np.abs(ref["cos"]) < MIN_COS)))


# ---------------------------------------------------------------- ray sets
def _snap(x, step=2.0 ** -8):
    return np.clip(np.round(np.asarray(x) / step) * step, -4.0, 4.0)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _point_on(prim, rng):
    if isinstance(prim, S.Triangle):
        b = rng.random(2)
        b = 1.0 - b if b.sum() > 1.0 else b
        return prim.p0 + b[0] * prim.e1 + b[1] * prim.e2
    if isinstance(prim, S.Rectangle):
        s = rng.uniform(-1.0, 1.0, 2)
        return prim.c + s[0] * prim.eu + s[1] * prim.ev
    r, phi = math.sqrt(rng.random()), 2.0 * math.pi * rng.random()
    if isinstance(prim, Ellipse):
        return prim.c + r * math.cos(phi) * prim.a + r * math.sin(phi) * prim.b
    if isinstance(prim, S.Disk):
        a = np.cross(prim.n, [1.0, 0.0, 0.0] if abs(prim.n[0]) < 0.9 else [0.0, 1.0, 0.0])
        a /= np.linalg.norm(a)
        return prim.c + prim.r * r * (math.cos(phi) * a + math.sin(phi) * np.cross(prim.n, a))
    u = _unit(rng, 1)[0]
    return prim.c + (prim.r * u if isinstance(prim, S.Sphere) else prim.B @ u)


def _candidates(name, d, prims, boxes, rng, n):
    """n candidate rays of one set: float32 origins on the 2^-8 grid, float32 directions, mint, maxt"""
    mint, maxt = np.full(n, 1500 * 2.0 ** -24, np.float32), np.full(n, np.inf, np.float32)
    if name == "aimed":
        groups = {}
        for i, (_, inst, shape, _) in enumerate(prims):
            groups.setdefault((inst, shape), []).append(i)
        groups = list(groups.values())
        target = np.array([_point_on(prims[rng.choice(groups[rng.integers(len(groups))])][0], rng) for _ in range(n)])
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
    if name == "inside":
        lo, hi = box_spans(boxes, o.astype(np.float64), w.astype(np.float64))
        crossed = lo < hi
        for i in range(n):
            ks = np.flatnonzero(crossed[i])
            how = i % 3
            if len(ks) == 0:
                continue
            a, b = lo[i, rng.choice(ks)], hi[i, rng.choice(ks)]
            k = rng.choice(ks)
            within = lo[i, k] + rng.random() * (hi[i, k] - lo[i, k])
            if how == 0:                                                # begins inside an instance's box
                mint[i] = within
            elif how == 1:                                              # ends inside one
                maxt[i] = within
            else:                                                       # begins where one box ends, ends where another begins or ends
                mint[i], maxt[i] = min(a, b) + 0.25 * rng.random(), max(a, b) + 0.25 * rng.random()
    return o, w, mint, maxt


GROVES = {"dyadic": dyadic_grove, "dyadic_wide": lambda: dyadic_grove(17), "general": general_grove}


@functools.lru_cache(maxsize=None)
def _ray_sets(which):
    d = GROVES[which]()
    prims = world_primitives(d)
    boxes = instance_boxes(d, prims)
    sets = {}
    for seed, name in enumerate(("aimed", "through", "nadir", "inside")):
        rng = np.random.default_rng(100 + seed)
        o, w, mint, maxt = _candidates(name, d, prims, boxes, rng, 2 * N_RAYS)
        ref = reference_hits(d, o, w, mint, maxt, prims=prims)
        ok = np.flatnonzero(~np.isfinite(ref["t"]) | (np.abs(ref["cos"]) >= 0.25))[:N_RAYS]
        assert len(ok) == N_RAYS, name
        sets[name] = tuple(np.ascontiguousarray(a[ok]) for a in (o, w, mint, maxt))
    return d, prims, boxes, sets


def ray_sets(which):
    """which: a key of GROVES -> {name: (origins, directions, mint, maxt)}, float32, 4 096 rays each"""
    return _ray_sets(which)[3]


@functools.lru_cache(maxsize=None)
def reference(which, name):
    """reference_hits on one ray set, computed once and left unchanged"""
    d, prims, _, sets = _ray_sets(which)
    return reference_hits(d, *sets[name], prims=prims)


# ---------------------------------------------------------------- the fp32 scale, from the oracle on the expanded dyadic scene
@functools.lru_cache(maxsize=None)
def expanded_oracle(which="dyadic"):
    """the oracle's ray_intersect on the expanded dyadic scene over its four ray sets -> {name: result}, [(instance, member)] per
    expanded shape"""
    import tests.oracle_binding as ob
    plain, where = expand(GROVES[which]())
    scene = ob.OracleScene(plain)
    return {name: scene.ray_intersect(*rays) for name, rays in ray_sets(which).items()}, np.array(where)


@functools.lru_cache(maxsize=None)
def fp32_scale():
    """E_t, E_p, E_n: the largest |t - t_ref|, |p - p_ref|, |n - n_ref| of the ORACLE on the expanded dyadic scene against the float64
    restatement -- what fp32 intersection costs at these coordinates; the code under test is not involved.  Measured on the rays
    whose winner is beyond doubt (edge and cos rules, runner-up gap >= 1e-3); the gap rule proper then uses 64 E_t.  A mirrored
    mesh's oracle normal, recomputed from the expanded vertices, points the other way: compared up to that sign."""
    results, where = expanded_oracle()
    e = np.zeros(3)
    for name, got in results.items():
        ref = reference("dyadic", name)
        sure = kept(ref, 1e-3 / 64.0) & np.isfinite(ref["t"]) & np.isfinite(got["t"])
        got, ref = {k: v[sure] for k, v in got.items()}, {k: v[sure] for k, v in ref.items()}
        sure = slice(None)
        dn = np.minimum(np.abs(got["n"] - ref["n"]).max(1), np.abs(got["n"] + ref["n"]).max(1))
        e = np.maximum(e, [np.abs(got["t"] - ref["t"])[sure].max(), np.abs(got["p"] - ref["p"])[sure].max(), dn[sure].max()])
    return tuple(float(x) for x in e)


# ---------------------------------------------------------------- shadow rays: direct light of a point emitter among the instances
LAMP, INTENSITY, GROUND_Z, GROUND_RHO, N_SHADOW = [0.125, -0.25, -2.0], 20.0, -3.5, [0.7, 0.5, 0.3], 256


@functools.lru_cache(maxsize=None)
def _shadow():
    d = general_grove()
    prims = world_primitives(d)
    assert instance_boxes(d, prims)[:, 0, 2].min() >= GROUND_Z + 0.5     # the sensors, 0.25 above the ground, see it unoccluded
    rng = np.random.default_rng(300)
    x = np.c_[rng.uniform(-3.0, 3.0, (N_SHADOW, 2)), np.full(N_SHADOW, GROUND_Z)]
    x[:, 1] = np.minimum(x[:, 1], 2.5)                                   # clear of the wall behind the grove
    w = np.c_[rng.uniform(-0.3, 0.3, (N_SHADOW, 2)), -np.ones(N_SHADOW)]
    w /= np.linalg.norm(w, axis=1)[:, None]
    origins = (x - 0.25 * w).astype(np.float32)
    x = origins.astype(np.float64) + ((GROUND_Z - origins[:, 2].astype(np.float64)) / w.astype(np.float32).astype(np.float64)[:, 2])[:, None] * w.astype(np.float32).astype(np.float64)
    to_lamp = np.asarray(LAMP) - x
    r = np.linalg.norm(to_lamp, axis=1)
    ref = reference_hits(d, x, to_lamp / r[:, None], np.full(N_SHADOW, 1e-3), r, prims=prims)
    # the segment from the ground point to the lamp: occluders beyond the lamp on the same line do not count (maxt = r)
    beyond = reference_hits(d, x, to_lamp / r[:, None], r + 1e-3, np.full(N_SHADOW, np.inf), prims=prims)
    keep = ref["edge"] >= EDGE_MARGIN
    visible = ~np.isfinite(ref["t"])
    cos = to_lamp[:, 2] / r
    expected = np.asarray(GROUND_RHO)[None, :] / math.pi * INTENSITY * (cos / (r * r) * visible)[:, None]
    return d, origins, w.astype(np.float32), expected, keep, visible, np.isfinite(beyond["t"])


def shadow_case(integrator="path", medium=False):
    """-> dictionary, origins, directions, expected radiance (n, 3), kept, visible, "an occluder lies beyond the lamp".  A diffuse
    ground under a `point` emitter inside general_grove(): every sample of `max_depth` = 2 is rho / pi x I cos(theta) / r^2 x V, V
    from reference_hits on the segment from the ground point to the lamp; the restatement alone drops the segments that pass
    within the edge margin of an occluder."""
    d, origins, w, expected, keep, visible, beyond = _shadow()
    d = copy.deepcopy(d)
    del d["sun"]
    fmt = lambda a: ", ".join("%.9g" % v for v in a.ravel())
    d["integrator"] = {"type": integrator, "max_depth": 2}
    d["sensor"] = {"type": "mradiancemeter", "origins": fmt(origins), "directions": fmt(w),
                   "film": {"type": "hdrfilm", "width": N_SHADOW, "height": 1, "rfilter": {"type": "box"}},
                   "sampler": {"type": "independent", "sample_count": 4}}
    d["ground"] = {"type": "rectangle", "to_world": T.translate([0.0, 0.0, GROUND_Z]) @ T.scale(4.0), "bsdf": _diffuse(GROUND_RHO)}
    d["lamp"] = {"type": "point", "position": list(LAMP), "intensity": INTENSITY}
    if medium:                                                          # a medium of no effect (optical depth < 1e-7) puts `volpath` on its ring row
        xf = T.translate([-8, -8, -8]) @ T.scale(16.0)
        grid = lambda v: {"type": "gridvolume", "data": np.full((2, 2, 2), v, np.float32), "to_world": xf}
        d["air"] = {"type": "cube", "to_world": T.scale(8.0), "bsdf": {"type": "null"},
                    "interior": {"type": "heterogeneous", "sigma_t": grid(1e-9), "albedo": grid(0.5), "phase": {"type": "isotropic"}}}
    return d, origins, w, expected, keep, visible, beyond
