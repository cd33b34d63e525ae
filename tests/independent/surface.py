"""An estimator of surface transport (`path`) that shares NOTHING with oracle/ or the product.

TEST INFRASTRUCTURE, the surface counterpart of walk.py.  Both oracle/ and the HIP kernels restate one reading of
src/integrators/path.cpp (emitter sampling + BSDF sampling combined by MIS, Russian roulette, `max_depth`), so their
bit-equality says nothing about that reading.  This file computes the same radiance in a structurally different way:

  * numpy float64, counter-based Philox random numbers, vectorised over walks;
  * an ANALOG WALK: a walk starts on a sensor ray and bounces by sampling a direction from a density of this file's own
    choice (cosine or uniform hemisphere, cosine over the whole sphere for a leaf); it carries the per-channel weight
    f cos / pdf and scores  weight x Le  when it meets the front of an area emitter,  weight x L_env  when it escapes under
    a constant environment.  No emitter is ever sampled: no next-event estimation, no area / cone / selection pdf in the
    estimate of a diffuse or bilambertian scene, no MIS, no Russian roulette (fixed vertex count, bounded remainder);
  * ray / rectangle, disk, sphere, box, triangle intersection written here in WORLD SPACE from the shape definitions
    (src/shapes/rectangle.cpp:30-60: the square [-1, 1]^2 x {0} with normal +z, disk.cpp:30-62: the unit disk, cube.cpp: the
    box [-1, 1]^3, sphere.cpp:25-70: centre and radius) -- the primitives below hold the images of those definitions as plain
    points and vectors, there is no 4 x 4 matrix and no local frame in this file;
  * BSDFs written from the formulas:
      diffuse       rho / pi on the front side, black from behind (src/bsdfs/diffuse.cpp:85-88, 111-117);
      bilambertian  rho / pi towards the side of incidence, tau / pi through, on either face (src/bsdfs/bilambertian.cpp:131-148);
      rpv           src/bsdfs/rpv.cpp:107-141, one-sided (:148-154), in the frame-free form derived at `rpv_brdf`;
  * `max_depth` restated from path.cpp:124-149: the walk counts its vertices, the first surface hit (or the escape of the
    sensor ray) is vertex 1, emission is collected at vertices 1 .. max_depth: 1 = visible emitters only, 2 = direct light.

One rule of the reference is NOT physics and is restated as such (`rpv_rule="reference"`): RPV::sample returns the BRDF
value f where the weight of a cosine-sampled direction is f cos / pdf = pi f (rpv.cpp:97-104).  In `path` the light gathered at an
rpv vertex through the BSDF-sampling strategy (path.cpp:177-204) is therefore 1 / pi of what it should be, while the light
gathered through emitter sampling (path.cpp:157-172, which calls eval) is right.  With w_e + w_b = 1 the MIS weights of the two
strategies, `path` computes at an rpv vertex
    L_o = integral f cos [ (w_e + w_b / pi) Le_seen + (1 / pi) L_reflected ] d omega
and the walk restates exactly that: the weight behind an rpv vertex is divided by pi and the emission met at the NEXT vertex is
multiplied by pi w_e + w_b.  w_e needs the solid-angle density with which `path` samples that emitter point: 1 / 4 pi for the
constant environment (constant.cpp:84-92), 1 / (2 pi (1 - cos theta_max)) for a sphere seen from outside (sphere.cpp:190-219),
dist^2 / (A |cos|) for a flat emitter (shape.cpp:293-323), each times 1 / #emitters (scene.cpp:180-201).  The weights are the power
heuristic p^2 / (p_e^2 + p_b^2) in `path` and `volpath` (path.cpp:223-227, volpath.cpp:479-483): rpv_rule="reference".  `volpathmis`
keeps densities and values apart (volpathmis.cpp:291-295, 318-319: f = weight x pdf, again 1 / pi of the true f cos on the sampled
side) and combines them as 1 / (p_e / f + p_b / f) (:484-497): the same expression with the balance heuristic p / (p_e + p_b):
rpv_rule="reference_balance".  So the three integrators do NOT render an rpv surface under an area or environment emitter to one
radiance -- a property of the reference, kept by oracle/ and the kernels, and stated here rather than hidden.
rpv_rule="physical" is the plain analog walk.  Scenes without `rpv` never touch any of this.

`point_direct_image` is the deterministic evaluator for a `point` emitter (an analog walk cannot hit a point): midpoint
quadrature of rho / pi x I cos / r^2 x V (point.cpp:98-105) over every pixel's footprint.

It must not import anything from eradiate-kernel_amd/ or oracle/ (tests/test_independent_surface_pin.py checks that).
"""
import math

import numpy as np

T_MIN = 1e-7                                                                      # a ray leaving a surface ignores hits closer than this


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# ---- materials -----------------------------------------------------------------------------------------------------------
class Material:
    """kind: "diffuse" (rho), "bilambertian" (rho, tau), "rpv" (rho0, k, g, rho_c), "black"; Le: radiance of the front side or None."""

    def __init__(self, kind, rho=0.0, tau=0.0, rpv=None, Le=None):
        self.kind = kind
        self.rho = np.broadcast_to(np.asarray(rho, np.float64), (3,)).copy()
        self.tau = np.broadcast_to(np.asarray(tau, np.float64), (3,)).copy()
        self.rpv = rpv
        self.Le = None if Le is None else np.broadcast_to(np.asarray(Le, np.float64), (3,)).copy()

    def max_albedo(self):
        if self.kind == "diffuse":
            return float(self.rho.max())
        if self.kind == "bilambertian":
            return float((self.rho + self.tau).max())
        if self.kind == "rpv":
            return 1.0                                                               # not bounded by its parameters: the caller states a bound
        return 0.0


def rpv_brdf(params, cos_i, cos_o, cos_io):
    """rpv.cpp:107-141 for unit vectors wi, wo pointing away from the surface: cos_i = n.wi, cos_o = n.wo, cos_io = wi.wo.
    The reference writes it with azimuths; s1 s2 cos(phi1 - phi2) = wi.wo - c1 c2, so cos_g = wi.wo and
    tan1 tan2 cos(phi1 - phi2) = (wi.wo - c1 c2) / (c1 c2): no frame is needed."""
    rho0, k, g, rho_c = params
    c1, c2 = cos_i, cos_o
    t1sq, t2sq = (1.0 - c1 * c1) / (c1 * c1), (1.0 - c2 * c2) / (c2 * c2)
    G = np.sqrt(np.maximum(0.0, t1sq + t2sq - 2.0 * (cos_io - c1 * c2) / (c1 * c2)))
    F = (1.0 - g * g) / (1.0 + g * g + 2.0 * g * cos_io) ** 1.5
    return rho0 * (c1 * c2 * (c1 + c2)) ** (k - 1.0) * F * (1.0 + (1.0 - rho_c) / (1.0 + G)) / math.pi


# ---- primitives (world space) --------------------------------------------------------------------------------------------
class Rectangle:
    """centre + s eu + t ev, s, t in [-1, 1]; front normal eu x ev."""

    def __init__(self, centre, eu, ev, material):
        self.c, self.eu, self.ev = (np.asarray(x, np.float64) for x in (centre, eu, ev))
        self.n = _unit(np.cross(self.eu, self.ev))
        self.area = 4.0 * float(np.linalg.norm(np.cross(self.eu, self.ev)))
        self.material = material
        self.sample_area = self.area

    def hit(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - o) @ self.n) / (d @ self.n)
        t = np.where(np.isfinite(t) & (t > T_MIN), t, np.inf)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - self.c
        s, u = (q @ self.eu) / (self.eu @ self.eu), (q @ self.ev) / (self.ev @ self.ev)   # eu, ev are orthogonal
        return np.where((np.abs(s) <= 1.0) & (np.abs(u) <= 1.0), t, np.inf)

    def normal(self, p):
        return np.broadcast_to(self.n, p.shape)


class Disk:
    """Points of the plane through `centre` with front normal `normal` within `radius`."""

    def __init__(self, centre, normal, radius, material):
        self.c, self.n, self.r = np.asarray(centre, np.float64), _unit(normal), float(radius)
        self.area = math.pi * self.r * self.r
        self.material = material
        self.sample_area = self.area

    def hit(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.c - o) @ self.n) / (d @ self.n)
        t = np.where(np.isfinite(t) & (t > T_MIN), t, np.inf)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - self.c
        return np.where((q * q).sum(1) <= self.r * self.r, t, np.inf)

    def normal(self, p):
        return np.broadcast_to(self.n, p.shape)


class Sphere:
    def __init__(self, centre, radius, material):
        self.c, self.r = np.asarray(centre, np.float64), float(radius)
        self.area = 4.0 * math.pi * self.r * self.r
        self.material = material
        self.sample_area = self.area

    def hit(self, o, d):
        oc = o - self.c
        b = (oc * d).sum(1)
        disc = b * b - ((oc * oc).sum(1) - self.r * self.r)
        root = np.sqrt(np.maximum(disc, 0.0))
        t0, t1 = -b - root, -b + root
        t = np.where(t0 > T_MIN, t0, np.where(t1 > T_MIN, t1, np.inf))
        return np.where(disc >= 0.0, t, np.inf)

    def normal(self, p):
        return (p - self.c) / self.r


class Box:
    """centre + a e0 + b e1 + c e2 with a, b, c in [-1, 1]; e0, e1, e2 mutually orthogonal half-axes; normals point outwards."""

    def __init__(self, centre, e0, e1, e2, material):
        self.c = np.asarray(centre, np.float64)
        ax = np.array([e0, e1, e2], np.float64)
        self.half = np.linalg.norm(ax, axis=1)
        self.u = ax / self.half[:, None]
        assert np.abs(self.u @ self.u.T - np.eye(3)).max() < 1e-9
        self.material = material
        self.sample_area = 8.0 * float(self.half[0] * self.half[1] + self.half[1] * self.half[2] + self.half[0] * self.half[2])

    def hit(self, o, d):
        po, pd = (o - self.c) @ self.u.T, d @ self.u.T                               # coordinates along the three axes
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (-self.half - po) / pd, (self.half - po) / pd
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        par = pd == 0.0
        inside = np.abs(po) <= self.half
        lo = np.where(par, np.where(inside, -np.inf, np.inf), lo)
        hi = np.where(par, np.where(inside, np.inf, -np.inf), hi)
        t_in, t_out = lo.max(1), hi.min(1)
        t = np.where(t_in > T_MIN, t_in, np.where(t_out > T_MIN, t_out, np.inf))
        return np.where(t_in <= t_out, t, np.inf)

    def normal(self, p):
        q = ((p - self.c) @ self.u.T) / self.half                                     # in [-1, 1]^3: the face is where |q| is largest
        k = np.argmax(np.abs(q), axis=1)
        return np.sign(q[np.arange(len(k)), k])[:, None] * self.u[k]


class Triangle:
    """p0, p1, p2; front normal (p1 - p0) x (p2 - p0) (a mesh without vertex normals, src/librender/mesh.cpp:352-397)."""

    def __init__(self, p0, p1, p2, material, sample_area=None):
        self.p0 = np.asarray(p0, np.float64)
        self.e1, self.e2 = np.asarray(p1, np.float64) - self.p0, np.asarray(p2, np.float64) - self.p0
        cr = np.cross(self.e1, self.e2)
        self.n = _unit(cr)
        self.area = 0.5 * float(np.linalg.norm(cr))
        self.material = material
        self.sample_area = self.area if sample_area is None else float(sample_area)   # area of the whole mesh it belongs to

    def hit(self, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.p0 - o) @ self.n) / (d @ self.n)
        t = np.where(np.isfinite(t) & (t > T_MIN), t, np.inf)
        q = o + np.where(np.isfinite(t), t, 0.0)[:, None] * d - self.p0
        # barycentric coordinates from the 2 x 2 Gram system of the edges
        a11, a12, a22 = self.e1 @ self.e1, self.e1 @ self.e2, self.e2 @ self.e2
        b1, b2 = q @ self.e1, q @ self.e2
        det = a11 * a22 - a12 * a12
        u, v = (a22 * b1 - a12 * b2) / det, (a11 * b2 - a12 * b1) / det
        return np.where((u >= 0.0) & (v >= 0.0) & (u + v <= 1.0), t, np.inf)

    def normal(self, p):
        return np.broadcast_to(self.n, p.shape)


class Scene:
    def __init__(self, prims, env=None, n_emitters=None, rpv_rule="reference", rpv_density="uniform", diffuse_density="cosine"):
        self.prims = list(prims)
        self.env = None if env is None else np.broadcast_to(np.asarray(env, np.float64), (3,)).copy()
        self.n_emitters = n_emitters                                                  # emitters as `path` counts them: only the rpv rule needs it
        self.rpv_rule, self.rpv_density, self.diffuse_density = rpv_rule, rpv_density, diffuse_density

    def intersect(self, o, d):
        """Nearest hit: distance (inf = none) and primitive index."""
        t = np.full(o.shape[0], np.inf)
        pid = np.full(o.shape[0], -1, np.int64)
        for i, prim in enumerate(self.prims):
            ti = prim.hit(o, d)
            closer = ti < t
            t = np.where(closer, ti, t)
            pid = np.where(closer, i, pid)
        return t, pid

    def max_Le(self):
        le = [p.material.Le.max() for p in self.prims if p.material.Le is not None] + ([self.env.max()] if self.env is not None else [])
        return float(max(le))


def remainder_bound(scene, vertices, max_albedo=None, emission_factor=1.0):
    """Upper bound on the expectation of what a walk cut after `vertices` vertices leaves out: every later vertex adds at most
    weight x emission_factor x max Le, and the expected weight shrinks by at most the largest albedo per bounce:
    sum_{k >= vertices} a^k max Le = a^vertices max Le / (1 - a)."""
    a = max(p.material.max_albedo() for p in scene.prims) if max_albedo is None else max_albedo
    assert a < 1.0
    return emission_factor * a ** vertices * scene.max_Le() / (1.0 - a)


# ---- directions ----------------------------------------------------------------------------------------------------------
def _about(n, cos_t, phi):
    """Unit vectors at polar cosine cos_t and azimuth phi about the unit vectors n."""
    helper = np.where(np.abs(n[:, [0]]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    a = np.cross(n, helper)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = np.cross(n, a)
    s = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t))
    out = (s * np.cos(phi))[:, None] * a + (s * np.sin(phi))[:, None] * b + cos_t[:, None] * n
    return out / np.linalg.norm(out, axis=1, keepdims=True)


def _hemisphere(rng, n, density):
    """Direction about n and f-independent factor cos / pdf: cosine density -> pi, uniform density -> 2 pi cos."""
    m = n.shape[0]
    u1, u2 = rng.random(m), rng.random(m)
    if density == "cosine":
        cos_t = np.sqrt(1.0 - u1)
        return _about(n, cos_t, 2.0 * math.pi * u2), np.full(m, math.pi), cos_t
    cos_t = 1.0 - u1                                                                 # uniform over the hemisphere: pdf 1 / 2 pi
    return _about(n, cos_t, 2.0 * math.pi * u2), 2.0 * math.pi * cos_t, cos_t


def _emitter_direction_density(scene, x, d, t, prim, n_hit):
    """Solid-angle density with which `path` would have sampled the emitter point met from x along d (see the module docstring)."""
    if prim is None:
        p = np.full(x.shape[0], 1.0 / (4.0 * math.pi))
    elif isinstance(prim, Sphere):
        sin2 = prim.r * prim.r / ((prim.c - x) ** 2).sum(1)
        p = 1.0 / (2.0 * math.pi * (1.0 - np.sqrt(np.maximum(0.0, 1.0 - sin2))))
    else:
        p = t * t / (prim.sample_area * np.abs((d * n_hit).sum(1)))
    return p / scene.n_emitters


# ---- the walk ------------------------------------------------------------------------------------------------------------
def radiance(scene, rng, o, d, max_depth=-1, max_vertices=64):
    """Radiance [n, 3] arriving at the points o from the directions d, one walk per ray.  `max_depth` as in path.cpp (-1: no
    limit); the walk visits at most `max_vertices` vertices (the caller bounds what that leaves out, `remainder_bound`)."""
    n = o.shape[0]
    o, d = o.copy(), d.copy()
    w = np.ones((n, 3))
    total = np.zeros((n, 3))
    alive = np.ones(n, bool)
    rpv_from = np.zeros(n, bool)                                                     # the previous vertex was an rpv one (reference rule)
    p_b = np.zeros(n)                                                                # density of the reference's own rpv sampling there
    power = 1 if scene.rpv_rule == "reference_balance" else 2
    last = max_vertices if max_depth < 0 else min(max_depth, max_vertices)
    for vertex in range(1, last + 1):
        ids = np.nonzero(alive)[0]
        if ids.size == 0:
            break
        oo, dd = o[ids], d[ids]
        t, pid = scene.intersect(oo, dd)
        boost = np.ones(ids.size)
        miss = pid < 0
        if miss.any():
            k = ids[miss]
            if scene.env is not None:
                if rpv_from[k].any():
                    pe = _emitter_direction_density(scene, oo[miss], dd[miss], None, None, None)
                    we = pe ** power / (pe ** power + p_b[k] ** power)
                    boost[miss] = np.where(rpv_from[k], math.pi * we + (1.0 - we), 1.0)
                total[k] += w[k] * boost[miss][:, None] * scene.env
            alive[k] = False
        for i, prim in enumerate(scene.prims):
            sel = pid == i
            if not sel.any():
                continue
            k = ids[sel]
            mat = prim.material
            x = oo[sel] + t[sel][:, None] * dd[sel]
            nrm = prim.normal(x)
            wi = -dd[sel]
            cos_i = (wi * nrm).sum(1)
            front = cos_i > 0.0
            if mat.Le is not None:                                                    # area.cpp:63-71: the front side emits
                b = np.ones(k.size)
                if rpv_from[k].any():
                    pe = _emitter_direction_density(scene, oo[sel], dd[sel], t[sel], prim, nrm)
                    we = pe ** power / (pe ** power + p_b[k] ** power)
                    b = np.where(rpv_from[k], math.pi * we + (1.0 - we), 1.0)
                total[k] += np.where(front[:, None], w[k] * b[:, None] * mat.Le, 0.0)
            rpv_from[k] = False
            if vertex == last:
                continue
            if mat.kind == "diffuse":
                nd, factor, _ = _hemisphere(rng, nrm, scene.diffuse_density)
                w[k] *= (mat.rho / math.pi) * factor[:, None]
                alive[k] &= front
            elif mat.kind == "bilambertian":
                # cosine density over the whole sphere, |cos| / 2 pi: f |cos| / pdf = 2 rho towards the side of incidence, 2 tau through
                side = np.where(front, 1.0, -1.0)
                nd, _, _ = _hemisphere(rng, nrm * side[:, None], "cosine")
                through = rng.random(k.size) < 0.5
                nd = np.where(through[:, None], nd - 2.0 * (nd * nrm).sum(1)[:, None] * nrm, nd)
                w[k] *= 2.0 * np.where(through[:, None], mat.tau, mat.rho)
            elif mat.kind == "rpv":
                nd, factor, cos_o = _hemisphere(rng, nrm, scene.rpv_density)
                ok = front & (cos_o > 0.0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    f = rpv_brdf(mat.rpv, np.where(ok, cos_i, 1.0), np.where(ok, cos_o, 1.0), (wi * nd).sum(1))
                w[k] *= (np.where(ok, f, 0.0) * factor)[:, None]
                alive[k] &= ok
                if scene.rpv_rule != "physical":
                    w[k] /= math.pi
                    rpv_from[k] = True
                    p_b[k] = cos_o / math.pi
            else:
                alive[k] = False
                continue
            o[k], d[k] = x, nd
    return total


# ---- sensor --------------------------------------------------------------------------------------------------------------
class Pinhole:
    """Pinhole camera; film x runs to the camera's right seen from behind, y runs down.  Film position (sx, sy) in [0, 1]^2 ->
    direction forward + (1 - 2 sx) tan(fov_x / 2) left + (1 - 2 sy) tan(fov_x / 2) / aspect up (src/sensors/perspective.cpp:
    `fov` spans the film's x axis by default)."""

    def __init__(self, width, height, fov_x_deg, origin, target, up):
        self.w, self.h = int(width), int(height)
        self.o = np.asarray(origin, np.float64)
        self.f = _unit(np.asarray(target, np.float64) - self.o)
        self.left = _unit(np.cross(np.asarray(up, np.float64), self.f))
        self.up = np.cross(self.f, self.left)
        self.tan = math.tan(math.radians(fov_x_deg) / 2.0)

    def rays(self, sx, sy):
        d = (self.f[None, :] + ((1.0 - 2.0 * sx) * self.tan)[:, None] * self.left[None, :]
             + ((1.0 - 2.0 * sy) * self.tan * self.h / self.w)[:, None] * self.up[None, :])
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.broadcast_to(self.o, d.shape).copy(), d

    def sample(self, rng, pix):
        n = pix.shape[0]
        return self.rays(((pix % self.w) + rng.random(n)) / self.w, ((pix // self.w) + rng.random(n)) / self.h)


def render_chunk(scene, camera, per_pixel, seed, chunk, max_depth=-1, max_vertices=64):
    """Sums and sums of squares [pixels, 3] of `per_pixel` walks per pixel, on the Philox stream (seed, chunk)."""
    rng = np.random.Generator(np.random.Philox(key=[int(seed), int(chunk)]))
    npx = camera.w * camera.h
    pix = np.tile(np.arange(npx), per_pixel)
    o, d = camera.sample(rng, pix)
    val = radiance(scene, rng, o, d, max_depth, max_vertices).reshape(per_pixel, npx, 3)
    return val.sum(0), (val * val).sum(0)


def finish(s1, s2, count, camera):
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0) / max(count - 1, 1)
    return mean.reshape(camera.h, camera.w, 3), var.reshape(camera.h, camera.w, 3)


def render(scene, camera, per_pixel, seed, max_depth=-1, max_vertices=64, chunk_walks=64):
    """Per-pixel mean radiance [h, w, 3] and the variance of that mean; chunks of `chunk_walks` walks per pixel, so the result
    does not depend on how the chunks are spread over processes (make_pin.py)."""
    assert per_pixel % chunk_walks == 0
    s1 = s2 = 0.0
    for c in range(per_pixel // chunk_walks):
        a, b = render_chunk(scene, camera, chunk_walks, seed, c, max_depth, max_vertices)
        s1, s2 = s1 + a, s2 + b
    return finish(s1, s2, per_pixel, camera)


# ---- direct light of a point emitter, deterministic --------------------------------------------------------------------------
def point_direct(scene, o, d, position, intensity):
    """Radiance [n, 3] that `max_depth = 2` sees along the rays under one point emitter: rho / pi x I cos / r^2 x V at the first hit
    (diffuse surfaces only); also the primitive hit (-1: none) and the visibility V, for the caller's edge detection."""
    position, intensity = np.asarray(position, np.float64), np.asarray(intensity, np.float64)
    t, pid = scene.intersect(o, d)
    out = np.zeros((o.shape[0], 3))
    vis = np.zeros(o.shape[0], bool)
    for i, prim in enumerate(scene.prims):
        sel = pid == i
        if not sel.any():
            continue
        assert prim.material.kind == "diffuse"
        x = o[sel] + t[sel][:, None] * d[sel]
        nrm = prim.normal(x)
        to_l = position - x
        r = np.linalg.norm(to_l, axis=1)
        wl = to_l / r[:, None]
        cos_l = (wl * nrm).sum(1)
        lit = (cos_l > 0.0) & ((-d[sel] * nrm).sum(1) > 0.0)
        ts, _ = scene.intersect(x, wl)
        v = lit & ~(ts < r * (1.0 - 1e-9))
        out[sel] = np.where(v[:, None], prim.material.rho / math.pi * intensity * (np.maximum(cos_l, 0.0) / (r * r))[:, None], 0.0)
        vis[sel] = v
    return out, pid, vis


def point_direct_image(scene, camera, position, intensity, sub=16):
    """Midpoint quadrature over sub x sub points of every pixel's footprint -> mean [h, w, 3] and `smooth` [h, w]: True where all
    points of the footprint meet one primitive with one visibility, so that no silhouette or shadow edge crosses the pixel (the
    integrand is smooth there and the quadrature error is O(sub^-2) of its curvature)."""
    w, h = camera.w, camera.h
    gx = (np.arange(w * sub) + 0.5) / (w * sub)
    gy = (np.arange(h * sub) + 0.5) / (h * sub)
    sx, sy = np.meshgrid(gx, gy)
    o, d = camera.rays(sx.ravel(), sy.ravel())
    val, pid, vis = point_direct(scene, o, d, position, intensity)
    val = val.reshape(h, sub, w, sub, 3).mean((1, 3))
    pid = pid.reshape(h, sub, w, sub)
    vis = vis.reshape(h, sub, w, sub)
    smooth = (pid.min((1, 3)) == pid.max((1, 3))) & (vis.min((1, 3)) == vis.max((1, 3)))
    return val, smooth
