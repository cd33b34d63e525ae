"""The analog walk of surface.py with smooth Fresnel interfaces: a third statement of `dielectric` and `conductor`, in float64, that
shares nothing with eradiate-kernel_amd/, oracle/ or tests/specular_ref.py.  TEST INFRASTRUCTURE.

Built on surface.py's primitives, scene, camera and directions by import (that file is not edited).  What is new here:

  dielectric   a boundary between two media given by their ABSOLUTE indices n_int (behind the surface, against its normal) and n_ext.
               A walk that meets it from the medium of index n1 towards n2 is reflected with the probability R of unpolarised light,
               R = (r_s^2 + r_p^2) / 2,  r_s = (n1 c1 - n2 c2) / (n1 c1 + n2 c2),  r_p = (n2 c1 - n1 c2) / (n2 c1 + n1 c2),
               c2 from Snell's law n1 s1 = n2 s2 (R = 1 beyond the critical angle), and refracted otherwise along
               (n1 / n2) d + ((n1 / n2) c1 - c2) n.  The lobe is CHOSEN, analog, so the weight carries neither R nor 1 - R; it carries
               the lobe's colour and, across the boundary, (n1 / n2)^2: radiance over index squared is what a ray conserves, and the
               walk runs from the sensor towards the light.
  conductor    a one-sided mirror of complex index eta + i k per channel seen from vacuum: the weight takes colour x
               (|r_s|^2 + |r_p|^2) / 2 with r_s = (c - g) / (c + g), r_p = (e c - g) / (e c + g), e = (eta + i k)^2, g = sqrt(e - s^2);
               from behind it absorbs.  A `twosided(conductor)` is two of them back to back (problems_specular.py).
  diffuse      as in surface.py (cosine density, weight rho), black from behind.

No emitter is sampled, there is no MIS and no Russian roulette.  A lamp is black apart from its emission, so a walk scores at most
once; `leftover` returns what the cut after `max_vertices` can still hide (problems_specular.py turns it into the remainder bound).

It must not import anything from eradiate-kernel_amd/ or oracle/."""
import math

import numpy as np

from . import surface as S


class Material(S.Material):
    """S.Material plus kind "dielectric" (n_int, n_ext; rho = colour of the reflected lobe, tau = of the transmitted one) and
    kind "conductor" (eta, k per channel; rho = colour)."""

    def __init__(self, kind, rho=0.0, tau=0.0, Le=None, n_int=1.0, n_ext=1.0, eta=0.0, k=1.0):
        super().__init__(kind, rho, tau, None, Le)
        self.n_int, self.n_ext = float(n_int), float(n_ext)
        self.eta = np.broadcast_to(np.asarray(eta, np.float64), (3,)).copy()
        self.k = np.broadcast_to(np.asarray(k, np.float64), (3,)).copy()


def dielectric_reflectance(c1, n1, n2):
    """R and the cosine of the refracted ray (0 beyond the critical angle) for a ray that meets the boundary at cosine c1 >= 0"""
    s2 = n1 / n2 * np.sqrt(np.maximum(0.0, 1.0 - c1 * c1))
    total = s2 >= 1.0
    c2 = np.sqrt(np.maximum(0.0, 1.0 - s2 * s2))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_s = (n1 * c1 - n2 * c2) / (n1 * c1 + n2 * c2)
        r_p = (n2 * c1 - n1 * c2) / (n2 * c1 + n1 * c2)
        R = 0.5 * (r_s * r_s + r_p * r_p)
    return np.where(total | (c1 <= 0.0), 1.0, R), np.where(total, 0.0, c2)


def conductor_reflectance(c, eta, k):
    """[n, 3]: per channel, for rays that meet the mirror at cosine c > 0"""
    e = (eta + 1j * k)[None, :] ** 2
    c = c[:, None].astype(np.complex128)
    g = np.sqrt(e - (1.0 - c * c))
    with np.errstate(divide="ignore", invalid="ignore"):
        r_s, r_p = (c - g) / (c + g), (e * c - g) / (e * c + g)
    return 0.5 * (np.abs(r_s) ** 2 + np.abs(r_p) ** 2)


def radiance(scene, rng, o, d, max_depth=-1, max_vertices=64, leftover=None):
    """surface.radiance for scenes of diffuse, dielectric and conductor surfaces.  leftover: a list that receives, per walk, the
    largest channel of the weight of a walk still alive after the last vertex (0 for one that ended)."""
    n = o.shape[0]
    o, d = o.copy(), d.copy()
    w = np.ones((n, 3))
    total = np.zeros((n, 3))
    alive = np.ones(n, bool)
    last = max_vertices if max_depth < 0 else min(max_depth, max_vertices)
    for vertex in range(1, last + 1):
        ids = np.nonzero(alive)[0]
        if ids.size == 0:
            break
        oo, dd = o[ids], d[ids]
        t, pid = scene.intersect(oo, dd)
        miss = pid < 0
        if miss.any():
            if scene.env is not None:
                total[ids[miss]] += w[ids[miss]] * scene.env
            alive[ids[miss]] = False
        for i, prim in enumerate(scene.prims):
            sel = pid == i
            if not sel.any():
                continue
            k = ids[sel]
            mat = prim.material
            x = oo[sel] + t[sel][:, None] * dd[sel]
            nrm = prim.normal(x)
            cos_i = -(dd[sel] * nrm).sum(1)
            front = cos_i > 0.0
            if mat.Le is not None:
                total[k] += np.where(front[:, None], w[k] * mat.Le, 0.0)
            if vertex == last:
                continue
            if mat.kind == "diffuse":
                nd, factor, _ = S._hemisphere(rng, nrm, scene.diffuse_density)
                w[k] *= (mat.rho / math.pi) * factor[:, None]
                alive[k] &= front & bool(mat.rho.max() > 0.0)
            elif mat.kind == "conductor":
                w[k] *= mat.rho * conductor_reflectance(np.abs(cos_i), mat.eta, mat.k)
                nd = dd[sel] + 2.0 * cos_i[:, None] * nrm
                alive[k] &= front
            elif mat.kind == "dielectric":
                n1, n2 = np.where(front, mat.n_ext, mat.n_int), np.where(front, mat.n_int, mat.n_ext)
                toward = np.where(front[:, None], nrm, -nrm)                           # the normal on the side the walk comes from
                c1 = np.abs(cos_i)
                R, c2 = dielectric_reflectance(c1, n1, n2)
                reflected = rng.random(k.size) < R
                ratio = n1 / n2
                bent = ratio[:, None] * dd[sel] + (ratio * c1 - c2)[:, None] * toward
                nd = np.where(reflected[:, None], dd[sel] + 2.0 * c1[:, None] * toward, bent)
                nd /= np.linalg.norm(nd, axis=1, keepdims=True)
                w[k] *= np.where(reflected[:, None], mat.rho, mat.tau * (ratio * ratio)[:, None])
            else:
                assert mat.kind == "black", mat.kind
                alive[k] = False
                continue
            o[k], d[k] = x, nd
    if leftover is not None:
        leftover.append(np.where(alive, w.max(1), 0.0))
    return total


def render_chunk(scene, camera, per_pixel, seed, chunk, max_depth=-1, max_vertices=64, leftover=None):
    """surface.render_chunk with this file's walk"""
    rng = np.random.Generator(np.random.Philox(key=[int(seed), int(chunk)]))
    npx = camera.w * camera.h
    pix = np.tile(np.arange(npx), per_pixel)
    o, d = camera.sample(rng, pix)
    val = radiance(scene, rng, o, d, max_depth, max_vertices, leftover).reshape(per_pixel, npx, 3)
    return val.sum(0), (val * val).sum(0)


def render(scene, camera, per_pixel, seed, max_depth=-1, max_vertices=64, chunk_walks=64):
    assert per_pixel % chunk_walks == 0
    s1 = s2 = 0.0
    for c in range(per_pixel // chunk_walks):
        a, b = render_chunk(scene, camera, chunk_walks, seed, c, max_depth, max_vertices)
        s1, s2 = s1 + a, s2 + b
    return S.finish(s1, s2, per_pixel, camera)


def remainder_bound(scene, camera, vertices, max_index_ratio, walks_per_pixel=64, seed=1):
    """Upper bound on the expectation of what the cut after `vertices` vertices leaves out, from a run of the walk itself: a lamp is
    black apart from its emission, so a walk scores at most once more, with at most its weight at the cut times the largest factor a
    later boundary crossing can put on it (max_index_ratio^2: a walk cut inside the denser medium) times the largest radiance.
    Returns (bound, share of the walks still alive at the cut)."""
    left = []
    render_chunk(scene, camera, walks_per_pixel, seed, 0, -1, vertices, left)
    return float(left[0].mean()) * max_index_ratio ** 2 * scene.max_Le(), float((left[0] > 0).mean())
