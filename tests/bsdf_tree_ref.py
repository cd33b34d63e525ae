"""A float64 restatement of one `path` / `volpath` sample on a single flat sheet whose BSDF is a tree: leaves (`diffuse`, `rpv`,
`bilambertian`) under `blendbsdf` and `twosided`, with textured parameters.  TEST INFRASTRUCTURE: plain numpy, no device code; the
reference's sources are cited by file and line and are never read at run time.

Why it exists: the CPU oracle knows no textures, blends or adapters, so the wrappers of csrc/integrator_dev.h (bsdf_apply_textures,
blend_weight, blend_eval_pdf, blend_sample, twosided_side, HitBsdfTex) have no bit-level reference.  Under a `constant` emitter at
max_depth = 3 a lane of SamplingIntegrator::sample on one sheet is a closed function of five uniforms -- one emitter sample (eval,
pdf, MIS weight) and one BSDF sample (sample, MIS weight, the radiance the escaping ray meets) -- and that function is written here.

A tree is described ONCE, as a small structure of dictionaries (diffuse(), rpv(), bilambertian(), blend(), twosided() below);
bsdf_dict() turns it into the scene dictionary's BSDF and Evaluator into the restatement, so the two cannot drift apart.

What is NOT restated: `volpathmis` (another estimator: weight matrices instead of the power heuristic), area emitters, wi.z == 0."""
import copy
import importlib

import numpy as np

import tests.oracle_binding as ob
import tests.sheet_shared as shared
import tests.test_gpu_textures as gt

SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

INV_PI, INV_FOUR_PI = 1.0 / np.pi, 1.0 / (4.0 * np.pi)
LUMINANCE = np.array([0.212671, 0.715160, 0.072169])                      # core/spectrum.h:246-248
SKY = np.array([0.9, 1.3, 0.6], np.float32)                               # the chromatic `constant` emitter's radiance
N_LANES = 4099                                                            # 16 full blocks of 256 and a ragged tail
N_FILM = 300                                                              # the rays that also make up the mradiancemeter of the row tests
SEED_OFFSET = 11

# ---- the fp32 scale E (section b of tests/test_bsdf_tree_ref.py): max over kept lanes and channels of
# |oracle - float64| / (|float64| + mean(SKY)), MEASURED ON THE CPU from oracle_sample of plain, untextured leaves -- nothing measured
# on the device enters it -- and rounded up to two digits.  Canonical: rectangle, disk and quad as tests/test_gpu_textures.py places
# them; world: the rectangle and the quad expanded by the instance placements below.  The device bound is DEVICE_FACTOR * E: the
# factor the instanced-intersection pin uses, for the wrappers' extra roundings (three per eval / pdf, one division in the rescaled
# sample1) and two more fp32 affine transforms of an instanced hit.
E_CANONICAL = 1.6e-6        # measured 1.575e-6
E_WORLD = 1.6e-6            # measured 1.575e-6
DEVICE_FACTOR = 8.0
# The bilinear cases (BILINEAR below) are held to the texture tests' ATOL instead, absolute, on the value.

THRESHOLD_MARGIN = 1e-5          # sample1 against a blend's weight, the rescaled one against a bilambertian's r / (r + t)
HORIZON_MARGIN = 1e-3            # |wo.z| of the emitter-sampled and of the BSDF-sampled direction
WI_MARGIN = 0.2                  # |wi.z|
MAX_DROP = 0.02                  # the share of a case's lanes the rules above may leave out

MUTATIONS = ("mixture_pdf", "children_exchanged", "sides_exchanged", "unrescaled_sample1", "wo_not_flipped_back",
             "clamp_before_interpolation", "no_clamp", "rpv_weight_times_pi")


def f32(x):
    """the value the device holds: rounded to float32, then exact in float64"""
    return np.asarray(np.asarray(x, np.float32), np.float64)


# ================================================================ the description of a tree
def diffuse(reflectance):
    return {"kind": "diffuse", "reflectance": reflectance}


def rpv(rho_0, k, g, rho_c):
    return {"kind": "rpv", "rho_0": rho_0, "k": k, "g": g, "rho_c": rho_c}


def bilambertian(reflectance, transmittance):
    return {"kind": "bilambertian", "reflectance": reflectance, "transmittance": transmittance}


def blend(child_0, child_1, weight):
    return {"kind": "blend", "children": [child_0, child_1], "weight": weight}


def twosided(front, back=None):
    return {"kind": "twosided", "children": [front] if back is None else [front, back]}


_PARAMS = {"diffuse": ("reflectance",), "rpv": ("rho_0", "k", "g", "rho_c"), "bilambertian": ("reflectance", "transmittance")}


def _is_texture(v):
    return isinstance(v, dict)


def _param_dict(v):
    return copy.copy(v) if _is_texture(v) else (float(v) if np.ndim(v) == 0 else {"type": "rgb", "value": [float(x) for x in v]})


def bsdf_dict(tree):
    """the tree as the scene dictionary's BSDF.  Nested BSDFs are taken in the order of their names (Properties order)."""
    kind = tree["kind"]
    if kind in _PARAMS:
        return dict({"type": kind}, **{name: _param_dict(tree[name]) for name in _PARAMS[kind]})
    if kind == "blend":
        w = tree["weight"]
        return {"type": "blendbsdf", "weight": copy.copy(w) if _is_texture(w) else float(w),
                "bsdf_a": bsdf_dict(tree["children"][0]), "bsdf_b": bsdf_dict(tree["children"][1])}
    out = {"type": "twosided", "brdf_a": bsdf_dict(tree["children"][0])}
    if len(tree["children"]) == 2:
        out["brdf_b"] = bsdf_dict(tree["children"][1])
    return out


# ================================================================ warps (warp.h), float64
def square_to_uniform_disk_concentric(u):
    """warp.h:80-118 (Shirley's concentric map as the reference writes it)"""
    x, y = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    q13 = np.abs(x) < np.abs(y)
    r, rp = np.where(q13, y, x), np.where(q13, x, y)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = 0.25 * np.pi * rp / r
    phi = np.where(q13, 0.5 * np.pi - phi, phi)
    phi = np.where((x == 0) & (y == 0), 0.0, phi)
    return np.c_[r * np.cos(phi), r * np.sin(phi)]


def square_to_cosine_hemisphere(u):
    """warp.h:326-341: the concentric disk lifted to the hemisphere; its density is z / pi (:343-350)"""
    p = square_to_uniform_disk_concentric(u)
    return np.c_[p, np.sqrt(np.maximum(1.0 - p[:, 0] ** 2 - p[:, 1] ** 2, 0.0))]


def square_to_uniform_sphere(u):
    """warp.h:235-244: z = 1 - 2 v, the azimuth from u"""
    z = 1.0 - 2.0 * u[:, 1]
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return np.c_[r * np.cos(2.0 * np.pi * u[:, 0]), r * np.sin(2.0 * np.pi * u[:, 0]), z]


def mis_weight(pdf_a, pdf_b):
    """path.cpp:226-230, volpath.cpp:479-483: the power heuristic"""
    a, b = pdf_a * pdf_a, pdf_b * pdf_b
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(a > 0, a / (a + b), 0.0)


# ================================================================ the evaluator of a tree at given uv
class Sample:
    """BSDFSample and weight of n lanes, with what the lane-dropping rules and the branch counts need"""

    def __init__(self, n):
        self.wo, self.pdf, self.weight = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3))
        self.threshold = np.full(n, np.inf)                    # distance of a sample1 from the nearest threshold it was tested against
        self.tags = {}                                          # branch name -> (n,) int, -1 where the lane never met that branch

    def select(self, mask, a, b):
        """a where mask, b elsewhere; thresholds met on the way down accumulate"""
        self.wo, self.pdf, self.weight = np.where(mask[:, None], a.wo, b.wo), np.where(mask, a.pdf, b.pdf), np.where(mask[:, None], a.weight, b.weight)
        self.threshold = np.minimum(self.threshold, np.where(mask, a.threshold, b.threshold))
        for name in set(a.tags) | set(b.tags):
            none = np.full(len(mask), -1)
            self.tags[name] = np.where(mask, a.tags.get(name, none), b.tags.get(name, none))
        return self


class Evaluator:
    """eval_pdf(wi, wo) and sample(wi, sample1, sample2) of a tree at n hits with texture coordinates `uv`, float64.
    mono: colours are their luminance (the *_mono variants).  mutation: one of MUTATIONS, a deliberately wrong restatement."""

    def __init__(self, tree, uv, mono=False, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.tree, self.uv, self.n, self.mono, self.mutation = tree, np.asarray(uv, np.float64), len(uv), mono, mutation
        self.edge = np.full(self.n, np.inf)                    # distance of the hit to the nearest discontinuity of any lookup, in texels
        self.root = self._bind(tree)

    # ---- parameters at the hits
    def _colour(self, v):
        if _is_texture(v):
            value, edge = gt.texture_eval(v, self.uv)                # float64, from the fp32 texels
            self.edge = np.minimum(self.edge, edge)
        else:
            value = np.broadcast_to(f32(v), (self.n, 3)) if np.ndim(v) else np.full((self.n, 3), float(f32(v)))
        if self.mono:
            value = np.repeat((value @ LUMINANCE)[:, None], 3, axis=1)
        return np.array(value, np.float64)

    def _weight(self, w):
        """blendbsdf.cpp:162-164: clamp(eval_1, 0, 1) AFTER the lookup; eval_1 of a three-channel bitmap is its luminance (bitmap.cpp:285-302)"""
        if not _is_texture(w):
            return np.full(self.n, float(f32(w)))
        if self.mutation == "clamp_before_interpolation":
            w = dict(w)
            for key in ("data", "color0", "color1"):
                if key in w:
                    w[key] = np.clip(np.asarray(w[key], np.float32), 0.0, 1.0)
        value, edge = gt.texture_eval(w, self.uv)
        self.edge = np.minimum(self.edge, edge)
        out = value @ LUMINANCE if np.asarray(w.get("data", 0.0)).ndim == 3 else value[:, 0]
        return out if self.mutation in ("no_clamp", "clamp_before_interpolation") else np.clip(out, 0.0, 1.0)

    def _bind(self, tree):
        node = {"kind": tree["kind"]}
        if tree["kind"] in _PARAMS:
            node.update({name: self._colour(tree[name]) for name in _PARAMS[tree["kind"]]})
            return node
        children = list(tree["children"])
        if self.mutation == {"blend": "children_exchanged", "twosided": "sides_exchanged"}[tree["kind"]]:
            children = children[::-1]
        node["children"] = [self._bind(c) for c in children]
        if tree["kind"] == "blend":
            node["weight"] = self._weight(tree["weight"])
        return node

    # ---- leaves
    @staticmethod
    def _eval_rpv(b, wi, wo):
        """rpv.cpp:107-141: the BRDF (the BRF over pi), no cosine"""
        with np.errstate(invalid="ignore", divide="ignore"):
            sin1, sin2 = np.hypot(wi[:, 0], wi[:, 1]), np.hypot(wo[:, 0], wo[:, 1])
            cos1, cos2 = wi[:, 2], wo[:, 2]
            # cos(phi1 - phi2) from the tangential parts (frame.h:107-118 clamps a degenerate azimuth to (1, 0): its factor sin is 0 then)
            dphi = np.where((sin1 > 0) & (sin2 > 0), (wi[:, 0] * wo[:, 0] + wi[:, 1] * wo[:, 1]) / (sin1 * sin2), 1.0)
            tan1, tan2 = sin1 / cos1, sin2 / cos2
            G = np.sqrt(np.maximum(tan1 ** 2 + tan2 ** 2 - 2.0 * tan1 * tan2 * dphi, 0.0))
            cos_g = (cos1 * cos2 + sin1 * sin2 * dphi)[:, None]
            g, k = b["g"], b["k"]
            F = (1.0 - g ** 2) / (1.0 + g ** 2 + 2.0 * g * cos_g) ** 1.5
            P = (cos1 * cos2 * (cos1 + cos2))[:, None] ** (k - 1.0)
            return b["rho_0"] * (P * F * (1.0 + (1.0 - b["rho_c"]) / (1.0 + G)[:, None])) * INV_PI

    @staticmethod
    def _bilambertian_weight(b):
        """bilambertian.cpp:82-89: hmean(r / (r + t)), 0 where r = t = 0"""
        with np.errstate(invalid="ignore", divide="ignore"):
            rw = np.mean(b["reflectance"] / (b["reflectance"] + b["transmittance"]), axis=1)
        return np.where(np.isnan(rw), 0.0, rw)

    def _leaf_eval_pdf(self, b, wi, wo):
        kind = b["kind"]
        if kind == "bilambertian":                                         # bilambertian.cpp:121-193
            same = np.signbit(wi[:, 2]) == np.signbit(wo[:, 2])
            val = np.where(same[:, None], b["reflectance"], b["transmittance"]) * (INV_PI * np.abs(wo[:, 2]))[:, None]
            rw = self._bilambertian_weight(b)
            return val, INV_PI * np.abs(wo[:, 2]) * np.where(same, rw, 1.0 - rw)
        active = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        pdf = np.where(active, INV_PI * wo[:, 2], 0.0)                     # diffuse.cpp:122-135, rpv.cpp:157-167
        if kind == "diffuse":                                              # diffuse.cpp:106-120
            return np.where(active[:, None], b["reflectance"] * (INV_PI * wo[:, 2])[:, None], 0.0), pdf
        return np.where(active[:, None], self._eval_rpv(b, wi, wo) * np.abs(wo[:, 2])[:, None], 0.0), pdf     # rpv.cpp:143-155

    def _leaf_sample(self, b, wi, s1, s2):
        kind, out = b["kind"], Sample(self.n)
        wo = square_to_cosine_hemisphere(s2)
        pdf = INV_PI * wo[:, 2]
        if kind == "bilambertian":                                         # bilambertian.cpp:64-119
            rw = self._bilambertian_weight(b)
            reflect = s1 < rw
            with np.errstate(invalid="ignore", divide="ignore"):
                value = np.where(reflect[:, None], b["reflectance"] / rw[:, None], b["transmittance"] / (1.0 - rw)[:, None])
            out.pdf = pdf * np.where(reflect, rw, 1.0 - rw)
            z = np.where(wi[:, 2] > 0, wo[:, 2], -wo[:, 2])
            out.wo = np.c_[wo[:, :2], np.where(reflect, z, -z)]
            out.weight = np.where((out.pdf > 0)[:, None], value, 0.0)
            out.threshold = np.abs(s1 - rw)
            out.tags["bilambertian_lobe"] = np.where(reflect, 0, 1)
            return out
        active = wi[:, 2] > 0
        if kind == "diffuse":                                              # diffuse.cpp:78-104
            out.wo, out.pdf = np.where(active[:, None], wo, 0.0), np.where(active, pdf, 0.0)
            out.weight = np.where((active & (pdf > 0))[:, None], b["reflectance"], 0.0)
            return out
        # rpv.cpp:85-105: the weight is the BRDF's value, NOT pi times it (f cos / pdf would be): kept as the reference has it
        value = self._eval_rpv(b, wi, wo) * (np.pi if self.mutation == "rpv_weight_times_pi" else 1.0)
        out.wo, out.pdf = wo, pdf
        out.weight = np.where((active & (pdf > 0))[:, None], value, 0.0)
        return out

    # ---- inner nodes
    def _eval_pdf(self, node, wi, wo):
        kind = node["kind"]
        if kind == "blend":                                                # blendbsdf.cpp:126-160
            w = node["weight"]
            (v0, p0), (v1, p1) = (self._eval_pdf(c, wi, wo) for c in node["children"])
            return v0 * (1.0 - w)[:, None] + v1 * w[:, None], p0 * (1.0 - w) + p1 * w
        if kind == "twosided":                                             # twosided.cpp:128-181: the side by the sign of wi.z, both z negated behind
            flip = np.array([1.0, 1.0, -1.0])
            front, back = wi[:, 2] > 0, wi[:, 2] < 0
            v0, p0 = self._eval_pdf(node["children"][0], wi, wo)
            v1, p1 = self._eval_pdf(node["children"][-1], wi * flip, wo * flip)
            return np.where(front[:, None], v0, np.where(back[:, None], v1, 0.0)), np.where(front, p0, np.where(back, p1, 0.0))
        return self._leaf_eval_pdf(node, wi, wo)

    def _sample(self, node, wi, s1, s2):
        kind = node["kind"]
        if kind == "blend":                                                # blendbsdf.cpp:103-123
            w = node["weight"]
            first = s1 > w
            with np.errstate(invalid="ignore", divide="ignore"):
                rescaled = np.where(first, (s1 - w) / (1.0 - w), s1 / w)
            if self.mutation == "unrescaled_sample1":
                rescaled = s1
            a, b = self._sample(node["children"][0], wi, rescaled, s2), self._sample(node["children"][1], wi, rescaled, s2)
            out = Sample(self.n).select(first, a, b)                       # the child's sample and weight, unchanged: bs.pdf is the CHILD's density
            out.threshold = np.minimum(out.threshold, np.abs(s1 - w))
            out.tags["blend_child"] = np.where(first, 0, 1)
            if self.mutation == "mixture_pdf":
                out.pdf = np.where(out.pdf > 0, self._eval_pdf(node, wi, out.wo)[1], 0.0)
            return out
        if kind == "twosided":                                             # twosided.cpp:94-126
            flip = np.array([1.0, 1.0, -1.0])
            front, back = wi[:, 2] > 0, wi[:, 2] < 0
            a, b = self._sample(node["children"][0], wi, s1, s2), self._sample(node["children"][-1], wi * flip, s1, s2)
            if self.mutation != "wo_not_flipped_back":
                b.wo = b.wo * flip
            out = Sample(self.n).select(front, a, b)
            neither = ~front & ~back                                       # :109: the zero sample
            out.wo[neither], out.pdf[neither], out.weight[neither] = 0.0, 0.0, 0.0
            out.tags["twosided_side"] = np.where(front, 0, np.where(back, 1, -1))
            return out
        return self._leaf_sample(node, wi, s1, s2)

    def eval_pdf(self, wi, wo):
        return self._eval_pdf(self.root, wi, wo)

    def sample(self, wi, s1, s2):
        return self._sample(self.root, wi, s1, s2)


# ================================================================ the one-surface sample of `path` and `volpath`
# The draws that precede the emitter sample's next_2d (decided by test_bsdf_tree_ref.py's comparison with the oracle, not guessed):
# `path` (path.cpp:100-211): none.  `volpath` (volpath.cpp:38-257), rgb: the channel (:63-67) and the loop's unconditional roulette
# draw (:86-91); mono: the roulette draw alone.  Then next_2d (emitter), next_1d and next_2d (BSDF) -- five uniforms.
STREAM_OFFSET = {("path", False): 0, ("path", True): 0, ("volpath", False): 2, ("volpath", True): 1}


def lane_uniforms(base_seed, seed_offset, n, count=8):
    """the first uniforms of the PCG32 streams seeded base_seed + seed_offset + i: what lane i of SamplingIntegrator::sample draws"""
    out = np.zeros((n, count), np.float32)
    row = np.zeros(count, np.float32)
    L = ob.lib()
    for i in range(n):
        L.oracle_sampler_stream(int(base_seed), int(seed_offset) + i, count, row.ctypes.data_as(ob.fp))
        out[i] = row
    return out.astype(np.float64)


def local_directions(normal, dp_du, v):
    """v in the shading frame of a hit (interaction.h:571-596): s = dp_du made orthogonal to the normal, t = n x s.  The frame matters:
    a sampled direction is made in it, and rpv's value depends on the azimuth between that direction and wi."""
    s = dp_du - normal * np.sum(normal * dp_du, axis=1)[:, None]
    s /= np.linalg.norm(s, axis=1)[:, None]
    t = np.cross(normal, s)
    return np.c_[np.sum(v * s, axis=1), np.sum(v * t, axis=1), np.sum(v * normal, axis=1)]


def surface_dp_du(surface, p, uv):
    """dp/du of the surfaces of tests/test_gpu_textures.py at their own (group-space) points p, float64"""
    m = gt.mat(gt.RECT_XF)[:3, :3]
    if surface == "rectangle":                                             # rectangle.cpp:66-74: to_world * (2, 0, 0)
        return np.tile(2.0 * m[:, 0], (len(p), 1))
    if surface == "disk":                                                  # disk.cpp:190-207: the radial direction
        phi = 2.0 * np.pi * uv[:, 1]
        return np.c_[np.cos(phi), np.sin(phi), np.zeros(len(p))] @ m.T
    # mesh.cpp:499-520: from the face's texture coordinates
    assert surface == "quad_uv"
    out = np.zeros((len(p), 3))
    found = np.zeros(len(p), bool)
    for face in gt.QUAD_FACES:
        v, t = gt.QUAD.astype(np.float64)[face], gt.QUAD_UV.astype(np.float64)[face]
        dp0, dp1 = v[1] - v[0], v[2] - v[0]
        b = np.linalg.lstsq(np.c_[dp0, dp1], (p - v[0]).T, rcond=None)[0].T              # the barycentric coordinates in this face
        inside = (b[:, 0] > 0) & (b[:, 1] > 0) & (b.sum(axis=1) < 1) & ~found
        duv0, duv1 = t[1] - t[0], t[2] - t[0]
        det = duv0[0] * duv1[1] - duv0[1] * duv1[0]
        out[inside] = (duv1[1] * dp0 - duv0[1] * dp1) / det
        found |= inside
    assert found.all()
    return out


class Lanes:
    """what the restatement says about every lane of a case: the value, its two terms, and what decides whether a lane is kept"""


def sheet_sample(evaluator, normal, dp_du, directions, uniforms, integrator="path", mono=False, reaches_sky=None):
    """One sample per lane: rays of direction `directions` (the fp32 values, as float64) that hit a sheet of unit normal `normal`
    at the evaluator's uv, under the `constant` emitter SKY, max_depth = 3, no roulette.  path.cpp:100-211 as path_sample orders it:
      emitter term  mis_weight(ds.pdf, bsdf.pdf) * bsdf.eval * L / ds.pdf       when ds.pdf != 0   (constant.cpp:81-117: 1 / 4 pi)
      BSDF term     mis_weight(bs.pdf, 1 / 4 pi) * weight * L                   the new ray leaves a flat sheet and meets the sky
    reaches_sky(local directions) -> (mask, margin): for the one case with a second, black surface (backdrop_case): whether a ray
    that leaves the hit meets the sky -- the shadow test of the emitter sample and the hit of the BSDF-sampled ray"""
    k = STREAM_OFFSET[(integrator, bool(mono))]
    u = np.asarray(uniforms, np.float64)
    L = f32(SKY)
    if mono:
        L = np.full(3, L @ LUMINANCE)
    wi = local_directions(normal, dp_du, -np.asarray(directions, np.float64))
    wo_e = local_directions(normal, dp_du, square_to_uniform_sphere(u[:, k:k + 2]))
    f, bpdf = evaluator.eval_pdf(wi, wo_e)
    out = Lanes()
    out.emitter_term = mis_weight(np.full(len(u), INV_FOUR_PI), bpdf)[:, None] * f * (L / INV_FOUR_PI)
    bs = evaluator.sample(wi, u[:, k + 2], u[:, k + 3:k + 5])
    out.bsdf_term = mis_weight(bs.pdf, INV_FOUR_PI)[:, None] * bs.weight * L
    clear = np.full(len(u), np.inf)
    if reaches_sky is not None:
        (seen_e, clear_e), (seen_b, clear_b) = reaches_sky(wo_e), reaches_sky(bs.wo)
        out.emitter_term, out.bsdf_term = out.emitter_term * seen_e[:, None], out.bsdf_term * seen_b[:, None]
        clear = np.minimum(clear_e, clear_b)
    out.value = out.emitter_term + out.bsdf_term
    out.tags = bs.tags
    out.kept = (bs.threshold >= THRESHOLD_MARGIN) & (np.abs(wo_e[:, 2]) >= HORIZON_MARGIN) \
        & ((np.abs(bs.wo[:, 2]) >= HORIZON_MARGIN) | (bs.pdf == 0)) & (evaluator.edge >= gt.MARGIN) & (np.abs(wi[:, 2]) >= WI_MARGIN) & (clear >= HORIZON_MARGIN)
    return out


def device_bound(placement):
    """the bound on scaled_error of a device value: instanced sheets against the world-space scale"""
    return DEVICE_FACTOR * (E_WORLD if placement in ("placed", "mirrored") else E_CANONICAL)


def exceeds_bound(name, placement, got, expected):
    """per lane: whether `got` leaves the restatement's `expected` by more than the device test allows for tree `name` --
    gt.ATOL absolute for the bilinear trees, device_bound() on scaled_error for all others"""
    if name in BILINEAR:
        return np.abs(np.asarray(got, np.float64) - expected).max(axis=1) > gt.ATOL
    return scaled_error(got, expected).max(axis=1) > device_bound(placement)


def scaled_error(got, expected):
    """|got - expected| / (|expected| + mean(SKY)): relative where a value is sizeable, absolute at the emitter's scale near zero"""
    return np.abs(np.asarray(got, np.float64) - expected) / (np.abs(expected) + float(f32(SKY).mean()))


# ================================================================ surfaces, placements and rays
BACKDROP_HEIGHT, BACKDROP_SIZE = 0.4, 1.6
PLACE_MIRRORED = shared.PLACE @ T.scale([1.0, 1.0, -1.0])
SURFACES = ("rectangle", "disk", "quad_uv")
PLACEMENTS = {"placed": shared.PLACE, "mirrored": PLACE_MIRRORED}


def placement_matrix(placement):
    """float64, from the definitions (tests/test_gpu_instance.place_matrix); the mirror is exact"""
    M = shared.place_matrix()
    return M @ np.diag([1.0, 1.0, -1.0, 1.0]) if placement == "mirrored" else M


class Case:
    pass


def build_case(tree, surface, placement=None, expanded=False, integrator="path", n=N_LANES, backdrop=False):
    """A sheet with the tree as its BSDF and n rays onto it, lanes taking turns between the two sides, tilted off the normal as
    tests/test_gpu_twosided.sheet_case tilts them.  placement: the sheet is the one member of a group instanced under PLACE or
    its mirror image; expanded: the same world-space sheet as a plain shape (what the oracle can load).  Hit points keep
    gt.MARGIN from every discontinuity of the tree's textures and 0.02 from the surface's seams.
    backdrop (the plain rectangle only): every ray meets the BACK of the sheet, and a black rectangle stands 0.4 before its front,
    1.6 times its size.  No light reaches the backdrop along a path that carries any -- what the sheet reflects backwards leaves
    backwards -- so the value is that of the sheet alone; but a sampled wo that is not negated back after a back-side hit runs into
    it.  Without it nothing on a single sheet under a constant sky can tell where a sampled ray goes."""
    if placement == "backdrop":
        placement, backdrop = None, True
    shape, p, uv, normal, seam = gt.SURFACES[surface](8 * n, np.random.default_rng(2024))      # the same points whichever cases run
    edge = Evaluator(tree, uv).edge
    keep = np.flatnonzero((edge >= gt.MARGIN) & (seam >= 0.02))[:n]
    assert len(keep) == n, "not enough hit points away from the discontinuities"
    p, uv, normal = p[keep], uv[keep], normal[keep]
    dp_du = surface_dp_du(surface, p, uv)
    shape = dict(shape, bsdf=bsdf_dict(tree))
    c = Case()
    if placement:
        M = placement_matrix(placement)
        assert np.allclose(np.asarray(PLACEMENTS[placement].matrix, np.float64), M, atol=1e-6)
        p = p @ M[:3, :3].T + M[:3, 3]
        dp_du = dp_du @ M[:3, :3].T                                         # dp_du as a vector
        normal = normal @ np.linalg.inv(M[:3, :3])                          # instance.cpp:134-143: normals through the inverse transpose
        normal /= np.linalg.norm(normal, axis=1)[:, None]
        if expanded and shape["type"] == "mesh":
            v = shape["vertex_positions"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
            shape["vertex_positions"] = v.astype(np.float32)
            if placement == "mirrored":
                normal = -normal                                            # mesh.cpp:485-497: a plain mesh's normal is its world-space winding's
        elif expanded:
            shape["to_world"] = PLACEMENTS[placement] @ shape["to_world"]
        else:
            shape = {"type": "instance", "to_world": PLACEMENTS[placement], "group": {"type": "shapegroup", "member": shape}}
    # three lanes of four meet the front, the fourth the back: a one-sided tree is dark from behind, and a reflecting one has no
    # emitter term for half the emitter samples, so an even split would leave only a quarter of the lanes with both terms
    sign = np.where(np.arange(n) % 4 != 3, 1.0, -1.0)[:, None]
    c.reaches_sky = None
    if backdrop:
        assert surface == "rectangle" and not placement
        sign = np.full((n, 1), -1.0)
        xf = gt.RECT_XF @ T.translate([0.0, 0.0, BACKDROP_HEIGHT])
        c.backdrop = {"type": "rectangle", "to_world": xf @ T.scale([BACKDROP_SIZE, BACKDROP_SIZE, 1.0]), "bsdf": {"type": "diffuse", "reflectance": 0.0}}
        assert np.abs(np.c_[[-1, 1, 1, -1], [-1, -1, 1, 1], [0] * 4, [1] * 4] * [BACKDROP_SIZE, BACKDROP_SIZE, 1, 1] @ gt.mat(xf).T).max() <= 4.0
        to_sheet = np.linalg.inv(gt.mat(gt.RECT_XF)[:3, :3])
        at = 2.0 * uv - 1.0                                                  # rectangle.cpp:205: the hit in the rectangle's own coordinates
        s = dp_du - normal * np.sum(normal * dp_du, axis=1)[:, None]
        s /= np.linalg.norm(s, axis=1)[:, None]
        t = np.cross(normal, s)

        def reaches_sky(w):
            """a ray from the hit in the shading-frame direction w against the backdrop, in the rectangle's own coordinates"""
            d = (w[:, :1] * s + w[:, 1:2] * t + w[:, 2:] * normal) @ to_sheet.T
            with np.errstate(invalid="ignore", divide="ignore"):
                q = at + d[:, :2] * (BACKDROP_HEIGHT / d[:, 2])[:, None]
            inside = np.abs(q).max(axis=1) - BACKDROP_SIZE                   # < 0: the ray meets the backdrop
            towards = d[:, 2] > 0
            return ~(towards & (inside < 0)), np.where(towards, np.abs(inside), np.inf)
        c.reaches_sky = reaches_sky
    towards = normal * sign
    tilt = towards + 0.3 * np.cross(towards, [0.3, 0.5, 0.8])
    tilt /= np.linalg.norm(tilt, axis=1)[:, None]
    c.origins, c.directions = (p + 1.5 * tilt).astype(np.float32), (-tilt).astype(np.float32)
    assert np.abs(np.r_[c.origins.ravel(), p.ravel()]).max() <= 4.0         # E is measured for coordinates <= 4
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    c.scene = {"type": "scene", "integrator": {"type": integrator, "max_depth": 3},
               "sensor": {"type": "mradiancemeter", "origins": fmt(c.origins[:N_FILM]), "directions": fmt(c.directions[:N_FILM]),
                          "film": {"type": "hdrfilm", "width": N_FILM, "height": 1, "rfilter": {"type": "box"}},
                          "sampler": {"type": "independent", "sample_count": 4}},
               "sheet": shape,
               "sky": {"type": "constant", "radiance": {"type": "rgb", "value": [float(x) for x in SKY]}}}
    if backdrop:
        c.scene["backdrop"] = c.backdrop
    c.tree, c.uv, c.normal, c.dp_du, c.n, c.integrator = tree, uv, normal, dp_du, n, integrator
    return c


def with_thin_medium(scene):
    """tests/test_gpu_twosided.sheet_case(medium=True): a medium of no effect (optical depth < 1e-7) puts `volpath` on its ring row"""
    d = dict(scene, integrator=dict(scene["integrator"], type="volpath"))
    xf = T.translate([-8, -8, -8]) @ T.scale(16.0)
    grid = lambda v: {"type": "gridvolume", "data": np.full((2, 2, 2), v, np.float32), "to_world": xf}
    d["air"] = {"type": "cube", "to_world": T.scale(8.0), "bsdf": {"type": "null"},
                "interior": {"type": "heterogeneous", "sigma_t": grid(1e-9), "albedo": grid(0.5), "phase": {"type": "isotropic"}}}
    return d


_SEED = []


def base_seed():
    """sensor.seed of these scenes (the sampler's default): the same for every case"""
    if not _SEED:
        _SEED.append(int(SD.build_scene_desc(build_case(diffuse(0.5), "rectangle", n=N_FILM).scene)[0].sensor.sampler_seed))
    return _SEED[0]


_UNIFORMS = {}


def case_uniforms(n=N_LANES):
    if n not in _UNIFORMS:
        _UNIFORMS[n] = lane_uniforms(base_seed(), SEED_OFFSET, n)
    return _UNIFORMS[n]


def restate(case, integrator=None, mono=False, mutation=None):
    ev = Evaluator(case.tree, case.uv, mono=mono, mutation=mutation)
    return sheet_sample(ev, case.normal, case.dp_du, case.directions.astype(np.float64), case_uniforms(case.n), integrator or case.integrator, mono, case.reaches_sky)


# ================================================================ the catalogue
def _nearest(data, **kw):
    return dict({"type": "bitmap", "data": np.asarray(data, np.float32), "filter_type": "nearest", "to_uv": gt.UV23}, **kw)


RGB44 = _nearest(gt.B44C)                                                  # 4 x 4 rgb texels in [0, 1)
RGB53 = _nearest(0.8 * gt.B53, wrap_mode="clamp")                          # 5 x 3
RGB44_DIM = _nearest(0.6 * gt.B44C, wrap_mode="mirror")                    # a reflectance beside a transmittance of 0.3
W44 = _nearest(gt.B44, wrap_mode="mirror")                                 # one channel, in [0, 1)
W_CLAMPED = shared.WEIGHTS["nearest_clamped"]                                  # texels -0.5 / 1.5 / 0.25 / 0.75 / 0.5, nearest
W_CHECKER = shared.WEIGHTS["checkerboard"]                                     # 0.8 / 0.1
RPV_A = rpv([0.12, 0.34, 0.21], 0.75, -0.15, [0.3, 0.5, 0.2])
RPV_B = rpv([0.25, 0.18, 0.4], 1.2, 0.1, 0.6)
D0, D1 = diffuse([0.15, 0.55, 0.35]), diffuse([0.85, 0.25, 0.6])
BILAMB = bilambertian([0.5, 0.3, 0.4], [0.2, 0.35, 0.1])

CATALOGUE = {
    "blend_dtex_rpv": blend(diffuse(RGB44), RPV_A, 0.3),
    "blend_rpvtex_d_wtex": blend(rpv(RGB53, 0.75, -0.15, [0.3, 0.5, 0.2]), D1, W44),
    "blend_d_bilamb": blend(D0, BILAMB, 0.6),                              # children of different sampling densities
    "blend_bilambtex_rpv_wchecker": blend(bilambertian(RGB44_DIM, 0.3), RPV_B, W_CHECKER),
    "blend_d_d_wclamped": blend(D0, D1, W_CLAMPED),
    "twosided_rpv": twosided(RPV_A),
    "twosided_rpv_dchecker": twosided(RPV_B, diffuse(gt.CHECKER)),
    "twosided_blend_rpvtex": twosided(blend(RPV_A, D1, W44), rpv(RGB53, 1.2, 0.1, 0.6)),
    "twosided_d_blend": twosided(D0, blend(diffuse(RGB44), RPV_B, 0.4)),
}
# held to gt.ATOL: a bilinear colour, and (for the clamp-before-interpolation mutation, which a nearest lookup cannot show) a bilinear weight
BILINEAR = {
    "blend_dbilinear_rpv": blend(diffuse(gt.TEXTURES["b44rgb_bilinear_clamp"]), RPV_A, 0.3),
    "blend_d_d_wbilinear": blend(D0, D1, dict(W_CLAMPED, filter_type="bilinear")),
}
# grey parameters, for the mono variant
GREY = {
    "grey_blend": blend(diffuse(W44), rpv(0.3, 0.75, -0.15, 0.5), 0.3),
    "grey_twosided": twosided(rpv(0.3, 1.2, 0.1, 0.6), diffuse({"type": "checkerboard", "color0": 0.7, "color1": 0.15, "to_uv": T.scale([4.0, 4.0, 1.0])})),
}
ALL_TREES = dict(CATALOGUE, **BILINEAR, **GREY)
# (surface, placement): the plain sheets, and the rectangle and the quad inside an instance and inside its mirror image
SHEETS = [(s, None) for s in SURFACES] + [(s, p) for s in ("rectangle", "quad_uv") for p in ("placed", "mirrored")]
# the sheet met from behind with a black backdrop before its front (build_case): where a sampled ray goes
BACKDROP_CASES = [("twosided_rpv", "rectangle", "backdrop"), ("twosided_blend_rpvtex", "rectangle", "backdrop")]
# the plain leaves the oracle can speak about (section a)
LEAVES = {"diffuse": D0, "rpv": RPV_A, "bilambertian": BILAMB}
GREY_LEAVES = {"diffuse": diffuse(0.45), "rpv": rpv(0.3, 0.75, -0.15, 0.5), "bilambertian": bilambertian(0.5, 0.25)}


def expected_branches(tree):
    """the branches a tree is meant to reach on kept lanes: tag -> the values that must occur"""
    out = {}

    def walk(t):
        if t["kind"] == "blend":
            out["blend_child"] = {0, 1}
        if t["kind"] == "twosided":
            out["twosided_side"] = {0, 1}
        if t["kind"] == "bilambertian":
            out["bilambertian_lobe"] = {0, 1}
        for c in t.get("children", []):
            walk(c)
    walk(tree)
    return out
