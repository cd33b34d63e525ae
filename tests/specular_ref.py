"""A float64 restatement of one `path` / `volpath` sample on a single flat sheet whose BSDF is a smooth `dielectric` or `conductor`
(alone, or under `twosided`), under the chromatic constant sky of tests/bsdf_tree_ref.py.  TEST INFRASTRUCTURE: plain numpy, no
device code; the reference's sources are cited by file and line and are never read at run time.

Why it exists: the CPU oracle knows neither plugin, so fresnel_dielectric, fresnel_conductor, reflect, refract, dielectric_sample and
conductor_sample of csrc/integrator_dev.h have no bit-level reference.  On one sheet under a `constant` emitter at max_depth = 3 a
lane is a closed function of the ray and of sample1:

    dielectric, transmitted   SKY * specular_transmittance * eta_ti^2
    dielectric, reflected     SKY * specular_reflectance
    conductor                 SKY * specular_reflectance * F(cos theta)          (0 from behind: the path ends)

A delta lobe has eval = pdf = 0, so the emitter sample of a hit contributes nothing, and the sky the sampled ray meets counts in
full (the integrators' MIS weight of a delta sample is 1).  The emitter sample is still DRAWN wherever the hit's own record has a
smooth lobe (twosided.cpp:78-88: the adapter's union over both sides): `twosided(conductor, diffuse)` draws it on the mirror's side
as well, which moves sample1 two uniforms down the stream.

The formulas are written from the physics, not in the reference's order of operations: Snell's law for sin(theta_t), the amplitude
ratios in their sin / cos form, the refracted direction as eta d + (eta cos(theta_i) - cos(theta_t)) n, and the conductor's
reflectance from complex arithmetic with epsilon = (eta + i k)^2 in complex128.  fp32_value() is the other thing: the reference's
statements (fresnel.h:33-116, dielectric.cpp:201-310, conductor.cpp:217-270) in numpy float32, in their order -- the scale E_SPEC of
what single precision does to these formulas is its distance from the float64 restatement, measured on the CPU.

Sheets, lanes, streams and the seed offset are those of tests/bsdf_tree_ref.py, by import.  The rays are this file's own: the angle of
incidence runs from the normal down to cos(theta) = 0.05, from above and from below, so total internal reflection is on every
dielectric sheet that has a denser side.

What is NOT restated: `volpathmis`, area emitters, wi.z == 0, a second bounce.  Two conceivable mutations change no value on one
sheet under a uniform sky and are therefore not in MUTATIONS: `sample1 < r` against `<=` (a set of measure zero), and the emitter sample
not drawn on the mirror's side of `twosided(conductor, diffuse)` -- a conductor reads no uniform, so a shifted stream moves nothing
there; the row tests of tests/test_gpu_specular.py put a diffuse plate before that mirror, where the stream does matter."""
import numpy as np

import tests.bsdf_tree_ref as R
import tests.test_gpu_textures as gt

f32 = R.f32

# ---- the fp32 scale: max over every case's kept lanes and channels of scaled_error(fp32_value, restatement), MEASURED ON THE CPU
# (tests/test_specular.py prints and re-measures it) and rounded up to two digits.  Nothing measured on the device enters it.
E_SPEC = 3.4e-7             # measured 3.35e-7 (the rgb conductor; the dielectric cases stay under 6.1e-8)
DEVICE_FACTOR = R.DEVICE_FACTOR
THRESHOLD_MARGIN = R.THRESHOLD_MARGIN       # |sample1 - r_i|
TIR_MARGIN = 1e-4                           # |sin(theta_t) - 1|: around the critical angle the lobe is decided by the last bit of cos(theta_i)
MAX_DROP = R.MAX_DROP
COS_MIN = 0.05                              # the most grazing ray
SEED_OFFSET = R.SEED_OFFSET
N_LANES, N_FILM = R.N_LANES, R.N_FILM

MUTATIONS = ("no_eta_ti_squared", "eta_exchanged_inside", "cos_theta_t_sign", "k_ignored", "conductor_from_behind")


# ================================================================ the description of a tree
def dielectric(int_ior, ext_ior, reflectance=None, transmittance=None):
    return {"kind": "dielectric", "int_ior": int_ior, "ext_ior": ext_ior, "reflectance": reflectance, "transmittance": transmittance}


def conductor(eta=None, k=None, reflectance=None):
    return {"kind": "conductor", "eta": eta, "k": k, "reflectance": reflectance}


def bsdf_dict(tree):
    kind = tree["kind"]
    if kind == "dielectric":
        out = {"type": "dielectric", "int_ior": float(tree["int_ior"]), "ext_ior": float(tree["ext_ior"])}
        for key, name in (("reflectance", "specular_reflectance"), ("transmittance", "specular_transmittance")):
            if tree[key] is not None:
                out[name] = R._param_dict(tree[key])
        return out
    if kind == "conductor":
        out = {"type": "conductor"}
        for key, name in (("eta", "eta"), ("k", "k"), ("reflectance", "specular_reflectance")):
            if tree[key] is not None:
                out[name] = R._param_dict(tree[key])
        return out
    if kind == "twosided":
        out = {"type": "twosided", "brdf_a": bsdf_dict(tree["children"][0])}
        if len(tree["children"]) == 2:
            out["brdf_b"] = bsdf_dict(tree["children"][1])
        return out
    return R.bsdf_dict(tree)


def has_smooth_lobe(tree):
    """whether the record of a hit has a smooth lobe: a twosided's flags are the union over its sides (twosided.cpp:78-88)"""
    if tree["kind"] in ("dielectric", "conductor"):
        return False
    if tree["kind"] == "twosided":
        return any(has_smooth_lobe(c) for c in tree["children"])
    return True


def stand_in(tree):
    """a tree of bsdf_tree_ref's own kinds with the same textures: what R.build_case keeps the hit points clear of"""
    if tree["kind"] == "twosided":
        return R.twosided(*[stand_in(c) for c in tree["children"]])
    if tree["kind"] == "dielectric":
        return R.bilambertian(tree["reflectance"] if R._is_texture(tree["reflectance"]) else 0.5,
                              tree["transmittance"] if R._is_texture(tree["transmittance"]) else 0.5)
    if tree["kind"] == "conductor":
        return R.diffuse(tree["reflectance"] if R._is_texture(tree["reflectance"]) else 0.5)
    return tree


# ================================================================ the physics, float64
def fresnel_dielectric(cos_i, eta, mutation=None):
    """unpolarised reflectance of a smooth interface met at cos_i (its sign: the side; eta = n_below / n_above for cos_i > 0 above),
    with the cosine of the refracted ray and the relative index along the direction of travel.  Snell: sin_t = sin_i / eta_it."""
    outside = cos_i >= 0
    if mutation == "eta_exchanged_inside":
        outside = np.ones_like(outside)
    eta_it = np.where(outside, eta, 1.0 / eta)                            # n_t / n_i
    ci = np.abs(cos_i)
    sin_i = np.sqrt(np.maximum(1.0 - ci * ci, 0.0))
    sin_t = sin_i / eta_it
    tir = sin_t >= 1.0
    cos_t = np.sqrt(np.maximum(1.0 - sin_t * sin_t, 0.0))
    theta_i, theta_t = np.arctan2(sin_i, ci), np.arctan2(sin_t, cos_t)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_s = -np.sin(theta_i - theta_t) / np.sin(theta_i + theta_t)
        r_p = np.sin(theta_i - theta_t) * np.cos(theta_i + theta_t) / (np.cos(theta_i - theta_t) * np.sin(theta_i + theta_t))
        r = 0.5 * (r_s * r_s + r_p * r_p)
    normal = sin_i < 1e-9                                                 # the limit of both ratios at normal incidence
    r = np.where(normal, ((1.0 - eta_it) / (1.0 + eta_it)) ** 2, r)
    r = np.where(eta_it == 1.0, 0.0, r)                                   # no interface
    r = np.where(tir | (ci == 0), 1.0, r)
    return r, np.where(tir, 0.0, cos_t), eta_it, np.abs(sin_t - 1.0)


def fresnel_conductor(cos_i, eta, k):
    """|r_s|^2 and |r_p|^2 of a medium of complex index eta + i k met from vacuum, averaged"""
    eps = (np.asarray(eta, np.complex128) + 1j * np.asarray(k, np.complex128)) ** 2
    c = np.asarray(cos_i, np.complex128)
    root = np.sqrt(eps - (1.0 - c * c))
    with np.errstate(invalid="ignore", divide="ignore"):
        r_s = (c - root) / (c + root)
        r_p = (eps * c - root) / (eps * c + root)
    return 0.5 * (np.abs(r_s) ** 2 + np.abs(r_p) ** 2)


class Evaluator(R.Evaluator):
    """R.Evaluator with the two specular leaves.  mutation: one of MUTATIONS (or of R.MUTATIONS)"""

    def __init__(self, tree, uv, mono=False, mutation=None):
        self.spec_mutation = mutation if mutation in MUTATIONS else None
        self.margin = np.full(len(uv), np.inf)                            # distance of sin(theta_t) from 1
        super().__init__(tree, uv, mono=mono, mutation=None if mutation in MUTATIONS else mutation)

    def _scalar(self, v, default):
        """a conductor's eta / k: a constant; mono: the float32 luminance the loader keeps"""
        value = np.broadcast_to(f32(default if v is None else v), (3,)).astype(np.float64)
        if self.mono and not (value[0] == value[1] == value[2]):
            value = np.full(3, float(f32(value @ R.LUMINANCE)))
        return value

    def _bind(self, tree):
        kind = tree["kind"]
        if kind == "dielectric":
            eta = float(np.float32(tree["int_ior"]) / np.float32(tree["ext_ior"]))
            return {"kind": kind, "eta": eta, "reflectance": self._colour(1.0 if tree["reflectance"] is None else tree["reflectance"]),
                    "transmittance": self._colour(1.0 if tree["transmittance"] is None else tree["transmittance"])}
        if kind == "conductor":
            return {"kind": kind, "eta": self._scalar(tree["eta"], 0.0), "k": self._scalar(tree["k"], 1.0),
                    "reflectance": self._colour(1.0 if tree["reflectance"] is None else tree["reflectance"])}
        return super()._bind(tree)

    def _leaf_eval_pdf(self, b, wi, wo):
        if b["kind"] in ("dielectric", "conductor"):                       # delta lobes alone
            return np.zeros((self.n, 3)), np.zeros(self.n)
        return super()._leaf_eval_pdf(b, wi, wo)

    def _leaf_sample(self, b, wi, s1, s2):
        kind = b["kind"]
        if kind not in ("dielectric", "conductor"):
            out = super()._leaf_sample(b, wi, s1, s2)
            out.delta = np.zeros(self.n, bool)
            return out
        out = R.Sample(self.n)
        cos_i = wi[:, 2]
        d = -wi                                                            # the direction the light of this path travels backwards: towards the sheet
        if kind == "conductor":
            active = cos_i > 0
            if self.spec_mutation == "conductor_from_behind":
                active = cos_i != 0
            k = np.zeros(3) if self.spec_mutation == "k_ignored" else b["k"]
            F = np.stack([fresnel_conductor(np.abs(cos_i), b["eta"][c], k[c]) for c in range(3)], axis=1)
            n = np.array([0.0, 0.0, 1.0])
            mirrored = d - 2.0 * (d @ n)[:, None] * n
            out.wo, out.pdf = np.where(active[:, None], mirrored, 0.0), np.where(active, 1.0, 0.0)
            out.weight = np.where(active[:, None], b["reflectance"] * F, 0.0)
            out.tags["conductor_side"] = np.where(cos_i > 0, 0, 1)
            out.delta = np.ones(self.n, bool)
            return out
        r, cos_t, eta_it, margin = fresnel_dielectric(cos_i, b["eta"], self.spec_mutation)
        self.margin = np.minimum(self.margin, margin)
        reflect = s1 <= r
        n = np.c_[np.zeros(self.n), np.zeros(self.n), np.where(cos_i >= 0, 1.0, -1.0)]      # the normal against the travelling light
        ratio = 1.0 / eta_it                                                                 # n_i / n_t = eta_ti
        mirrored = d - 2.0 * np.sum(d * n, axis=1)[:, None] * n
        bent = ratio[:, None] * d + (ratio * np.abs(cos_i) - cos_t)[:, None] * n
        if self.spec_mutation == "cos_theta_t_sign":                       # the sign of the side seen from above, whichever side the ray meets
            bent[:, 2] = -np.abs(bent[:, 2])
        scale = 1.0 if self.spec_mutation == "no_eta_ti_squared" else (ratio * ratio)[:, None]
        out.wo = np.where(reflect[:, None], mirrored, bent)
        out.pdf = np.where(reflect, r, 1.0 - r)
        out.weight = np.where(reflect[:, None], b["reflectance"], b["transmittance"] * scale)
        out.threshold = np.abs(s1 - r)
        tir = (r == 1.0) & (cos_t == 0.0) & (cos_i != 0)
        out.tags["dielectric_branch"] = np.where(tir, 3, np.where(reflect, 0, np.where(cos_i > 0, 1, 2)))     # reflection, in, out, total internal reflection
        out.delta = np.ones(self.n, bool)
        return out

    def _sample(self, node, wi, s1, s2):
        if node["kind"] == "twosided":
            flip = np.array([1.0, 1.0, -1.0])
            a, b = self._sample(node["children"][0], wi, s1, s2), self._sample(node["children"][-1], wi * flip, s1, s2)
            out = super()._sample(node, wi, s1, s2)
            out.delta = np.where(wi[:, 2] > 0, a.delta, b.delta)
            return out
        if node["kind"] == "blend":
            out = super()._sample(node, wi, s1, s2)
            out.delta = np.zeros(self.n, bool)
            return out
        return self._leaf_sample(node, wi, s1, s2)


# ================================================================ the one-surface sample
def sheet_sample(evaluator, tree, normal, dp_du, directions, uniforms, integrator="path", mono=False, reaches_sky=None):
    """R.sheet_sample for a tree that may hold delta lobes: the emitter sample is drawn iff the hit's record has a smooth lobe, and a
    delta sample meets the sky with the weight 1 (path.cpp:195-199, volpath.cpp:232-238: no emitter pdf for a delta lobe)"""
    k = R.STREAM_OFFSET[(integrator, bool(mono))]
    u = np.asarray(uniforms, np.float64)
    L = f32(R.SKY)
    if mono:
        L = np.full(3, L @ R.LUMINANCE)
    n = len(u)
    wi = R.local_directions(normal, dp_du, -np.asarray(directions, np.float64))
    out = R.Lanes()
    out.emitter_term, horizon = np.zeros((n, 3)), np.full(n, np.inf)
    wo_e = None
    if has_smooth_lobe(tree):
        wo_e = R.local_directions(normal, dp_du, R.square_to_uniform_sphere(u[:, k:k + 2]))
        f, bpdf = evaluator.eval_pdf(wi, wo_e)
        out.emitter_term = R.mis_weight(np.full(n, R.INV_FOUR_PI), bpdf)[:, None] * f * (L / R.INV_FOUR_PI)
        horizon = np.abs(wo_e[:, 2])
        k += 2
    bs = evaluator.sample(wi, u[:, k], u[:, k + 1:k + 3])
    mis = np.where(bs.delta, (bs.pdf > 0).astype(np.float64), R.mis_weight(bs.pdf, R.INV_FOUR_PI))
    out.bsdf_term = mis[:, None] * bs.weight * L
    clear = np.full(n, np.inf)
    if reaches_sky is not None:
        seen_b, clear = reaches_sky(bs.wo)
        out.bsdf_term = out.bsdf_term * seen_b[:, None]
        if wo_e is not None:
            seen_e, clear_e = reaches_sky(wo_e)
            out.emitter_term, clear = out.emitter_term * seen_e[:, None], np.minimum(clear, clear_e)
    out.value = out.emitter_term + out.bsdf_term
    out.tags, out.wi, out.wo, out.delta = bs.tags, wi, bs.wo, bs.delta
    # a smooth lobe keeps R's margins (horizon of both sampled directions); a delta lobe needs neither: its direction is not compared
    smooth_ok = (np.abs(bs.wo[:, 2]) >= R.HORIZON_MARGIN) | (bs.pdf == 0) | bs.delta
    out.kept = (bs.threshold >= THRESHOLD_MARGIN) & (evaluator.margin >= TIR_MARGIN) & (horizon >= R.HORIZON_MARGIN) & smooth_ok \
        & (evaluator.edge >= gt.MARGIN) & (np.abs(wi[:, 2]) >= 0.5 * COS_MIN) & (clear >= R.HORIZON_MARGIN)
    return out


def scaled_error(got, expected):
    return R.scaled_error(got, expected)


def device_bound():
    return DEVICE_FACTOR * E_SPEC


# ================================================================ the reference's statements in float32
def _fma(a, b, c):
    """one rounding: the product and the sum in float64 (exact product of two float32), rounded once to float32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def fp32_fresnel(cos_i, eta):
    """fresnel.h:33-70, statement for statement, numpy float32"""
    one = np.float32(1.0)
    cos_i, eta = np.asarray(cos_i, np.float32), np.float32(eta)
    outside = cos_i >= 0
    rcp_eta = one / eta
    eta_it, eta_ti = np.where(outside, eta, rcp_eta).astype(np.float32), np.where(outside, rcp_eta, eta).astype(np.float32)
    cos_t_sqr = _fma(-_fma(-cos_i, cos_i, one), eta_ti * eta_ti, one)
    ci, ct = np.abs(cos_i), np.sqrt(np.maximum(cos_t_sqr, np.float32(0.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        a_s = _fma(-eta_it, ct, ci) / _fma(eta_it, ct, ci)
        a_p = _fma(-eta_it, ci, ct) / _fma(eta_it, ci, ct)
    r = np.float32(0.5) * (a_s * a_s + a_p * a_p)
    r = np.where((eta == one) | (ci == 0), np.float32(0.0) if eta == one else one, r).astype(np.float32)
    return r, np.where(cos_i >= 0, -ct, ct).astype(np.float32), eta_it, eta_ti


def fp32_fresnel_conductor(cos_i, eta_r, eta_i):
    """fresnel.h:91-116, statement for statement, numpy float32"""
    f = np.float32
    cos_i, eta_r, eta_i = np.asarray(cos_i, f), f(eta_r), f(eta_i)
    cos2 = cos_i * cos_i
    sin2 = f(1.0) - cos2
    sin4 = sin2 * sin2
    temp_1 = eta_r * eta_r - eta_i * eta_i - sin2
    a2pb2 = np.sqrt(np.maximum(temp_1 * temp_1 + f(4.0) * eta_i * eta_i * eta_r * eta_r, f(0.0)))
    a = np.sqrt(np.maximum(f(0.5) * (a2pb2 + temp_1), f(0.0)))
    term_1, term_2 = a2pb2 + cos2, f(2.0) * cos_i * a
    with np.errstate(invalid="ignore", divide="ignore"):
        r_s = (term_1 - term_2) / (term_1 + term_2)
        term_3, term_4 = a2pb2 * cos2 + sin4, term_2 * sin2
        r_p = r_s * (term_3 - term_4) / (term_3 + term_4)
    return (f(0.5) * (r_s + r_p)).astype(f)


def fp32_value(case, integrator=None, mono=False):
    """the value and the lobe (0 reflection, 1 transmission, -1 none) of every lane, in float32 in the reference's order: wi.z from the
    float32 normal and direction, then dielectric.cpp:201-310 / conductor.cpp:217-270.  Specular leaves (alone or under twosided) only:
    lanes that meet another kind of leaf come back NaN and are left out by the caller."""
    f = np.float32
    integrator = integrator or case.integrator
    u = R.case_uniforms(case.n)
    k = R.STREAM_OFFSET[(integrator, bool(mono))] + (2 if has_smooth_lobe(case.tree) else 0)
    s1 = u[:, k].astype(f)
    normal = case.normal.astype(f)
    d = -case.directions.astype(f)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    wi_z = dot(d, normal).astype(f)
    ev = Evaluator(case.tree, case.uv, mono=mono)
    L = R.SKY.astype(f)
    if mono:
        L = np.full(3, f(f32(R.SKY) @ R.LUMINANCE), f)
    value, lobe = np.full((case.n, 3), np.nan, f), np.full(case.n, -1)

    def leaf(node, z, where):
        if node["kind"] == "dielectric":
            r, cos_t, eta_it, eta_ti = fp32_fresnel(z, node["eta"])
            refl = s1 <= r
            w = np.where(refl[:, None], node["reflectance"].astype(f), node["transmittance"].astype(f) * (eta_ti * eta_ti)[:, None]).astype(f)
            value[where], lobe[where] = (w * L)[where], np.where(refl, 0, 1)[where]
        elif node["kind"] == "conductor":
            F = np.stack([fp32_fresnel_conductor(z, node["eta"][c], node["k"][c]) for c in range(3)], axis=1)
            active = z > 0
            w = np.where(active[:, None], node["reflectance"].astype(f) * F, f(0.0)).astype(f)
            value[where], lobe[where] = (w * L)[where], np.where(active, 0, -1)[where]

    root = ev.root
    if root["kind"] == "twosided":
        leaf(root["children"][0], wi_z, wi_z > 0)
        leaf(root["children"][-1], -wi_z, wi_z < 0)
    else:
        leaf(root, wi_z, np.ones(case.n, bool))
    return value, lobe


# ================================================================ cases
def build_case(tree, surface, placement=None, integrator="path", n=N_LANES):
    """R.build_case's sheet (its hit points, its placement, its sensor), with `tree` as the BSDF and rays of this file's own: lane i
    meets the sheet at cos(theta) spread evenly over [COS_MIN, 1] (in a scrambled order, so the 300 rays of the film span it too), three
    lanes of four from above and the fourth from below (R's split), at an azimuth of its own.  `backdrop`: R's case -- every ray
    meets the BACK, a black rectangle stands before the front -- with R's rays, which are steep enough to be refracted onto it."""
    c = R.build_case(stand_in(tree), surface, placement, integrator=integrator, n=n)
    holder = c.scene["sheet"]
    if holder["type"] == "instance":
        holder["group"]["member"] = dict(holder["group"]["member"], bsdf=bsdf_dict(tree))
    else:
        c.scene["sheet"] = dict(holder, bsdf=bsdf_dict(tree))
    c.tree = tree
    if placement == "backdrop":
        return c
    rng = np.random.default_rng(77)
    cos = COS_MIN + (1.0 - COS_MIN) * (rng.permutation(n) + 0.5) / n
    phi = 2.0 * np.pi * rng.random(n)
    sign = np.where(np.arange(n) % 4 != 3, 1.0, -1.0)
    s = c.dp_du - c.normal * np.sum(c.normal * c.dp_du, axis=1)[:, None]
    s /= np.linalg.norm(s, axis=1)[:, None]
    t = np.cross(c.normal, s)
    sin = np.sqrt(1.0 - cos * cos)
    towards = (sign * cos)[:, None] * c.normal + (sin * np.cos(phi))[:, None] * s + (sin * np.sin(phi))[:, None] * t
    p = c.origins.astype(np.float64) + 1.5 * c.directions.astype(np.float64)            # R's hit points, to float32 accuracy
    c.origins, c.directions = (p + 1.5 * towards).astype(np.float32), (-towards).astype(np.float32)
    fmt = lambda a: ", ".join("%.9g" % x for x in a.ravel())
    c.scene["sensor"] = dict(c.scene["sensor"], origins=fmt(c.origins[:N_FILM]), directions=fmt(c.directions[:N_FILM]))
    return c


def restate(case, integrator=None, mono=False, mutation=None):
    ev = Evaluator(case.tree, case.uv, mono=mono, mutation=mutation)
    return sheet_sample(ev, case.tree, case.normal, case.dp_du, case.directions.astype(np.float64), R.case_uniforms(case.n),
                        integrator or case.integrator, mono, case.reaches_sky)


GLASS = dielectric(1.5, 1.0)
BUBBLE = dielectric(1.0, 1.5)                                              # int_ior < ext_ior: the denser side is above
MATCHED = dielectric(1.0, 1.0, [0.9, 0.5, 0.7], [0.6, 0.8, 0.4])
GLASS_COLOURED = dielectric(1.5, 1.0, [0.9, 0.5, 0.7], [0.6, 0.8, 0.4])
GLASS_CHECKER = dielectric(1.33, 1.0, gt.CHECKER, R.RGB44)
MIRROR = conductor()
METAL = conductor([0.2, 0.9, 1.4], [3.9, 2.4, 1.9], [0.95, 0.9, 0.8])
METAL_CHECKER = conductor([0.2, 0.9, 1.4], [3.9, 2.4, 1.9], gt.CHECKER)

CATALOGUE = {
    "dielectric_glass": GLASS,
    "dielectric_bubble": BUBBLE,
    "dielectric_matched": MATCHED,
    "dielectric_coloured": GLASS_COLOURED,
    "dielectric_checker": GLASS_CHECKER,
    "conductor_mirror": MIRROR,
    "conductor_rgb": METAL,
    "conductor_checker": METAL_CHECKER,
    "twosided_c": R.twosided(METAL),
    "twosided_c_d": R.twosided(METAL, R.D0),
}
GREY = {
    "grey_dielectric": dielectric(1.5, 1.0, 0.8, 0.9),
    "grey_conductor": conductor(0.9, 2.4, 0.9),
    "mono_conductor": conductor([0.2, 0.9, 1.4], [3.9, 2.4, 1.9], 0.9),   # rgb eta / k: their luminance under gpu_mono
}
ALL_TREES = dict(CATALOGUE, **GREY)
SHEETS = R.SHEETS
# R's backdrop: the sheet met from behind, a black rectangle before its front -- where a refracted ray goes
BACKDROP_CASES = [("dielectric_glass", "rectangle", "backdrop")]
CASES = [(name, surface, placement) for name in CATALOGUE for surface, placement in SHEETS] + BACKDROP_CASES
VOLPATH_CASES = [("dielectric_coloured", "rectangle", None), ("dielectric_bubble", "quad_uv", "mirrored"), ("conductor_rgb", "disk", None),
                 ("twosided_c_d", "rectangle", "placed"), ("dielectric_checker", "quad_uv", None)]
MONO_CASES = [("grey_dielectric", "rectangle", None), ("grey_conductor", "quad_uv", "placed"), ("mono_conductor", "disk", None)]

_CASES = {}


def case_of(name, surface, placement):
    """built once, shared by every test, left unchanged"""
    key = (name, surface, placement)
    if key not in _CASES:
        _CASES[key] = build_case(ALL_TREES[name], surface, placement)
    return _CASES[key]


def expected_branches(name, placement):
    """the branches a case must populate on kept lanes: tag -> values.  dielectric_branch: 0 reflection, 1 transmission in (from
    above), 2 transmission out (from below), 3 total internal reflection -- on the denser side, which the bubble has above"""
    tree = ALL_TREES[name]
    out = {}

    def walk(t):
        if t["kind"] == "dielectric":
            eta = float(np.float32(t["int_ior"]) / np.float32(t["ext_ior"]))
            out["dielectric_branch"] = {1, 2} if eta == 1.0 else {0, 1, 2, 3}
            if placement == "backdrop":
                out["dielectric_branch"] = {0, 2}                          # R's rays: from behind and steep
        if t["kind"] == "conductor":
            out["conductor_side"] = {0, 1}
        if t["kind"] == "twosided":
            out["twosided_side"] = {0, 1}
            for c in t["children"]:
                walk(c)
            out.pop("conductor_side", None)                                # under an adapter a conductor is met from its front alone
    walk(tree)
    return out
