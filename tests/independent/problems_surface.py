"""The surface-transport problems of tests/test_independent_surface_pin.py, each stated twice: as a scene dictionary for the
oracle / the HIP path, and in the terms of tests/independent/surface.py.

As in problems.py only DATA is shared (numbers: sizes, colours, angles).  The geometry of the second statement is written out
again in world space -- centres, edge vectors, normals, worked out here by hand or with the Rodrigues formula below -- and never
passes through the loader's transforms, so a mistake in the handling of a `to_world` shows up as a disagreement.

Every factory returns (scene dictionary, surface.Scene, surface.Pinhole, max_depth, vertices): `vertices` is the fixed vertex
count at which the walks of an unlimited-depth problem are cut, with `remainder_bound` giving what that leaves out."""
import importlib
import math

import numpy as np

from . import surface as S

scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f


def rodrigues(axis, angle_deg, v):
    """v turned about `axis` by `angle_deg` (right-handed): v cos + (k x v) sin + k (k.v) (1 - cos)."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    v = np.asarray(v, np.float64)
    a = math.radians(angle_deg)
    return v * math.cos(a) + np.cross(k, v) * math.sin(a) + k * (k @ v) * (1.0 - math.cos(a))


def _rgb(v):
    return {"type": "rgb", "value": [float(x) for x in v]}


def _diffuse(v):
    return {"type": "diffuse", "reflectance": _rgb(v)}


def _sensor(origin, target, up, fov, width, height):
    return {"type": "perspective", "to_world": T.look_at(origin, target, up), "fov": float(fov), "near_clip": 0.1, "far_clip": 1000.0,
            "film": {"type": "hdrfilm", "width": width, "height": height, "rfilter": {"type": "box"}},
            "sampler": {"type": "independent", "sample_count": 1, "seed": 0}}


# ---- 1, 2: the cornell box of the benchmark ---------------------------------------------------------------------------------
def box(width=16, height=16, max_depth=-1):
    """scenes.c1_cornell exactly as the benchmark has it.  Restated: five walls of a 10 x 10 x 7 room open towards -y, normals
    inwards, and a 3 x 3 lamp 0.01 below the ceiling that faces down.  The lamp has no BSDF of its own: an emitting shape then
    gets a diffuse one with reflectance 0 (src/librender/shape.cpp:75-81), so it is black apart from its emission."""
    d = scenes.c1_cornell(width, height, 1, max_depth=max_depth)
    assert d["integrator"]["rr_depth"] == 5
    white, red, green = S.Material("diffuse", [0.8, 0.8, 0.8]), S.Material("diffuse", [0.8, 0.1, 0.1]), S.Material("diffuse", [0.1, 0.8, 0.1])
    lamp = S.Material("diffuse", 0.0, Le=[3.0, 3.0, 3.0])
    prims = [
        S.Rectangle([0, 0, 0], [5, 0, 0], [0, 5, 0], white),                          # floor, normal +z
        S.Rectangle([0, 0, 7], [5, 0, 0], [0, -5, 0], white),                         # ceiling, turned over: normal -z
        S.Rectangle([0, 5, 3.5], [5, 0, 0], [0, 0, 3.5], white),                      # back wall, normal -y
        S.Rectangle([-5, 0, 3.5], [0, 0, -3.5], [0, 5, 0], red),                      # left wall, normal +x
        S.Rectangle([5, 0, 3.5], [0, 0, 3.5], [0, 5, 0], green),                      # right wall, normal -x
        S.Rectangle([0, 0, 6.99], [1.5, 0, 0], [0, -1.5, 0], lamp),                   # lamp, normal -z
    ]
    for p, n in zip(prims, ([0, 0, 1], [0, 0, -1], [0, -1, 0], [1, 0, 0], [-1, 0, 0], [0, 0, -1])):
        assert np.allclose(p.n, n)
    cam = S.Pinhole(width, height, 40.0, [0, -14, 3.5], [0, 0, 3.5], [0, 0, 1])
    return d, S.Scene(prims), cam, max_depth, 80


def box_d3(width=16, height=16):
    return box(width, height, max_depth=3)


# ---- 3: an open scene under a sky ------------------------------------------------------------------------------------------
ORBS = {"sky": 0.5, "rpv": (0.2, 0.7, -0.1), "ground_radius": 14.0,                    # rpv inside the fuzzer's ranges (tests/test_gpu_fuzz.py)
        "lamp_centre": [-1.5, 0.5, 2.6], "lamp_radius": 0.6, "lamp_radiance": [6.0, 4.0, 2.0], "lamp_reflectance": 0.3,
        "ball_centre": [1.3, -0.6, 0.95], "ball_radius": 0.8, "ball_reflectance": [0.3, 0.5, 0.7],
        "cube_centre": [-0.9, 1.9, 1.15], "cube_axis": [0.3, 0.2, 1.0], "cube_angle": 35.0, "cube_scale": [0.9, 0.5, 0.7],
        "cube_reflectance": [0.7, 0.4, 0.2], "origin": [0.0, -6.0, 8.0], "target": [0.0, 0.0, 0.5], "fov": 40.0}


def orbs(width=16, height=16, lamp_radius_factor=1.0, grey=False, rpv_rule="reference"):
    """A grey constant sky and a sphere lamp (two emitters) over an rpv ground disk, with a diffuse sphere and a turned,
    non-uniformly scaled diffuse cube as occluders and receivers.  Every sensor ray meets the ground or an object (asserted by the
    tests): a pixel of pure sky would have no variance on either side and nothing to test.  `grey`: the twin with grey colours
    (the channel means of the chromatic ones) for the spectral variant."""
    o = dict(ORBS)
    if grey:
        for key in ("lamp_radiance", "ball_reflectance", "cube_reflectance"):
            o[key] = [float(np.mean(o[key]))] * 3
    radius = o["lamp_radius"] * lamp_radius_factor
    rho0, k, g = o["rpv"]
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": -1, "rr_depth": 5, "block_size": 32},
         "sensor": _sensor(o["origin"], o["target"], [0, 0, 1], o["fov"], width, height),
         "ground": {"type": "disk", "to_world": T.scale(o["ground_radius"]), "bsdf": {"type": "rpv", "rho_0": rho0, "k": k, "g": g}},
         "lamp": {"type": "sphere", "center": o["lamp_centre"], "radius": radius, "bsdf": _diffuse([o["lamp_reflectance"]] * 3),
                  "emitter": {"type": "area", "radiance": _rgb(o["lamp_radiance"])}},
         "ball": {"type": "sphere", "center": o["ball_centre"], "radius": o["ball_radius"], "bsdf": _diffuse(o["ball_reflectance"])},
         "cube": {"type": "cube", "to_world": T.translate(o["cube_centre"]) @ T.rotate(o["cube_axis"], o["cube_angle"]) @ T.scale(o["cube_scale"]),
                  "bsdf": _diffuse(o["cube_reflectance"])},
         "sky": {"type": "constant", "radiance": _rgb([o["sky"]] * 3)}}
    axes = [rodrigues(o["cube_axis"], o["cube_angle"], np.eye(3)[i] * o["cube_scale"][i]) for i in range(3)]
    prims = [
        S.Disk([0, 0, 0], [0, 0, 1], o["ground_radius"], S.Material("rpv", rpv=(rho0, k, g, rho0))),      # rpv.cpp:76-80: rho_c defaults to rho_0
        S.Sphere(o["lamp_centre"], radius, S.Material("diffuse", o["lamp_reflectance"], Le=o["lamp_radiance"])),
        S.Sphere(o["ball_centre"], o["ball_radius"], S.Material("diffuse", o["ball_reflectance"])),
        S.Box(o["cube_centre"], axes[0], axes[1], axes[2], S.Material("diffuse", o["cube_reflectance"])),
    ]
    cam = S.Pinhole(width, height, o["fov"], o["origin"], o["target"], [0, 0, 1])
    return d, S.Scene(prims, env=[o["sky"]] * 3, n_emitters=2, rpv_rule=rpv_rule), cam, -1, 56


ORBS_MAX_ALBEDO = 0.7      # the largest diffuse reflectance of the scene; the rpv ground's albedo / pi stays below it (test_rpv_albedo_bound_of_the_orbs_problem)


def orbs_grey(width=16, height=16):
    return orbs(width, height, grey=True)


def orbs_balance(width=16, height=16):
    """`orbs` as `volpathmis` renders it: the reference's rpv sampling rule under the balance heuristic (surface.py's docstring)."""
    return orbs(width, height, rpv_rule="reference_balance")


# ---- 4: leaves under two lamps ---------------------------------------------------------------------------------------------
CANOPY = {"leaves": 12, "seed": 20261019, "rho": [0.5, 0.55, 0.45], "tau": [0.4, 0.35, 0.3], "ground": [0.3, 0.25, 0.2], "ground_half": 14.0,
          "quad": {"centre": [-1.4, 3.0, 4.5], "half": 1.6, "radiance": [5.0, 4.0, 3.0]},
          "disk": {"centre": [1.6, 2.6, 4.0], "radius": 1.5, "radiance": [2.0, 3.0, 5.0]}, "lamp_reflectance": 0.2,
          "origin": [0.0, -6.5, 7.0], "target": [0.0, 0.0, 0.8], "fov": 36.0}


def canopy(width=16, height=16, swap=False):
    """A dozen seeded, randomly turned bilambertian rectangles over a diffuse ground, lit by a two-triangle mesh lamp and a disk lamp
    overhead that both face down; no sky.  `swap`: rho and tau of the leaves exchanged (the mutation the pin must reject)."""
    c = CANOPY
    rho, tau = (c["tau"], c["rho"]) if swap else (c["rho"], c["tau"])
    rng = np.random.default_rng(c["seed"])
    q, k = c["quad"], c["disk"]
    qc, qh = np.asarray(q["centre"], np.float64), q["half"]
    # corners in an order whose (p1 - p0) x (p2 - p0) points down
    corners = [qc + [-qh, -qh, 0], qc + [-qh, qh, 0], qc + [qh, qh, 0], qc + [qh, -qh, 0]]
    lampbsdf = _diffuse([c["lamp_reflectance"]] * 3)
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": -1, "rr_depth": 5, "block_size": 32},
         "sensor": _sensor(c["origin"], c["target"], [0, 0, 1], c["fov"], width, height),
         "ground": {"type": "rectangle", "to_world": T.scale(c["ground_half"]), "bsdf": _diffuse(c["ground"])},
         "quad": {"type": "mesh", "vertex_positions": np.array(corners, np.float32), "faces": np.array([[0, 1, 2], [0, 2, 3]], np.uint32),
                  "bsdf": lampbsdf, "emitter": {"type": "area", "radiance": _rgb(q["radiance"])}},
         "disk": {"type": "disk", "to_world": T.translate(k["centre"]) @ T.rotate([1, 0, 0], 180) @ T.scale(k["radius"]),
                  "bsdf": lampbsdf, "emitter": {"type": "area", "radiance": _rgb(k["radiance"])}}}
    lamp_q = S.Material("diffuse", c["lamp_reflectance"], Le=q["radiance"])
    lamp_d = S.Material("diffuse", c["lamp_reflectance"], Le=k["radiance"])
    quad_area = 4.0 * qh * qh
    prims = [S.Rectangle([0, 0, 0], [c["ground_half"], 0, 0], [0, c["ground_half"], 0], S.Material("diffuse", c["ground"])),
             S.Triangle(corners[0], corners[1], corners[2], lamp_q, quad_area), S.Triangle(corners[0], corners[2], corners[3], lamp_q, quad_area),
             S.Disk(k["centre"], [0, 0, -1], k["radius"], lamp_d)]
    assert np.allclose(prims[1].n, [0, 0, -1]) and np.allclose(prims[2].n, [0, 0, -1])
    leaf = S.Material("bilambertian", rho, tau)
    for i in range(c["leaves"]):
        centre = rng.uniform([-2.2, -2.2, 0.9], [2.2, 2.2, 2.4])
        axis = rng.normal(size=3)
        angle = float(rng.uniform(0.0, 180.0))
        half = rng.uniform(0.5, 0.9, 2)
        centre, axis, half = [float(x) for x in centre], [float(x) for x in axis], [float(x) for x in half]
        d["leaf%02d" % i] = {"type": "rectangle", "to_world": T.translate(centre) @ T.rotate(axis, angle) @ T.scale([half[0], half[1], 1.0]),
                             "bsdf": {"type": "bilambertian", "reflectance": _rgb(rho), "transmittance": _rgb(tau)}}
        prims.append(S.Rectangle(centre, rodrigues(axis, angle, [half[0], 0, 0]), rodrigues(axis, angle, [0, half[1], 0]), leaf))
    cam = S.Pinhole(width, height, c["fov"], c["origin"], c["target"], [0, 0, 1])
    return d, S.Scene(prims), cam, -1, 180


# ---- 5: direct light of a point emitter ------------------------------------------------------------------------------------
POINT = {"position": [1.0, -1.5, 5.0], "intensity": [30.0, 25.0, 20.0], "ground": [0.6, 0.5, 0.4], "ground_half": 14.0,
         "ball_centre": [-0.4, 0.3, 1.4], "ball_radius": 0.9, "ball_reflectance": [0.4, 0.6, 0.8],
         "origin": [0.0, -6.0, 8.0], "target": [0.0, 0.0, 0.5], "fov": 40.0}


def point_direct(width=16, height=16):
    """A point emitter over a diffuse ground with a diffuse sphere that casts a shadow, max_depth = 2 (direct light only)."""
    c = POINT
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": 2, "rr_depth": 5, "block_size": 32},
         "sensor": _sensor(c["origin"], c["target"], [0, 0, 1], c["fov"], width, height),
         "ground": {"type": "rectangle", "to_world": T.scale(c["ground_half"]), "bsdf": _diffuse(c["ground"])},
         "ball": {"type": "sphere", "center": c["ball_centre"], "radius": c["ball_radius"], "bsdf": _diffuse(c["ball_reflectance"])},
         "bulb": {"type": "point", "position": c["position"], "intensity": _rgb(c["intensity"])}}
    prims = [S.Rectangle([0, 0, 0], [c["ground_half"], 0, 0], [0, c["ground_half"], 0], S.Material("diffuse", c["ground"])),
             S.Sphere(c["ball_centre"], c["ball_radius"], S.Material("diffuse", c["ball_reflectance"]))]
    cam = S.Pinhole(width, height, c["fov"], c["origin"], c["target"], [0, 0, 1])
    return d, S.Scene(prims), cam, 2, 2
