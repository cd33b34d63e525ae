"""The specular surface-transport problem of tests/test_specular_pin.py and tests/test_gpu_specular_pin.py, stated twice as
problems_surface.py states its own: as a scene dictionary for the HIP path -- the lit box of problems_surface.box with a glass
sphere, a tilted coloured conductor plate and an upright `twosided(conductor)` panel -- and in the terms of
tests/independent/specular.py, which knows no plugin, no relative index, no adapter and no local frame.

The second statement:

  sphere   a dielectric boundary by its two absolute indices, 1.5 inside and 1 outside (the dictionary gives int_ior / ext_ior, the
           loader makes eta of them, the device the two reciprocal ratios and their squares);
  plate    a one-sided conductor rectangle whose corners come from the Rodrigues formula of problems_surface, not from the loader's
           transforms: lying in z = 0 it is turned about x by 30 degrees (its normal leans towards the camera) and about z by -20.  The
           angle keeps the lamp's mirror image off the film: a pixel that lies wholly inside it has the same value in every walk
           but for the Fresnel factor's drift across it, a variance of 1e-15 against which no fp32 film passes a Z-test;
  panel    `twosided(conductor)` is two one-sided conductor rectangles back to back, 1e-9 apart, as problems_twosided.py does it.

`mutation`: the same problem with one thing wrong in the DICTIONARY alone -- what the pin must reject: "eta_inverted" (int_ior and
ext_ior exchanged: a bubble instead of a ball), "k_zero" (the plate's k = 0: a weak dielectric-like reflector instead of a metal)."""
import numpy as np

from . import problems_surface
from . import specular as X
from . import surface as S
from .problems_surface import rodrigues

T = problems_surface.T

BALL = {"centre": [-2.2, -0.8, 1.7], "radius": 1.5, "int_ior": 1.5, "ext_ior": 1.0}
PLATE = {"centre": [2.5, 0.3, 2.0], "half": [1.7, 1.3], "turns": [([1, 0, 0], 30.0), ([0, 0, 1], -20.0)],
         "eta": [0.2, 0.9, 1.4], "k": [3.9, 2.4, 1.9], "colour": [0.9, 0.7, 0.5]}
PANEL = {"centre": [0.4, 2.6, 3.3], "half": [1.6, 1.2], "turns": [([1, 0, 0], 90.0), ([0, 0, 1], 25.0)],
         "eta": [0.6, 0.6, 0.6], "k": [3.0, 3.0, 3.0], "colour": [0.6, 0.8, 0.9]}
GAP = 1e-9
MAX_INDEX_RATIO = 1.5


def _turned(turns, v):
    for axis, angle in turns:
        v = rodrigues(axis, angle, v)
    return np.asarray(v, np.float64)


def _to_world(rect):
    xf = T.scale([rect["half"][0], rect["half"][1], 1.0])
    for axis, angle in rect["turns"]:
        xf = T.rotate(list(axis), angle) @ xf
    return T.translate(rect["centre"]) @ xf


def _conductor(rect, k=None):
    return {"type": "conductor", "eta": problems_surface._rgb(rect["eta"]), "k": problems_surface._rgb(rect["k"] if k is None else k),
            "specular_reflectance": problems_surface._rgb(rect["colour"])}


def box_specular(width=16, height=16, mutation=None):
    assert mutation in (None, "eta_inverted", "k_zero")
    d, scene, cam, max_depth, vertices = problems_surface.box(width, height)
    inner, outer = (BALL["ext_ior"], BALL["int_ior"]) if mutation == "eta_inverted" else (BALL["int_ior"], BALL["ext_ior"])
    d["ball"] = {"type": "sphere", "center": BALL["centre"], "radius": BALL["radius"],
                 "bsdf": {"type": "dielectric", "int_ior": inner, "ext_ior": outer}}
    d["plate"] = {"type": "rectangle", "to_world": _to_world(PLATE), "bsdf": _conductor(PLATE, [0.0, 0.0, 0.0] if mutation == "k_zero" else None)}
    d["panel"] = {"type": "rectangle", "to_world": _to_world(PANEL), "bsdf": {"type": "twosided", "metal": _conductor(PANEL)}}
    prims = list(scene.prims)
    prims.append(S.Sphere(BALL["centre"], BALL["radius"], X.Material("dielectric", rho=1.0, tau=1.0, n_int=BALL["int_ior"], n_ext=BALL["ext_ior"])))
    for rect, both in ((PLATE, False), (PANEL, True)):
        eu, ev = _turned(rect["turns"], [rect["half"][0], 0, 0]), _turned(rect["turns"], [0, rect["half"][1], 0])
        n = _turned(rect["turns"], [0, 0, 1])
        mat = X.Material("conductor", rho=rect["colour"], eta=rect["eta"], k=rect["k"])
        c = np.asarray(rect["centre"], np.float64)
        if not both:
            prims.append(S.Rectangle(c, eu, ev, mat))
        else:
            prims += [S.Rectangle(c + 0.5 * GAP * n, eu, ev, mat), S.Rectangle(c - 0.5 * GAP * n, eu, -ev, mat)]
        assert np.allclose(prims[-1].n, -n if both else n, atol=1e-12)
    return d, S.Scene(prims), cam, max_depth, vertices


def sees_the_front(cam_origin=(0.0, -14.0, 3.5)):
    """the camera stands before the plate's front, and the ball is before it too: no sensor ray and no ray off the ball meets its back
    by construction of the problem -- (the value does not depend on it: a conductor is black from behind in both statements)"""
    n = _turned(PLATE["turns"], [0, 0, 1])
    return float((np.asarray(cam_origin) - np.asarray(PLATE["centre"])) @ n) > 0.0
