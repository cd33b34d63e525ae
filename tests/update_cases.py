"""Scene pairs (A, B, assignments) shared by the tests of traverse() / mts_scene_update (tests/test_traverse.py on the CPU,
tests/test_gpu_scene_update.py on the device)."""
import copy
import importlib

import numpy as np

scenes = importlib.import_module("eradiate-kernel_amd.scenes")


def spectral_edit():
    """C5S with explicit spectra on the ground and the sun; B: both gridvolume_spectral grids, a uniform value, a regular spectrum's values
    and range on the BSDF, the emitter's regular values."""
    a = scenes.c5_atmosphere_spectral(16, 16, 8, layers=8, nodes=5)
    a["sun"]["irradiance"] = {"type": "regular", "lambda_min": 300.0, "lambda_max": 900.0, "values": [1.0, 2.0, 1.5, 1.0]}
    b = copy.deepcopy(a)
    med = b["atmosphere"]["interior"]
    sig = (med["sigma_t"]["data"] * np.float32(1.3)).astype(np.float32)
    alb = (med["albedo"]["data"] * np.float32(0.9)).astype(np.float32)
    med["sigma_t"]["data"], med["albedo"]["data"] = sig, alb
    b["ground"]["bsdf"]["rho_0"] = {"type": "regular", "lambda_min": 320.0, "lambda_max": 880.0, "values": [0.3, 0.2, 0.1]}
    b["ground"]["bsdf"]["k"] = 0.75
    b["sun"]["irradiance"]["values"] = [0.5, 1.0, 2.5, 2.0]
    pre = "atmosphere.interior_medium."
    return a, b, {pre + "sigma_t.data": sig, pre + "albedo.data": alb, "ground.bsdf.rho_0.values": [0.3, 0.2, 0.1], "ground.bsdf.rho_0.range": (320.0, 880.0),
                  "ground.bsdf.k.value": 0.75, "sun.irradiance.values": [0.5, 1.0, 2.5, 2.0]}
