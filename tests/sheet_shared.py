"""Constants that several single-sheet tests share: the blend tests' weights and the instance tests' placement.  TEST
INFRASTRUCTURE: definitions only, so that a helper needing them does not import a whole test module for them."""
import importlib

import numpy as np

import tests.test_gpu_textures as gt

T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

# ---- the weights of a `blendbsdf` (tests/test_gpu_blendbsdf.py)
CLAMPED = np.array([[-0.5, 1.5, 0.25, 1.5], [1.5, 0.75, -0.5, -0.5], [-0.5, 1.5, 1.5, 0.5], [0.25, -0.5, 1.5, -0.5]], np.float32)
WEIGHTS = {
    "constant": 0.3,
    "bilinear_1ch": dict(gt.TEXTURES["b44_bilinear_repeat"]),
    "bilinear_3ch": dict(gt.TEXTURES["b44rgb_bilinear_clamp"]),
    "checkerboard": {"type": "checkerboard", "color0": 0.8, "color1": 0.1, "to_uv": T.scale([4.0, 4.0, 1.0])},
    "nearest_clamped": {"type": "bitmap", "data": CLAMPED, "filter_type": "nearest", "wrap_mode": "mirror", "to_uv": gt.UV23},
}

# ---- the placement of an instance (tests/test_gpu_instance.py): a rotation about a skew axis x an uneven scale x a translation
AXIS, ANGLE, SCALE, SHIFT = np.array([0.3, -0.5, 0.8]), 37.0, np.array([1.0, 0.6, 0.8]), np.array([0.2, -0.15, 0.1])
PLACE = T.rotate(AXIS.tolist(), ANGLE) @ T.scale(SCALE.tolist()) @ T.translate(SHIFT.tolist())


def place_matrix():
    """the same transform from the definitions, float64: Rodrigues' rotation matrix times diag(scale) times the translation"""
    k = AXIS / np.linalg.norm(AXIS)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(ANGLE)
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R @ np.diag(SCALE)
    M[:3, 3] = M[:3, :3] @ SHIFT
    return M
