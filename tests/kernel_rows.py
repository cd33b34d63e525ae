"""The names of a render kernel (csrc/kernel_names.h: kv, KernelUnit; csrc/render_plan.h: Tri) mirrored in Python, and for every row
of the kernel table (csrc/render_plan.cpp: KERNEL_ROWS) a small scene and the switches under which mts_render chooses that row.

tests/test_render_plan.py holds the mapping against the table (a kernel without a scene fails there, without a GPU), tests/test_abi.py
asks the library for its choice on each scene, tests/test_gpu_parity.py renders them."""
import importlib

scenes = importlib.import_module("eradiate-kernel_amd.scenes")

NESTED, FLAT = 0, 1
GENERAL, A, B, S, P, PS, H, C = range(8)
NO, YES, EITHER = 0, 1, 2
PATH, VOLPATH, VOLPATHMIS = 0, 1, 2
SWITCHES = ("MTSAMD_KERNEL", "MTSAMD_LEAN", "MTSAMD_BVH_THRESHOLD", "MTSAMD_WAVEFRONT_SPLIT")


def ring(paths):
    return 10000 + paths


def is_ring(variant):
    return variant >= 10000


def stat(variant, unit=GENERAL):
    """mts_stats.kernel_variant"""
    return variant + 100000 * unit


def stat_variant(kernel_variant):
    return kernel_variant % 100000


def stat_unit(kernel_variant):
    return kernel_variant // 100000


def spectral_cornell(width, height, spp):
    d = scenes.c1_cornell(width, height, spp)
    for k, v in d.items():
        if isinstance(v, dict) and "bsdf" in v:
            rgb = v["bsdf"]["reflectance"]["value"]
            v["bsdf"]["reflectance"] = {"type": "regular", "lambda_min": 400., "lambda_max": 700., "values": [rgb[2], rgb[1], rgb[0]]}
    d["light"]["emitter"]["radiance"] = {"type": "d65", "scale": 3.0}
    return d


_SMALL = dict(block_size=16)


# A film of 32 x 32 pixels, two samples per pixel: one spiral block and one workgroup of the 1024-path machine, two of the 512-path machine.
# The 256-path rows render it as four blocks of 16 x 16 pixels (_SMALL), one workgroup each, the spectral build's (_c5s) included.
def _c3(**integrator):
    d = scenes.c3_heterogeneous(32, 32, 2, res=8)
    d["integrator"] = dict(d["integrator"], **integrator)
    return d


def _c3_wavefront():
    d = _c3()
    d["sensor"]["sampler"]["wavefront"] = True
    return d


def _c2(**integrator):
    d = scenes.c2_homogeneous_slab(32, 32, 2)
    d["integrator"] = dict(d["integrator"], **integrator)
    return d


def _c5s(**integrator):
    d = scenes.c5_atmosphere_spectral(32, 32, 2, layers=8, nodes=5)
    d["integrator"] = dict(d["integrator"], **_SMALL, **integrator)
    return d


def _box():
    return scenes.c1_cornell(32, 32, 2)


def _box_spectral():
    return spectral_cornell(32, 32, 2)


_MIS, _MIS_PLAIN = dict(type="volpathmis", use_spectral_mis=True), dict(type="volpathmis", use_spectral_mis=False)


SCENES = {"c3": _c3, "c3_wavefront": _c3_wavefront, "c3_small_blocks": lambda: _c3(**_SMALL),
          "c3_mis": lambda: _c3(**_MIS), "c3_mis_plain": lambda: _c3(**_MIS_PLAIN),
          "c3_mis_small_blocks": lambda: _c3(**_MIS, **_SMALL), "c3_mis_plain_small_blocks": lambda: _c3(**_MIS_PLAIN, **_SMALL),
          "c2": _c2, "c2_mis": lambda: _c2(**_MIS), "c5s": _c5s, "c5s_mis": lambda: _c5s(**_MIS), "c5s_mis_plain": lambda: _c5s(**_MIS_PLAIN),
          "box": _box, "box_spectral": _box_spectral}


def _row(name, exact=True, **env):
    """name: the scene (one oracle film serves every row that renders it).  exact: the film equals the oracle's bit for bit, as the
    existing test of that scene and kernel holds it; otherwise that test's comparison (test_gpu_parity.assert_parity).  env: the
    switches that select the row (without their MTSAMD_ prefix)."""
    return {"name": name, "scene": SCENES[name], "exact": exact, "env": {"MTSAMD_" + k: v for k, v in env.items()}}


# (unit, variant, integrator, spectral MIS, wavefront streams, spectral build) -> scene, comparison, switches
ROWS = {
    (GENERAL, ring(1024), VOLPATH, EITHER, NO, False): _row("c3", LEAN="0"),
    (GENERAL, ring(1024), VOLPATH, EITHER, YES, False): _row("c3_wavefront", WAVEFRONT_SPLIT="1"),
    (GENERAL, ring(256), VOLPATH, EITHER, NO, False): _row("c3_small_blocks", exact=False),
    (GENERAL, ring(512), VOLPATHMIS, YES, NO, False): _row("c3_mis", LEAN="0"),
    (GENERAL, ring(512), VOLPATHMIS, NO, NO, False): _row("c3_mis_plain"),
    (GENERAL, ring(256), VOLPATHMIS, YES, NO, False): _row("c3_mis_small_blocks", exact=False),
    (GENERAL, ring(256), VOLPATHMIS, NO, NO, False): _row("c3_mis_plain_small_blocks", exact=False),
    (GENERAL, FLAT, VOLPATH, EITHER, EITHER, False): _row("c3", KERNEL="flat"),
    (GENERAL, FLAT, PATH, EITHER, EITHER, False): _row("box", LEAN="0"),
    (GENERAL, FLAT, VOLPATHMIS, YES, EITHER, False): _row("c3_mis", KERNEL="flat"),
    (GENERAL, FLAT, VOLPATHMIS, NO, EITHER, False): _row("c3_mis_plain", KERNEL="flat"),
    (GENERAL, NESTED, PATH, EITHER, EITHER, False): _row("box", KERNEL="nested"),
    (GENERAL, NESTED, VOLPATH, EITHER, EITHER, False): _row("c3", KERNEL="nested"),
    (GENERAL, NESTED, VOLPATHMIS, YES, EITHER, False): _row("c3_mis", KERNEL="nested"),
    (GENERAL, NESTED, VOLPATHMIS, NO, EITHER, False): _row("c3_mis_plain", KERNEL="nested"),
    (GENERAL, ring(256), VOLPATH, EITHER, NO, True): _row("c5s", LEAN="0"),
    (GENERAL, ring(256), VOLPATHMIS, YES, NO, True): _row("c5s_mis", LEAN="0"),
    (GENERAL, ring(256), VOLPATHMIS, NO, NO, True): _row("c5s_mis_plain", exact=False),
    (GENERAL, FLAT, PATH, EITHER, EITHER, True): _row("box_spectral", exact=False, LEAN="0"),
    (GENERAL, NESTED, PATH, EITHER, EITHER, True): _row("box_spectral", exact=False, KERNEL="nested"),
    (GENERAL, NESTED, VOLPATH, EITHER, EITHER, True): _row("c5s", exact=False, KERNEL="nested"),
    (GENERAL, NESTED, VOLPATHMIS, YES, EITHER, True): _row("c5s_mis", exact=False, KERNEL="nested"),
    (GENERAL, NESTED, VOLPATHMIS, NO, EITHER, True): _row("c5s_mis_plain", exact=False, KERNEL="nested"),
    (A, ring(1024), VOLPATH, EITHER, NO, False): _row("c3"),
    (A, ring(512), VOLPATHMIS, YES, NO, False): _row("c3_mis"),
    (B, ring(1024), VOLPATH, EITHER, NO, False): _row("c3", LEAN="2"),
    (B, ring(512), VOLPATHMIS, YES, NO, False): _row("c3_mis", LEAN="2"),
    (C, ring(1024), VOLPATH, EITHER, NO, False): _row("c3", BVH_THRESHOLD="0"),
    (C, ring(512), VOLPATHMIS, YES, NO, False): _row("c3_mis", BVH_THRESHOLD="0"),
    (H, ring(1024), VOLPATH, EITHER, NO, False): _row("c2"),
    (H, ring(512), VOLPATHMIS, YES, NO, False): _row("c2_mis"),
    (S, ring(256), VOLPATH, EITHER, NO, True): _row("c5s"),
    (S, ring(256), VOLPATHMIS, YES, NO, True): _row("c5s_mis"),
    (P, FLAT, PATH, EITHER, EITHER, False): _row("box"),
    (PS, FLAT, PATH, EITHER, EITHER, True): _row("box_spectral", exact=False),
}
