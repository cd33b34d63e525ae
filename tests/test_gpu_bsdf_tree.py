"""BSDF trees on the device, per sample (run with -m gpu on an MI355X): `blendbsdf`, `twosided` and textured parameters against the
float64 restatement of tests/bsdf_tree_ref.py, which tests/test_bsdf_tree_ref.py validates against the oracle on the CPU.

  a. the float64 pin -- SamplingIntegrator::sample on 4 099 caller-supplied rays per tree and sheet, lane by lane: `path` for every
     case, `volpath` rgb and `volpath` in gpu_mono for a subset.  On every kept lane `valid` and the sum's pattern of zeros agree exactly and
     the value agrees within DEVICE_FACTOR * E (E: the fp32 scale measured on the CPU; nothing measured here enters the bound); the
     bilinear cases within the texture tests' ATOL.  The device returns the sum of the emitter term and the BSDF term, so "which term is zero"
     is read through it: on a third to a half of the kept lanes one of the two is zero by the restatement, and a device term that is
     not would move the sum by far more than the bound.
  b. the rows -- the same dictionaries rendered through an mradiancemeter of 300 of the rays: the flat TEX / INST loop of `path`
     equals MTSAMD_KERNEL=nested bit for bit, and with a medium of no effect the ring TEX / INST row of `volpath` equals nested and
     flat.  mts_sample runs the nested formulation, so this is how the float64 pin reaches the flat loop's and the ring machine's own
     calls of blend_* and twosided_side.

Every figure printed here is measured on the device."""
import numpy as np
import pytest

import tests.bsdf_tree_ref as R
import tests.test_gpu_textures as gt
from tests.test_gpu_textures import bits, render

pytestmark = pytest.mark.gpu

CASES = [(name, surface, placement) for name in list(R.CATALOGUE) + list(R.BILINEAR) for surface, placement in R.SHEETS] + R.BACKDROP_CASES
# `volpath` rgb: one case per wrapper kind, an adapter over a blend, the bilinear lookup, and instanced ones
VOLPATH_CASES = [("blend_d_bilamb", "rectangle", None), ("blend_bilambtex_rpv_wchecker", "disk", None), ("twosided_rpv_dchecker", "quad_uv", None),
                 ("twosided_blend_rpvtex", "rectangle", "placed"), ("blend_rpvtex_d_wtex", "quad_uv", "mirrored"), ("blend_dbilinear_rpv", "rectangle", None)]
MONO_CASES = [("grey_blend", "rectangle", None), ("grey_twosided", "quad_uv", "placed")]
TEXTURED = {None: 1, "backdrop": 1, "placed": 2, "mirrored": 2}             # mts_stats.textured: the TEX and the INST instantiations

_CASES = {}


def case_of(name, surface, placement):
    """built once, shared by the pin and the rows, left unchanged"""
    key = (name, surface, placement)
    if key not in _CASES:
        _CASES[key] = R.build_case(R.ALL_TREES[name], surface, placement)
    return _CASES[key]


def assert_pinned(pkg, name, surface, placement, integrator, mono=False):
    case = case_of(name, surface, placement)
    ref = R.restate(case, integrator=integrator, mono=mono)                 # decides the lanes before any device value is looked at
    kept = ref.kept
    assert 1.0 - kept.mean() <= R.MAX_DROP
    scene = pkg.load_dict(dict(case.scene, integrator=dict(case.scene["integrator"], type=integrator)))
    assert int(scene._desc.sensor.sampler_seed) == R.base_seed()
    rgb, valid = scene.integrator().sample(scene, case.origins, case.directions, seed_offset=R.SEED_OFFSET)
    err = R.scaled_error(rgb, ref.value)
    absolute = np.abs(rgb - ref.value)
    print("%s %s %s %s%s: kept %d of %d, max scaled error %.3g (bound %.3g), max |difference| %.3g%s"
          % (name, surface, placement, integrator, " mono" if mono else "", kept.sum(), len(kept), err[kept].max(), R.device_bound(placement), absolute[kept].max(),
             " (bilinear: this one is bounded, by ATOL = %.3g)" % gt.ATOL if name in R.BILINEAR else ""))
    assert valid.all()
    assert np.array_equal(rgb[kept] == 0, ref.value[kept] == 0)
    assert not R.exceeds_bound(name, placement, rgb, ref.value)[kept].any()


# ================================================================ a. the float64 pin
@pytest.mark.parametrize("name,surface,placement", CASES)
def test_path_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    assert_pinned(gpu_rgb, name, surface, placement, "path")


@pytest.mark.parametrize("name,surface,placement", VOLPATH_CASES)
def test_volpath_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    assert_pinned(gpu_rgb, name, surface, placement, "volpath")


@pytest.mark.parametrize("name,surface,placement", MONO_CASES)
def test_volpath_mono_sample_equals_the_restatement(gpu_rgb, name, surface, placement):
    gpu_rgb.set_variant("gpu_mono")
    try:
        assert_pinned(gpu_rgb, name, surface, placement, "volpath", mono=True)
    finally:
        gpu_rgb.set_variant("gpu_rgb")


# ================================================================ b. the rows
def film_of(pkg, monkeypatch, d, kernel, row, textured):
    if kernel:
        monkeypatch.setenv("MTSAMD_KERNEL", kernel)
    else:
        monkeypatch.delenv("MTSAMD_KERNEL", raising=False)
    film, st = render(pkg.load_dict(d))
    assert st["textured"] == textured and st["kernel_variant"] == row, (kernel, st["textured"], st["kernel_variant"])     # no silent fallback
    return film


@pytest.mark.parametrize("name,surface,placement", CASES)
def test_rows_agree_with_the_nested_kernel(gpu_rgb, monkeypatch, name, surface, placement):
    case = case_of(name, surface, placement)
    textured = TEXTURED[placement]
    flat = film_of(gpu_rgb, monkeypatch, case.scene, None, 1, textured)                      # `path`: the flat row, in its TEX / INST loop
    nested = film_of(gpu_rgb, monkeypatch, case.scene, "nested", 0, textured)
    assert np.all(flat[..., 4] == 4.0) and flat[..., :3].std() > 0
    assert np.array_equal(bits(flat), bits(nested))
    d = R.with_thin_medium(case.scene)
    ring = film_of(gpu_rgb, monkeypatch, d, None, 11024, textured)                           # `volpath` in the medium: the ring row
    assert ring[..., :3].std() > 0
    for kernel, row in (("nested", 0), ("flat", 1)):
        assert np.array_equal(bits(ring), bits(film_of(gpu_rgb, monkeypatch, d, kernel, row, textured))), kernel
