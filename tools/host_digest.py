"""The host scene of every description of a fixed corpus, as eight hash words (csrc/scene_host.h: digest_host_scene, host mode).

    python tools/host_digest.py > after.txt

One line `name d0 ... d7` per case: the sensor cases (tests/sensor_cases.py), the scenes of scenes.py, tests/kernel_rows.py,
tests/update_cases.py and tests/transport_cases.py, and under `loader.` the scenes the tests of the later plugins build (loader_corpus).
After each, a line `name.traverse sha256` for what traverse() is built from (traverse_digest).  No GPU is touched: mts_debug_desc_digest builds the host scene, hashes its own
arrays and frees it.  Two trees that print the same lines hand the kernels the same scenes, bit for bit, on this corpus -- the check
for a change of scene_dict.py or scene_host.cpp that is meant to change nothing (profiles/host_digest.txt).
"""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
from tests import kernel_rows, sensor_cases, transport_cases, update_cases  # noqa: E402


def corpus():
    """(name, scene dictionary, keyword arguments of build_scene_desc)"""
    for name, (builder, kw) in sensor_cases.CASES.items():
        yield "sensor." + name, builder(), kw
    small = dict(width=16, height=12, spp=4)
    yield "scenes.c1", scenes.c1_cornell(**small), {}
    yield "scenes.c2", scenes.c2_homogeneous_slab(**small), {}
    yield "scenes.c3", scenes.c3_heterogeneous(res=8, **small), {}
    yield "scenes.c3_passes", scenes.c3_heterogeneous(res=8, samples_per_pass=2, **small), {}
    yield "scenes.c3_mono", scenes.c3_heterogeneous(res=8, **small), {"mono": True}
    yield "scenes.c4", scenes.c4_atmosphere(layers=8, **small), {}
    yield "scenes.c4_one_column", scenes.c4_atmosphere(layers=8, columns=1, **small), {}
    yield "scenes.c4_three_species", scenes.c4_three_species(layers=8, **small), {}
    yield "scenes.c4_blend_chain", scenes.c4_three_species(layers=8, chain=True, **small), {}
    yield "scenes.c5_spectral", scenes.c5_atmosphere_spectral(layers=8, nodes=5, **small), {"spectral": True}
    for name, builder in kernel_rows.SCENES.items():
        yield "kernel_rows." + name, builder(), {"spectral": name.startswith("c5s") or name.endswith("_spectral")}
    a, b, _ = update_cases.spectral_edit()
    yield "update.spectral_edit_a", a, {"spectral": True}
    yield "update.spectral_edit_b", b, {"spectral": True}
    yield "transport.absorbing_slab", transport_cases.absorbing_slab(spp=4)[0], {}
    yield "transport.absorbing_slab_heterogeneous", transport_cases.absorbing_slab(spp=4, heterogeneous=True)[0], {}
    yield "transport.single_scattering_slab", transport_cases.single_scattering_slab(spp=4)[0], {}
    yield "transport.white_furnace", transport_cases.white_furnace(spp=4)[0], {}
    yield "transport.white_furnace_heterogeneous", transport_cases.white_furnace(spp=4, heterogeneous=True)[0], {}
    yield "transport.white_furnace_tabphase", transport_cases.white_furnace(spp=4, phase={"type": "tabphase", "values": scenes.hg_table(0.5, 17)}, ground=False)[0], {}


def spectral_mix():
    """tests/sensor_cases.py's spectral camera scene with a `discrete` srf, and on its colour parameters one spectrum of every kind the
    loader builds: `regular` written out and from wavelength:value pairs, `irregular`, `d65` written out and from a constant inside an
    emitter, `uniform` from a float (the dictionaries of tests/test_bins.py and tests/update_cases.py)."""
    d = sensor_cases.spectral(dict(sensor_cases.VOLPATH), dict(sensor_cases.SRF_DISCRETE))
    d["ground"]["bsdf"] = {"type": "rpv", "rho_0": {"type": "regular", "lambda_min": 300.0, "lambda_max": 900.0, "values": [0.05, 0.1, 0.3]},
                           "k": {"type": "spectrum", "value": "400:0.1, 500:0.2, 600:0.3"}, "g": -0.2}
    d["sun"]["irradiance"] = {"type": "d65", "scale": 2.0}
    d["sky"] = {"type": "constant", "radiance": {"type": "irregular", "wavelengths": "500, 600, 650", "values": "1, 2, .5"}}
    d["lamp"] = {"type": "point", "position": [0, 0, 3], "intensity": {"type": "spectrum", "value": 1.5}}
    return d


def loader_corpus():
    """What the sensor / scenes / kernel_rows / update / transport cases above do not reach of the loader: textures, BSDF trees, specular
    BSDFs, instancing, the cone, several sensors, `moment`, every spectrum plugin, a colour grid under mono -- the dictionaries the
    tests of those plugins build."""
    from tests import test_blendbsdf as tb, test_cone as tc, test_instance as ti, test_moment as tm, test_scene_dict as tsd
    from tests import test_sensors as tse, test_specular as tsp, test_textures as tt, test_twosided as tw
    checker = {"type": "checkerboard", "color0": [0.1, 0.2, 0.3], "color1": 0.05, "to_uv": tt.T.scale(4.0)}
    for suffix, kw in (("", {}), ("_mono", {"mono": True})):
        yield "loader.diffuse_bitmap" + suffix, tt.textured_c3(), kw
        yield "loader.rpv_checkerboard" + suffix, tt.base({"type": "rpv", "rho_0": tt.bitmap(tt.GREY44), "k": checker, "g": -0.2}), kw
    yield "loader.blend_constant", tb.blended_c3(), {}
    yield "loader.blend_bitmap", tt.base(tb.blend(tt.bitmap(tb.W22, filter_type="nearest"), a={"type": "diffuse", "reflectance": tt.bitmap(tt.RGB43)})), {}
    yield "loader.blend_bitmap_mono", tt.base(tb.blend(tt.bitmap(tt.RGB43))), {"mono": True}
    yield "loader.twosided_one", tw.leafy_c3(back=None), {}
    yield "loader.twosided_two", tw.leafy_c3(), {}
    yield "loader.dielectric", tsp.lake_c3(tsp.GLASS), {}
    yield "loader.conductor", tsp.lake_c3(tsp.METAL), {}
    yield "loader.conductor_mono", tsp.lake_c3(tsp.METAL), {"mono": True}
    yield "loader.twosided_conductor_diffuse", tt.base(tw.two(tsp.METAL, tb.DIFFUSE)), {}
    yield "loader.instances", ti.grove(ti.PLACES[:2]), {}
    yield "loader.cone", tc.box_with(z_cone=dict(tc.CONE, bsdf=tb.DIFFUSE)), {}
    yield "loader.cone_instanced", tc.box_with(**tc.in_a_group()), {}
    yield "loader.two_sensors", tse.wavefront_beside_scalar()[0], {}
    yield "loader.four_sensors", tse.four_sensors(), {}
    yield "loader.moment_volpath", tm.wrap(scenes.c3_heterogeneous(8, 8, 2, res=8), "vp", samples_per_pass=1), {}
    yield "loader.spectral_mix", spectral_mix(), {"spectral": True}
    yield "loader.rgb_grid_mono", tsd.variant_scene("mono"), {"mono": True}
    yield "loader.rgb_grid", tsd.variant_scene("rgb"), {}
    yield "loader.spectral_grid", tsd.variant_scene("spectral"), {"spectral": True}


def desc_digest(d, **kw):
    desc, keep = SD.build_scene_desc(d, **kw)
    out = (C.c_uint64 * 8)()
    A.check(A.lib().mts_debug_desc_digest(C.byref(desc), out))
    return tuple(out)


def traverse_digest(desc, keep):
    """What traverse() is built from: sha256 over the keys of ParameterMap(desc, keep) in order, each followed by its value's bytes."""
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for key, value in importlib.import_module("eradiate-kernel_amd").ParameterMap(desc, keep).items():
        h.update(key.encode() + np.asarray(value).tobytes())
    return h.hexdigest()


def lines(cases):
    """Per case its digest line and, for what traverse() is built from, a second line `name.traverse sha256`."""
    for name, d, kw in cases:
        yield name + " " + " ".join("%016x" % w for w in desc_digest(d, **kw))
        yield name + ".traverse " + traverse_digest(*SD.build_scene_desc(d, **kw))


if __name__ == "__main__":
    import itertools
    for line in lines(itertools.chain(corpus(), loader_corpus())):
        print(line)
