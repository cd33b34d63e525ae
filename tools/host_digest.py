"""The host scene of every description of a fixed corpus, as eight hash words (csrc/scene_host.h: digest_host_scene, host mode).

    python tools/host_digest.py > after.txt

One line `name d0 ... d7` per case: the sensor cases (tests/sensor_cases.py), the scenes of scenes.py, tests/kernel_rows.py,
tests/update_cases.py and tests/transport_cases.py.  No GPU is touched: mts_debug_desc_digest builds the host scene, hashes its own
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


def desc_digest(d, **kw):
    desc, keep = SD.build_scene_desc(d, **kw)
    out = (C.c_uint64 * 8)()
    A.check(A.lib().mts_debug_desc_digest(C.byref(desc), out))
    return tuple(out)


if __name__ == "__main__":
    for name, d, kw in corpus():
        print(name, " ".join("%016x" % w for w in desc_digest(d, **kw)))
