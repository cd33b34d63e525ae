"""traverse() / ParameterMap without a GPU: the key sets, "an updated description is the description a fresh load_dict of the edited
dictionary produces" (through the CPU restatement, bit for bit), the host half of mts_scene_update (mts_debug_update_plan: traits
and kernel choice follow the update), and what an update refuses."""
import copy
import ctypes as C
import importlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
PKG = importlib.import_module("eradiate-kernel_amd")
from tests import oracle_binding as ob                                      # noqa: E402
from tests import update_cases                                              # noqa: E402


@pytest.fixture(scope="module")
def L():
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    return A.lib()


def test_import_line_of_the_reference(L):
    from mitsuba_amd.python.util import traverse, ParameterMap
    assert traverse is PKG.traverse and ParameterMap is PKG.ParameterMap


def pmap(d, **kw):
    desc, keep = SD.build_scene_desc(d, **kw)
    return PKG.ParameterMap(desc, keep), desc, keep


# ---------------------------------------------------------------- key sets (written out from the reference's traverse() methods)
GRID = ["data", "size"]
C4_MEDIUM = (["atmosphere.interior_medium.scale"] + ["atmosphere.interior_medium.albedo." + k for k in GRID]
             + ["atmosphere.interior_medium.sigma_t." + k for k in GRID])
KEYS = {
    "c4": ["atmosphere.to_world"] + C4_MEDIUM + ["atmosphere.interior_medium.phase_function.weight." + k for k in GRID]
          + ["atmosphere.interior_medium.phase_function.phase_1.values", "ground.to_world", "ground.bsdf.rho_0.value", "ground.bsdf.g.value",
             "ground.bsdf.k.value", "sun.irradiance.value"],
    "c3": ["ground.to_world", "ground.bsdf.reflectance.value", "slab.to_world", "slab.interior_medium.scale"]
          + ["slab.interior_medium.albedo." + k for k in GRID] + ["slab.interior_medium.sigma_t." + k for k in GRID]
          + ["slab.interior_medium.phase_function.g", "sun.irradiance.value"],
    "c1": [w + k for w in ("back", "ceiling", "floor", "left") for k in (".to_world", ".bsdf.reflectance.value")]
          + ["light.to_world", "light.emitter.radiance.value", "right.to_world", "right.bsdf.reflectance.value"],
    "three": ["atmosphere.to_world"] + C4_MEDIUM + ["atmosphere.interior_medium.phase_function.weight." + k for k in GRID]
             + ["atmosphere.interior_medium.phase_function.phase_0.weight." + k for k in GRID]
             + ["atmosphere.interior_medium.phase_function.phase_0.phase_1.values", "atmosphere.interior_medium.phase_function.phase_1.g",
                "ground.to_world", "ground.bsdf.rho_0.value", "ground.bsdf.g.value", "ground.bsdf.k.value", "sun.irradiance.value"],
}


@pytest.mark.parametrize("name", sorted(KEYS))
def test_key_set(name):
    d = {"c4": lambda: scenes.c4_atmosphere(16, 16, 16), "c3": lambda: scenes.c3_heterogeneous(32, 32, 16, res=16),
         "c1": lambda: scenes.c1_cornell(32, 32, 16), "three": lambda: scenes.c4_three_species(16, 16, 16)}[name]()
    p, desc, keep = pmap(d)
    assert list(p.keys()) == KEYS[name]
    assert len(p) == len(KEYS[name]) and all(k in p for k in KEYS[name]) and "nonsense" not in p
    assert [k for k, _ in p.items()] == KEYS[name]
    assert repr(p).startswith("ParameterMap[") and all(k in repr(p) for k in KEYS[name])
    for k in KEYS[name]:                                                     # geometry and sizes are listed, readable and read-only
        if k.endswith(".to_world"):
            assert np.asarray(p[k]).shape == (4, 4)
            with pytest.raises(RuntimeError, match="geometry updates are not supported yet"):
                p[k] = np.eye(4)
        if k.endswith(".size"):
            with pytest.raises(RuntimeError, match="read-only"):
                p[k] = (1, 2, 3)
    p.keep(KEYS[name][:2])
    assert list(p.keys()) == KEYS[name][:2]


def test_shared_objects_appear_once_and_names_do_not_clash():
    d = scenes.c2_homogeneous_slab(16, 16, 4)
    d["fog"] = {"type": "homogeneous", "id": "fog", "sigma_t": 0.5, "albedo": {"type": "rgb", "value": [0.9, 0.8, 0.7]}, "phase": {"type": "hg", "g": 0.3}}
    d["slab"]["interior"] = {"type": "ref", "id": "fog"}
    d["slab_2"] = dict(d["slab"], to_world=d["slab"]["to_world"], exterior={"type": "ref", "id": "fog"})
    p, desc, keep = pmap(d)
    keys = list(p.keys())
    # `fog` sorts first: the medium is reached at the scene level and not listed again below the two shapes that refer to it
    assert [k for k in keys if "scale" in k] == ["fog.scale"]
    assert "fog.phase_function.g" in keys and "fog.albedo.color.value" in keys and "fog.sigma_t.color.value" in keys
    assert not [k for k in keys if "interior_medium" in k or "exterior_medium" in k]
    # the reference's suffixes for clashing names (util.py:157-162)
    q, _, _ = pmap({"type": "scene", "a": dict(d["ground"], id="same"), "b": dict(d["ground"], id="same"), "c": dict(d["ground"], id="same"),
                    "sensor": d["sensor"]})
    assert [k for k in q.keys() if k.endswith("to_world")] == ["same.to_world", "same_1.to_world", "same_2.to_world"]


def test_mesh_buffers_are_listed_read_only():
    d = scenes.c1_cornell(16, 16, 2)
    d["blob"] = {"type": "mesh", "vertex_positions": np.eye(3, dtype=np.float32), "faces": np.array([[0, 1, 2]], np.uint32)}
    p, _, _ = pmap(d)
    assert p["blob.vertex_count"] == 3 and p["blob.face_count"] == 1 and p["blob.vertex_positions_buf"].size == 9 and p["blob.faces_buf"].tolist() == [0, 1, 2]
    with pytest.raises(RuntimeError, match="geometry updates are not supported yet"):
        p["blob.vertex_positions_buf"] = np.zeros(9)


# ---------------------------------------------------------------- update == fresh load, through the oracle
def tab(g, n=181):
    return scenes.hg_table(g, n)


def edited_c4(columns=2, third=False):
    """(A, B, assignments): the C4 atmosphere and the same dictionary with new grids, scale, tabphase table, rpv parameters and irradiance."""
    a = scenes.c4_three_species(16, 16, 8, layers=8) if third else scenes.c4_atmosphere(16, 16, 8, layers=8, columns=columns)
    b = copy.deepcopy(a)
    med = b["atmosphere"]["interior"]
    rng = np.random.default_rng(7)
    shape = med["sigma_t"]["data"].shape
    sig = (med["sigma_t"]["data"] * (0.5 + rng.random(shape[0], dtype=np.float32))[:, None, None]).astype(np.float32)
    alb = np.ascontiguousarray(np.broadcast_to(np.linspace(0.95, 0.6, shape[0], dtype=np.float32)[:, None, None], shape))
    med["sigma_t"]["data"], med["albedo"]["data"], med["scale"] = sig, alb, 1.75
    ph = med["phase"]["phase_0"] if third else med["phase"]
    ph["phase_1"]["values"] = tab(0.55)
    b["ground"]["bsdf"].update(rho_0=0.2, k=0.8, g=-0.1)
    b["sun"]["irradiance"] = {"type": "rgb", "value": [2.0, 1.5, 0.5]}
    pre = "atmosphere.interior_medium."
    sets = {pre + "sigma_t.data": sig, pre + "albedo.data": alb, pre + "scale": 1.75,
            pre + ("phase_function.phase_0.phase_1.values" if third else "phase_function.phase_1.values"): tab(0.55),
            "ground.bsdf.rho_0.value": 0.2, "ground.bsdf.k.value": 0.8, "ground.bsdf.g.value": -0.1,
            "sun.irradiance.value": {"type": "rgb", "value": [2.0, 1.5, 0.5]}}
    if third:
        med["phase"]["phase_1"]["g"] = -0.4
        sets[pre + "phase_function.phase_1.g"] = -0.4
    return a, b, sets


def edited_c3():
    a = scenes.c3_heterogeneous(16, 16, 8, res=8)
    b = copy.deepcopy(a)
    med = b["slab"]["interior"]
    sig = scenes.c3_sigma_t_grid(8, seed=99) * np.float32(1.5)
    alb = (0.5 + 0.4 * np.random.default_rng(3).random((8, 8, 8), dtype=np.float32)).astype(np.float32)
    med["sigma_t"]["data"], med["albedo"]["data"], med["scale"], med["phase"]["g"] = sig, alb, 0.6, -0.35
    b["ground"]["bsdf"]["reflectance"] = {"type": "rgb", "value": [0.9, 0.3, 0.1]}
    b["sun"]["irradiance"] = 2.5
    pre = "slab.interior_medium."
    return a, b, {pre + "sigma_t.data": sig, pre + "albedo.data": alb, pre + "scale": 0.6, pre + "phase_function.g": -0.35,
                  "ground.bsdf.reflectance.value": {"type": "rgb", "value": [0.9, 0.3, 0.1]}, "sun.irradiance.value": 2.5}


@pytest.mark.parametrize("mono", [False, True], ids=["rgb", "mono"])
@pytest.mark.parametrize("case", ["c4", "c4_one_column", "three_species", "c3"])
def test_update_equals_fresh_load_through_the_oracle(L, case, mono):
    a, b, sets = {"c4": edited_c4, "c4_one_column": lambda: edited_c4(columns=1), "three_species": lambda: edited_c4(third=True), "c3": edited_c3}[case]()
    p, desc, keep = pmap(a, mono=mono)
    before = ob.OracleScene(desc=desc, keep=keep, mono=mono).render()
    for k, v in sets.items():
        p[k] = v
    assert np.array_equal(ob.OracleScene(desc=desc, keep=keep, mono=mono).render(), before)      # assignments only mark and store
    p.update()
    updated = ob.OracleScene(desc=desc, keep=keep, mono=mono).render()
    fresh = ob.OracleScene(scene_dict=b, mono=mono).render()
    assert not np.array_equal(updated, before)
    assert np.array_equal(updated.view(np.uint32), fresh.view(np.uint32))
    for k, v in sets.items():                                                # ... and reads back what a load would hold
        if k.endswith(".data"):
            assert np.array_equal(p[k].reshape(-1), np.asarray(v, np.float32).reshape(-1))


def test_update_equals_fresh_load_spectral(L):
    if not os.path.exists(os.path.join(ROOT, "oracle", "liboracle_spectral.so")):
        pytest.skip("liboracle_spectral.so is not built")
    a, b, sets = update_cases.spectral_edit()
    p, desc, keep = pmap(a, spectral=True)
    for k, v in sets.items():
        p[k] = v
    p.update()
    updated = ob.OracleScene(desc=desc, keep=keep, spectral=True).render()
    fresh = ob.OracleScene(scene_dict=b, spectral=True).render()
    assert np.array_equal(updated.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(updated, ob.OracleScene(scene_dict=a, spectral=True).render())


# ---------------------------------------------------------------- the host half of mts_scene_update
def dirty_array(items):
    recs = (A.Dirty * max(len(items), 1))()
    for r, it in zip(recs, items):
        r.object, r.index = it[0], it[1]
        r.device_data = it[2] if len(it) > 2 else None
    return recs


def plan(L, before, after, items):
    t, v = C.c_int32(-1), C.c_int32(-1)
    rc = L.mts_debug_update_plan(C.byref(before) if before is not None else None, C.byref(after) if after is not None else None,
                                 dirty_array(items), len(items), C.byref(t), C.byref(v))
    return rc, (L.mts_last_error() or b"").decode(), t.value, v.value


def fresh(L, desc):
    t, v = C.c_int32(-1), C.c_int32(-1)
    L.mts_debug_scene_traits.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    assert L.mts_debug_scene_traits(C.byref(desc), C.byref(t)) == 0 and L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)) == 0, L.mts_last_error()
    return t.value, v.value


def all_dirty(desc):
    return ([(A.OBJ_VOLUME, i) for i in range(desc.volume_count)] + [(A.OBJ_PHASE, i) for i in range(desc.phase_count)]
            + [(A.OBJ_MEDIUM, i) for i in range(desc.medium_count)] + [(A.OBJ_BSDF, i) for i in range(desc.bsdf_count)]
            + [(A.OBJ_EMITTER, i) for i in range(desc.emitter_count)] + [(A.OBJ_SPECTRUM, i) for i in range(desc.spectrum_count)])


def x_varying(d, which=("sigma_t",)):
    d = copy.deepcopy(d)
    for w in which:
        g = d["atmosphere"]["interior"][w]["data"].copy()
        g[-1, -1, -1] *= np.float32(1.5)                                     # the last column of the last slice
        d["atmosphere"]["interior"][w]["data"] = g
    return d


def test_plan_follows_columns_equal(L):
    """A z-profile grid becomes x-varying and back: DVolume::columns_equal / bit 1 of DMedium::pair_affine, hence the majorant and the traits."""
    prof = scenes.c4_atmosphere(16, 16, 8, layers=8)
    for a, b in ((prof, x_varying(prof)), (x_varying(prof), prof), (prof, x_varying(prof, ("albedo",)))):
        da, ka = SD.build_scene_desc(a)
        db, kb = SD.build_scene_desc(b)
        med = da.media[0]
        for items in ([(A.OBJ_VOLUME, med.sigma_t_volume), (A.OBJ_VOLUME, med.albedo_volume)], all_dirty(da)):
            rc, msg, t, v = plan(L, da, db, items)
            assert rc == 0, msg
            assert (t, v) == fresh(L, db)


def test_plan_updated_description_is_the_fresh_one(L):
    """The description a ParameterMap rewrote gives, as an update of A, the traits and the kernel of a fresh B -- volpath and volpathmis, rgb and mono."""
    for integ in ("volpath", "volpathmis"):
        for mono in (False, True):
            a, b, sets = edited_c4()
            a["integrator"]["type"] = b["integrator"]["type"] = integ
            da, ka = SD.build_scene_desc(a, mono=mono)
            p, dp, kp = pmap(a, mono=mono)
            for k, val in sets.items():
                p[k] = val
            p.update()
            rc, msg, t, v = plan(L, da, dp, all_dirty(da))
            assert rc == 0, msg
            db, kb = SD.build_scene_desc(b, mono=mono)
            assert (t, v) == fresh(L, db)


def test_plan_grey_constvolume_becomes_coloured_and_back(L, monkeypatch):
    monkeypatch.delenv("MTSAMD_LEAN", raising=False)
    grey = scenes.c2_homogeneous_slab(16, 16, 4)
    col = copy.deepcopy(grey)
    col["slab"]["interior"]["albedo"] = {"type": "rgb", "value": [0.9, 0.5, 0.2]}
    dg, kg = SD.build_scene_desc(grey)
    dc, kc = SD.build_scene_desc(col)
    alb = dg.media[0].albedo_volume
    # (DMedium::grey, the homogeneous kernels' fast path, follows: tests/test_gpu_scene_update.py compares the device records and the film)
    for a, b in ((dg, dc), (dc, dg)):
        rc, msg, t, v = plan(L, a, b, [(A.OBJ_VOLUME, alb)])
        assert rc == 0, msg
        assert (t, v) == fresh(L, b)
    # through the map: the colour goes through load_dict's helper
    p, dp, kp = pmap(grey)
    p["slab.interior_medium.albedo.color.value"] = {"type": "rgb", "value": [0.9, 0.5, 0.2]}
    p.update()
    assert list(dp.volumes[alb].value) == list(dc.volumes[alb].value)
    assert plan(L, dg, dp, [(A.OBJ_VOLUME, alb)])[2:] == fresh(L, dc)


def test_plan_max_value_override_survives(L):
    a = scenes.c3_heterogeneous(16, 16, 4, res=8)
    a["slab"]["interior"]["sigma_t"]["max_value"] = 7.5
    b = copy.deepcopy(a)
    b["slab"]["interior"]["sigma_t"]["data"] = a["slab"]["interior"]["sigma_t"]["data"] * np.float32(0.5)
    p, dp, kp = pmap(a)
    p["slab.interior_medium.sigma_t.data"] = b["slab"]["interior"]["sigma_t"]["data"]
    p.update()
    v = dp.volumes[dp.media[0].sigma_t_volume]
    assert v.has_max_value == 1 and v.max_value == 7.5
    da, _ka = SD.build_scene_desc(a)
    db, _kb = SD.build_scene_desc(b)
    assert plan(L, da, dp, all_dirty(da))[:1] == (0,) and plan(L, da, dp, all_dirty(da))[2:] == fresh(L, db)
    assert np.array_equal(ob.OracleScene(desc=dp, keep=kp).render().view(np.uint32), ob.OracleScene(scene_dict=b).render().view(np.uint32))


# ---------------------------------------------------------------- refusals
def test_refusals_of_the_update_entry(L):
    base = scenes.c4_atmosphere(16, 16, 4, layers=8)
    da, ka = SD.build_scene_desc(base)
    med = da.media[0]
    sig, alb = med.sigma_t_volume, med.albedo_volume
    tab_i = next(i for i in range(da.phase_count) if da.phases[i].type == A.PHASE_TABULATED)

    def refused(change, items, *expect, d=base, **kw):
        b = copy.deepcopy(d)
        change(b)
        db, kb = SD.build_scene_desc(b, **kw)
        if kw or d is not base:
            before, _k = SD.build_scene_desc(d, **kw)
        else:
            before = da
        rc, msg, _t, _v = plan(L, before, db, items)
        assert rc != 0 and all(e in msg for e in expect), msg
        assert fresh(L, before)                                              # the description is still a valid one

    def grid_size(b):
        g = b["atmosphere"]["interior"]["sigma_t"]
        g["data"] = np.concatenate([g["data"], g["data"]], axis=0)
    refused(grid_size, [(A.OBJ_VOLUME, sig)], "volume %d" % sig, "'nz'")

    def channels(b):
        g = b["atmosphere"]["interior"]["albedo"]
        g["data"] = np.repeat(g["data"][..., None], 3, axis=3)
    refused(channels, [(A.OBJ_VOLUME, alb)], "volume %d" % alb, "'channels'")

    def vol_type(b):
        b["atmosphere"]["interior"]["albedo"] = 0.5
    refused(vol_type, [(A.OBJ_VOLUME, alb)], "volume %d" % alb, "'type'")

    def phase_type(b):
        b["atmosphere"]["interior"]["phase"]["phase_1"] = {"type": "hg", "g": 0.2}
    refused(phase_type, [(A.OBJ_PHASE, tab_i)], "phase %d" % tab_i, "'type'")

    def table_length(b):
        b["atmosphere"]["interior"]["phase"]["phase_1"]["values"] = tab(0.7, 91)
    refused(table_length, [(A.OBJ_PHASE, tab_i)], "phase %d" % tab_i, "'tab_count'")

    # a negative entry (the constructor of a fresh scene refuses it too: the description is edited after the build)
    db, kb = SD.build_scene_desc(base)
    bad = np.ascontiguousarray(np.concatenate([[-0.1], np.ones(180)]).astype(np.float32))
    db.phases[tab_i].tab_values = bad.ctypes.data_as(A.fp)
    rc, msg, _t, _v = plan(L, da, db, [(A.OBJ_PHASE, tab_i)])
    assert rc != 0 and "phase %d" % tab_i in msg and "'tab_values'" in msg and "non-negative" in msg, msg

    c3 = scenes.c3_heterogeneous(16, 16, 4, res=8)
    d3, k3 = SD.build_scene_desc(c3)
    e3, l3 = SD.build_scene_desc(c3)
    hg_i = d3.media[0].phase
    e3.phases[hg_i].g = 1.0
    rc, msg, _t, _v = plan(L, d3, e3, [(A.OBJ_PHASE, hg_i)])
    assert rc != 0 and "phase %d" % hg_i in msg and "'g'" in msg and "(-1, 1)" in msg, msg

    for items in ([(A.OBJ_VOLUME, da.volume_count)], [(A.OBJ_VOLUME, -1)], [(A.OBJ_MEDIUM, 7)], [(A.OBJ_SPECTRUM, 0)], [(A.OBJ_BSDF, da.bsdf_count)]):
        rc, msg, _t, _v = plan(L, da, da, items)
        assert rc != 0 and "index out of range" in msg, msg
    rc, msg, _t, _v = plan(L, da, da, [(9, 0)])
    assert rc != 0 and "unknown object kind" in msg, msg

    # device_data: grids of a scene in device memory only -- never a constvolume, a phase function, or a host-only scene
    slab, ks = SD.build_scene_desc(scenes.c2_homogeneous_slab(16, 16, 4))
    word = np.zeros(4, np.float32)
    rc, msg, _t, _v = plan(L, slab, slab, [(A.OBJ_VOLUME, slab.media[0].albedo_volume, word.ctypes.data)])
    assert rc != 0 and "device_data" in msg and "volume %d" % slab.media[0].albedo_volume in msg, msg
    rc, msg, _t, _v = plan(L, da, da, [(A.OBJ_PHASE, tab_i, word.ctypes.data)])
    assert rc != 0 and "device_data" in msg, msg
    rc, msg, _t, _v = plan(L, da, da, [(A.OBJ_VOLUME, sig, word.ctypes.data)])
    assert rc != 0 and "device_data" in msg, msg

    # n < 0, a NULL description, an ABI mismatch
    t, v = C.c_int32(), C.c_int32()
    assert L.mts_debug_update_plan(C.byref(da), C.byref(da), dirty_array([]), -1, C.byref(t), C.byref(v)) != 0 and b"negative" in L.mts_last_error()
    assert L.mts_debug_update_plan(C.byref(da), None, dirty_array([]), 0, C.byref(t), C.byref(v)) != 0 and b"NULL" in L.mts_last_error()
    other, ko = SD.build_scene_desc(base)
    other.abi_version = 9
    assert L.mts_debug_update_plan(C.byref(da), C.byref(other), dirty_array([]), 0, C.byref(t), C.byref(v)) != 0 and b"ABI version" in L.mts_last_error()
    assert L.mts_scene_update(None, C.byref(da), dirty_array([]), 0, None) != 0 and b"NULL" in L.mts_last_error()
    # an empty update is one
    assert plan(L, da, da, [])[2:] == fresh(L, da)


def test_refusals_of_the_map_leave_the_description_as_it_was(L):
    a = scenes.c4_atmosphere(16, 16, 4, layers=8)
    p, desc, keep = pmap(a)
    before = ob.OracleScene(desc=desc, keep=keep).render()
    pre = "atmosphere.interior_medium."
    grid = a["atmosphere"]["interior"]["sigma_t"]["data"]
    cases = [(pre + "sigma_t.data", np.concatenate([grid, grid], axis=0), "'size' / 'channels' cannot change"),
             (pre + "sigma_t.data", np.repeat(grid[..., None], 3, axis=3), "'size' / 'channels' cannot change"),
             (pre + "phase_function.phase_1.values", tab(0.7, 91), "'tab_count'"),
             (pre + "phase_function.phase_1.values", "-0.1 " + tab(0.7, 180), "non-negative"),
             ("ground.bsdf.rho_0.value", [1, 2], "colour")]
    for key, value, expect in cases:
        p[pre + "scale"] = 3.0                                               # a valid assignment in the same update is not applied either
        p[key] = value
        with pytest.raises(RuntimeError, match=expect):
            p.update()
        assert desc.media[0].scale == 1.0
        assert np.array_equal(ob.OracleScene(desc=desc, keep=keep).render(), before), key
    q, d3, k3 = pmap(scenes.c3_heterogeneous(16, 16, 4, res=8))
    q["slab.interior_medium.phase_function.g"] = 1.0
    with pytest.raises(RuntimeError, match="asymmetry"):
        q.update()
    assert abs(d3.phases[d3.media[0].phase].g - 0.8) < 1e-6 and fresh(L, d3)
    with pytest.raises(KeyError):
        q["slab.interior_medium.nothing"] = 1.0
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None:                                                    # a CPU tensor is host data like an array
        t = torch.from_numpy(scenes.c3_sigma_t_grid(8, seed=5))
        q["slab.interior_medium.sigma_t.data"] = t
        q.update()
        assert np.array_equal(q["slab.interior_medium.sigma_t.data"].reshape(-1), t.numpy().reshape(-1))


def test_repeated_updates_do_not_accumulate_arrays(L):
    """A wavelength loop updates thousands of times: every record keeps ONE live array, the replaced one is dropped."""
    import gc
    import weakref
    a, b, sets = edited_c4()
    p, desc, keep = pmap(a)
    arrays = {k: v for k, v in sets.items() if k.endswith(".data") or k.endswith(".values")}
    held, refs = None, []
    for rep in range(6):
        for k, v in arrays.items():
            v = np.array(v, np.float32) * np.float32(1.0 + 0.01 * rep) if not isinstance(v, str) else tab(0.5 + 0.01 * rep)
            p[k] = v
            if not isinstance(v, str) and rep < 5:
                refs.append(weakref.ref(v))
        del v
        p.update()
        if rep == 0:
            held = len(keep.keep)
        assert len(keep.keep) == held, rep
    gc.collect()
    assert refs and all(r() is None for r in refs[:-2])             # arrays of earlier rounds are gone (the last round's may be the live ones)
    assert fresh(L, desc)
    # the spectral variant's arrays have a slot of their own
    sa, sb, ssets = update_cases.spectral_edit()
    q, sdesc, skeep = pmap(sa, spectral=True)
    for rep in range(4):
        q["ground.bsdf.rho_0.values"] = [0.3 + 0.01 * rep, 0.2, 0.1]
        q["sun.irradiance.values"] = [0.5, 1.0 + 0.1 * rep, 2.5, 2.0]
        q.update()
        if rep == 0:
            held = (len(skeep.keep), len(skeep.spectrum_arrays))
        assert (len(skeep.keep), len(skeep.spectrum_arrays)) == held, rep
    assert abs(q["ground.bsdf.rho_0.values"][0] - 0.33) < 1e-6


def test_emitter_transform_is_frozen(L):
    a = scenes.c4_atmosphere(16, 16, 4, layers=8)
    b = copy.deepcopy(a)
    b["sun"]["direction"] = [0.0, 0.6, -0.8]
    b["sun"]["irradiance"] = 3.0
    da, ka = SD.build_scene_desc(a)
    db, kb = SD.build_scene_desc(b)
    rc, msg, _t, _v = plan(L, da, db, [(A.OBJ_EMITTER, 0)])
    assert rc != 0 and "emitter 0" in msg and "'to_world'" in msg, msg
    b["sun"]["direction"] = a["sun"]["direction"]
    dc, kc = SD.build_scene_desc(b)
    assert plan(L, da, dc, [(A.OBJ_EMITTER, 0)])[0] == 0


def test_an_update_keeps_its_variant_through_a_build_inside(L):
    """One update() of a mono scene converts a grid whose __array__ builds an rgb scene, and after it a colour: the description is that
    of a fresh mono load of the edited dictionary (the variant an update converts under is its builder's, not the last build's)."""
    from tests.test_scene_dict import RGB_GRID, BuildsInside, desc_digest, variant_scene
    new_grid = (RGB_GRID * np.float32(0.5)).astype(np.float32)
    p, desc, keep = pmap(variant_scene("mono"), mono=True)
    grid = BuildsInside("rgb", new_grid)
    p["box.interior_medium.sigma_t.data"] = grid
    p["floor.bsdf.reflectance.value"] = [0.9, 0.5, 0.1]
    p.update()
    assert len(grid.inner) == 1
    edited = variant_scene("mono", new_grid)
    edited["floor"]["bsdf"]["reflectance"] = [0.9, 0.5, 0.1]
    fresh_desc, fresh_keep = SD.build_scene_desc(edited, mono=True)
    assert desc.bsdfs[1].reflectance[0] == desc.bsdfs[1].reflectance[1] == fresh_desc.bsdfs[1].reflectance[0]
    assert desc_digest(desc) == desc_digest(fresh_desc)
