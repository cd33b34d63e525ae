"""`blendbsdf` (src/bsdfs/blendbsdf.cpp) without a GPU: loading from dictionaries and XML, the order of the children, the description's
record (MTS_BSDF_BLEND uses existing fields of mts_bsdf: the ABI stays 12), what loader and library refuse, the host plan (digest, traits,
kernel row, update plan), the keys of traverse() with an update against a fresh load, and the host side under ASan / UBSan in a
stand-alone program (tests/micro/blend_host_asan.cpp)."""
import copy
import ctypes as C
import glob
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import sensor_cases
from tests.test_textures import base, bitmap, bsdf_row, desc_digest, describe, dict_digest, plan, refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = importlib.import_module("eradiate-kernel_amd._capi")
PKG = importlib.import_module("eradiate-kernel_amd")
XML = importlib.import_module("eradiate-kernel_amd.xml_io")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

DIFFUSE = {"type": "diffuse", "reflectance": [0.2, 0.4, 0.6]}
RPV = {"type": "rpv", "rho_0": 0.3, "k": 0.6, "g": -0.2}
W22 = np.array([[0.0, 1.0], [0.5, 0.5]], np.float32)


def blend(weight=0.3, a=DIFFUSE, b=RPV, names=("first", "second")):
    return {"type": "blendbsdf", "weight": copy.deepcopy(weight), names[0]: copy.deepcopy(a), names[1]: copy.deepcopy(b)}


def blend_index(desc):
    found = [i for i in range(desc.bsdf_count) if desc.bsdfs[i].type == A.BSDF_BLEND]
    assert len(found) == 1
    return found[0]


# ---------------------------------------------------------------- loading
def test_record_of_a_constant_blend():
    desc, keep = describe(base(blend()))
    i = blend_index(desc)
    rec = desc.bsdfs[i]
    assert A.BSDF_BLEND == 4 and rec.type == 4
    assert rec.reflectance[0] == np.float32(0.3)
    c0, c1 = rec.spectrum[0], rec.spectrum[1]
    assert desc.bsdfs[c0].type == A.BSDF_DIFFUSE and desc.bsdfs[c1].type == A.BSDF_RPV and list(rec.spectrum[2:]) == [-1] * 4
    assert np.allclose(list(desc.bsdfs[c0].reflectance), [0.2, 0.4, 0.6]) and desc.bsdfs[c1].k[0] == np.float32(0.6)
    assert desc.texture_count == 0 and not desc.bsdf_textures            # a constant weight and plain children: no texture table
    assert [s for s in range(desc.shape_count) if desc.shapes[s].bsdf == i]   # the floor holds the blend, not a child


@pytest.mark.parametrize("names,first", [(("b", "a"), "a"), (("bsdf_10", "bsdf_2"), "bsdf_2"), (("_arg_1", "_arg_0"), "_arg_0"), (("zz", "aa_1"), "aa_1")])
def test_children_are_taken_in_name_order(names, first):
    """props.objects() is the name order of Properties (blendbsdf.cpp:61-69): the keys are written in the opposite order here"""
    desc, keep = describe(base(blend(names=names)))
    rec = desc.bsdfs[blend_index(desc)]
    kinds = (desc.bsdfs[rec.spectrum[0]].type, desc.bsdfs[rec.spectrum[1]].type)
    assert kinds == ((A.BSDF_RPV, A.BSDF_DIFFUSE) if first == names[1] else (A.BSDF_DIFFUSE, A.BSDF_RPV))


def test_weight_spellings():
    for w in (0.3, {"type": "spectrum", "value": 0.3}, {"type": "uniform", "value": 0.3}):
        desc, keep = describe(base(blend(w)))
        assert desc.bsdfs[blend_index(desc)].reflectance[0] == np.float32(0.3)
    for w in ([0.3, 0.3, 0.3], {"type": "rgb", "value": [0.1, 0.2, 0.3]}, {"type": "spectrum", "value": "400:0.1, 700:0.3"}):
        assert "eval_1 is not defined" in refusal(base(blend(w)))
    checker = {"type": "checkerboard", "color0": 0.0, "color1": 1.0}
    desc, keep = describe(base(blend(checker)))
    assert desc.textures[bsdf_row(desc, blend_index(desc))[0]].type == A.TEXTURE_CHECKERBOARD
    assert "eval_1 is not defined" in refusal(base(blend(dict(checker, color1=[0.1, 0.2, 0.3]))))


def test_textured_weight_and_textured_children():
    tex = bitmap(np.random.default_rng(3).random((4, 4, 3), dtype=np.float32))
    d = base(blend(bitmap(W22, filter_type="nearest"), a={"type": "diffuse", "reflectance": tex}))
    desc, keep = describe(d)
    i = blend_index(desc)
    rec = desc.bsdfs[i]
    assert desc.texture_count == 2
    row = bsdf_row(desc, i)
    assert row[0] >= 0 and row[1:] == [-1] * 5 and desc.textures[row[0]].channels == 1 and desc.textures[row[0]].filter_type == A.FILTER_NEAREST
    child = bsdf_row(desc, rec.spectrum[0])
    assert child[0] >= 0 and child[0] != row[0] and desc.textures[child[0]].channels == 3
    assert bsdf_row(desc, rec.spectrum[1]) == [-1] * 6
    # *_mono: a colour weight bitmap becomes its luminance, as every bitmap there
    mono, keep_m = describe(base(blend(tex)), mono=True)
    assert mono.textures[bsdf_row(mono, blend_index(mono))[0]].channels == 1


def test_shared_ref_children_are_one_record():
    d = base(blend(a={"type": "ref", "id": "mat"}, b={"type": "ref", "id": "mat"}))
    d["a_material"] = dict(DIFFUSE, id="mat")
    d["ceiling"]["bsdf"] = {"type": "ref", "id": "mat"}
    desc, keep = describe(d)
    rec = desc.bsdfs[blend_index(desc)]
    assert rec.spectrum[0] == rec.spectrum[1] == desc.shapes[[s for s in range(desc.shape_count) if desc.shapes[s].bsdf == rec.spectrum[0]][0]].bsdf
    assert sum(1 for i in range(desc.bsdf_count) if np.allclose(list(desc.bsdfs[i].reflectance), [0.2, 0.4, 0.6])) == 1
    # a blend declared at the scene level and referenced
    e = base({"type": "ref", "id": "mix"})
    e["a_mix"] = dict(blend(), id="mix")
    desc, keep = describe(e)
    assert desc.shapes[[s for s in range(desc.shape_count) if desc.bsdfs[desc.shapes[s].bsdf].type == A.BSDF_BLEND][0]].bsdf == blend_index(desc)


def test_xml_and_dict_give_the_same_description():
    xml = """<scene version="2.0.0">
        <bsdf type="rpv" id="veg"><float name="k" value="0.6"/><float name="g" value="-0.2"/><spectrum name="rho_0" value="0.3"/></bsdf>
        <shape type="rectangle">
            <bsdf type="blendbsdf">
                <%s name="weight" value="0.3"/>
                <bsdf type="diffuse"><rgb name="reflectance" value="0.2, 0.4, 0.6"/></bsdf>
                <ref id="veg"/>
            </bsdf>
        </shape>
        <emitter type="directional"><vector name="direction" x="0" y="0" z="-1"/></emitter>
        <sensor type="perspective"><film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/></film></sensor>
    </scene>"""
    for tag in ("float", "spectrum"):
        from_xml = XML.xml_to_dict(xml % tag)
        inner = [v for v in from_xml.values() if isinstance(v, dict) and v.get("type") == "rectangle"][0]["bsdf"]
        assert sorted(k for k in inner if k not in ("type", "weight")) == ["_arg_0", "_arg_1"]          # unnamed children (xml.cpp)
        dx, kx = describe(from_xml)
        d = copy.deepcopy(from_xml)
        [v for v in d.values() if isinstance(v, dict) and v.get("type") == "rectangle"][0]["bsdf"] = \
            {"type": "blendbsdf", "weight": 0.3, "a": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}}, "b": {"type": "ref", "id": "veg"}}
        dd, kd = describe(d)
        assert desc_digest(dx) == desc_digest(dd)
        rec = dx.bsdfs[blend_index(dx)]
        assert dx.bsdfs[rec.spectrum[0]].type == A.BSDF_DIFFUSE and dx.bsdfs[rec.spectrum[1]].type == A.BSDF_RPV
    tex = xml.replace('<%s name="weight" value="0.3"/>', '<texture type="checkerboard" name="weight"><float name="color0" value="0"/><float name="color1" value="1"/></texture>')
    dt, kt = describe(XML.xml_to_dict(tex))
    assert dt.texture_count == 1 and bsdf_row(dt, blend_index(dt))[0] == 0


def test_refusals_of_the_loader():
    # the reference's constructor errors, verbatim (blendbsdf.cpp:65,73)
    three = blend()
    three["third"] = copy.deepcopy(DIFFUSE)
    assert refusal(base(three)) == "BlendBSDF: Cannot specify more than two child BSDFs"
    one = blend()
    del one["second"]
    assert refusal(base(one)) == "BlendBSDF: Two child BSDFs must be specified!"
    none = blend()
    del none["weight"]
    assert "\"weight\" has not been specified" in refusal(base(none))
    # this backend's own: they name the plugin and where it sits
    for child, plugin in (({"type": "null"}, "\"null\""), (blend(), "\"blendbsdf\"")):
        msg = refusal(base(blend(b=child)))
        assert "\"blendbsdf\" floor.bsdf" in msg and "\"second\"" in msg and plugin in msg and "this backend" in msg, msg
    spectral = scenes.c5_atmosphere_spectral(8, 8, 2, layers=8)
    spectral["ground"]["bsdf"] = blend(a={"type": "diffuse", "reflectance": 0.5})
    msg = refusal(spectral, spectral=True)
    assert "\"blendbsdf\"" in msg and "spectral variant" in msg and "ground.bsdf" in msg, msg
    d = base(blend())
    d["integrator"] = {"type": "moment", "nested": d["integrator"]}
    msg = refusal(d)
    assert "\"blendbsdf\"" in msg and "moment" in msg and "floor.bsdf" in msg, msg
    assert "Unknown / unsupported BSDF plugin \"plastic\"" in refusal(base(blend(b={"type": "plastic"})))
    extra = blend()
    extra["roughness"] = 0.1
    assert "unreferenced property" in refusal(base(extra))


# ---------------------------------------------------------------- the library's side of the ABI
def test_abi_is_unchanged():
    L = A.lib()
    assert A.MTS_ABI_VERSION == L.mts_abi_version() == 12
    for name, cls in A.ABI_STRUCTS.items():
        assert L.mts_abi_sizeof(name.encode()) == C.sizeof(cls), name


def library_refusal(desc):
    with pytest.raises(RuntimeError) as e:
        desc_digest(desc)
    return str(e.value)


def test_refusals_of_the_library():
    def poked(poke, d=None):
        desc, keep = describe(base(blend()) if d is None else d)
        poke(desc, blend_index(desc))
        return library_refusal(desc)
    msg = poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(0, s.bsdf_count))
    assert msg.startswith("index out of range: bsdf") and "\"spectrum[0]\" (bsdf_0)" in msg, msg
    assert "index out of range" in poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(1, -1))
    msg = poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(1, i))
    assert "\"spectrum[1]\" (bsdf_1) is the blend itself" in msg, msg
    null = base(blend())
    null["ceiling"]["bsdf"] = {"type": "null"}

    def to_kind(kind):
        def poke(s, i):
            s.bsdfs[i].spectrum[0] = [k for k in range(s.bsdf_count) if s.bsdfs[k].type == kind and k != i][0]
        return poke
    msg = poked(to_kind(A.BSDF_NULL), null)
    assert "null children are not supported by this backend" in msg and "bsdf_0" in msg, msg
    two = base(blend())
    two["ceiling"]["bsdf"] = blend(0.6)
    desc, keep = describe(two)
    first, second = [i for i in range(desc.bsdf_count) if desc.bsdfs[i].type == A.BSDF_BLEND]
    desc.bsdfs[first].spectrum[1] = second
    assert "nested blends are not supported by this backend" in library_refusal(desc)
    for bad in (float("nan"), float("inf")):
        msg = poked(lambda s, i: s.bsdfs[i].reflectance.__setitem__(0, bad))
        assert "blendbsdf" in msg and "reflectance[0]" in msg and "not finite" in msg, msg
    msg = poked(lambda s, i: setattr(s.integrator, "spectral", 1))
    assert "blendbsdf is not supported in the spectral variant" in msg and msg.startswith("bsdf "), msg
    msg = poked(lambda s, i: setattr(s.integrator, "moment", 1))
    assert "blendbsdf is not supported inside a moment integrator's scene" in msg, msg
    assert "unknown BSDF type" in poked(lambda s, i: setattr(s.bsdfs[i], "type", 5))


# ---------------------------------------------------------------- host plan
def blended_c3(weight=0.3, a=DIFFUSE, b=RPV):
    d = scenes.c3_heterogeneous(8, 8, 2, res=8)
    d["ground"]["bsdf"] = blend(weight, a, b)
    return d


def test_digest_tells_weight_and_children():
    first = dict_digest(blended_c3())
    assert first == dict_digest(blended_c3()) and all(first)
    other = dict_digest(blended_c3(0.4))
    assert {k for k in range(8) if first[k] != other[k]} == {0}
    swapped = dict_digest(blended_c3(a=RPV, b=DIFFUSE))
    assert swapped[0] != first[0]


def test_digests_of_scenes_without_blends_are_the_parent_s():
    """tests/golden/host_digests_abi12.json: the eight words of every case of tests/test_host_digest.py's list, printed once by the
    commit before MTS_BSDF_BLEND"""
    import tests.test_host_digest as hd
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_digests_abi12.json")))
    assert sorted(golden) == sorted(sensor_cases.CASES)
    for case in sorted(sensor_cases.CASES):
        assert [str(w) for w in hd.digest(case)] == golden[case], case


def kernel_row(desc):
    L = A.lib()
    L.mts_debug_scene_traits.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    t, v = C.c_int32(-1), C.c_int32(-1)
    A.check(L.mts_debug_scene_traits(C.byref(desc), C.byref(t)))
    A.check(L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)))
    return t.value, v.value


def test_traits_and_kernel_row():
    MT_NO_RPV = 64                                                     # csrc/dscene.h
    plain, keep = describe(scenes.c3_heterogeneous(8, 8, 2, res=8))
    assert kernel_row(plain)[0] & MT_NO_RPV                            # the scene's own ground is diffuse
    desc, keep = describe(blended_c3())                                # its only rpv is a blend's child
    traits, row = kernel_row(desc)
    assert traits & MT_NO_RPV == 0 and traits == 0 and row == 11024    # the general unit's ring row, as a textured scene (constant weight, no texture record)
    desc, keep = describe(base(blend()))
    assert kernel_row(desc) == (0, 1)                                  # `path`: the flat row


def test_update_plan():
    da, ka = describe(blended_c3())
    db, kb = describe(blended_c3(0.4))
    i = blend_index(da)
    fresh = kernel_row(db)
    rc, msg, traits, kernel = plan(da, db, [(A.OBJ_BSDF, i)])
    assert rc == 0 and (traits, kernel) == fresh == (0, 11024), msg
    for c in (0, 1):
        dc, kc = describe(blended_c3())
        dc.bsdfs[i].spectrum[c] = dc.bsdfs[i].spectrum[1 - c]
        rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, i)])
        assert rc != 0 and "'spectrum[%d] (bsdf_%d)'" % (c, c) in msg and "the topology of a scene is frozen" in msg, msg
    dc, kc = describe(blended_c3())
    dc.bsdfs[i].type = A.BSDF_DIFFUSE
    rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, i)])
    assert rc != 0 and "'type'" in msg
    dc, kc = describe(blended_c3(float("nan")))
    rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, i)])
    assert rc != 0 and "not finite" in msg and "bsdf %d" % i in msg, msg
    # a child's colour, and a textured weight through its texture record
    child = da.bsdfs[i].spectrum[0]
    dc, kc = describe(blended_c3(a=dict(DIFFUSE, reflectance=0.9)))
    rc, msg, traits, kernel = plan(da, dc, [(A.OBJ_BSDF, child)])
    assert rc == 0 and kernel == 11024, msg
    ta, kta = describe(blended_c3(bitmap(W22, filter_type="nearest")))
    tb, ktb = describe(blended_c3(bitmap(W22[::-1].copy(), filter_type="nearest")))
    rc, msg, traits, kernel = plan(ta, tb, [(A.OBJ_TEXTURE, 0)])
    assert rc == 0 and (traits, kernel) == (0, 11024), msg


# ---------------------------------------------------------------- traverse()
def test_parameter_map_keys_and_round_trip():
    d = blended_c3(a={"type": "diffuse", "reflectance": bitmap(np.random.default_rng(3).random((4, 4, 3), dtype=np.float32))})
    desc, keep = describe(d)
    p = PKG.ParameterMap(desc, keep)
    ground = [k for k in p.keys() if k.startswith("ground.bsdf.")]
    assert ground == ["ground.bsdf.weight.value",
                      "ground.bsdf.bsdf_0.reflectance.data", "ground.bsdf.bsdf_0.reflectance.resolution", "ground.bsdf.bsdf_0.reflectance.transform",
                      "ground.bsdf.bsdf_1.rho_0.value", "ground.bsdf.bsdf_1.g.value", "ground.bsdf.bsdf_1.k.value"]
    assert p["ground.bsdf.weight.value"] == np.float32(0.3)
    new = np.random.default_rng(4).random((4, 4, 3), dtype=np.float32)
    p["ground.bsdf.weight.value"] = 0.65
    p["ground.bsdf.bsdf_0.reflectance.data"] = new
    p["ground.bsdf.bsdf_1.k.value"] = 0.8
    p.update()
    e = copy.deepcopy(d)
    e["ground"]["bsdf"]["weight"] = 0.65
    e["ground"]["bsdf"]["first"]["reflectance"]["data"] = new
    e["ground"]["bsdf"]["second"]["k"] = 0.8
    fresh, keep_f = describe(e)
    assert desc.bsdf_count == fresh.bsdf_count and desc.texture_count == fresh.texture_count
    for i in range(desc.bsdf_count):                                    # field by field
        for name, _ in A.Bsdf._fields_:
            a, b = getattr(desc.bsdfs[i], name), getattr(fresh.bsdfs[i], name)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, (i, name)
        assert bsdf_row(desc, i) == bsdf_row(fresh, i)
    assert desc_digest(desc) == desc_digest(fresh)
    assert p["ground.bsdf.weight.value"] == np.float32(0.65)
    before = desc_digest(desc)
    p["ground.bsdf.weight.value"] = [0.1, 0.2, 0.3]
    with pytest.raises(RuntimeError, match="eval_1 is not defined"):
        p.update()
    p["ground.bsdf.weight.value"] = float("nan")
    with pytest.raises(RuntimeError, match="not finite"):
        p.update()
    assert desc_digest(desc) == before and p["ground.bsdf.weight.value"] == np.float32(0.65)
    # a textured weight: the texture's keys under `weight`
    q = PKG.ParameterMap(*describe(blended_c3(bitmap(W22, filter_type="nearest"))))
    assert [k for k in q.keys() if k.startswith("ground.bsdf.weight.")] == ["ground.bsdf.weight.data", "ground.bsdf.weight.resolution", "ground.bsdf.weight.transform"]
    q = PKG.ParameterMap(*describe(blended_c3({"type": "checkerboard", "color0": 0.0, "color1": 1.0})))
    assert [k for k in q.keys() if k.startswith("ground.bsdf.weight.")] == ["ground.bsdf.weight.transform", "ground.bsdf.weight.color0.value", "ground.bsdf.weight.color1.value"]
    # scenes without a blend list what they listed
    plain = PKG.ParameterMap(*describe(scenes.c3_heterogeneous(8, 8, 2, res=8)))
    assert [k for k in plain.keys() if k.startswith("ground.bsdf.")] == ["ground.bsdf.reflectance.value"]


# ---------------------------------------------------------------- host side under ASan / UBSan: a stand-alone program, nothing loaded into Python
def test_host_side_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) or not glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64*"):
        pytest.skip("hipcc or clang's sanitizer runtime not found")
    csrc = os.path.join(ROOT, "eradiate-kernel_amd", "csrc")
    exe = str(tmp_path / "blend_host_asan")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DMTSAMD_HOST_ONLY",
                           "-Wall", "-Wno-unused-function", "-Wno-unused-result",
                           os.path.join(csrc, "scene_host.cpp"), os.path.join(csrc, "capi.cpp"), os.path.join(ROOT, "tests", "micro", "blend_host_asan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert "blend host sanitizer: 30 cases, 0 failed" in r.stdout, report
