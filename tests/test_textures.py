"""`bitmap` and `checkerboard` textures behind BSDF colour parameters, on the host -- no GPU: what the loader writes into the description
(records, the per-BSDF index table, luminance in mono, shared objects, refusals), the PFM reader, XML = dict, the host scene's digest,
the keys of traverse() and their read-only rules, and what the library refuses on its side of the ABI."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
PKG = importlib.import_module("eradiate-kernel_amd")
XML = importlib.import_module("eradiate-kernel_amd.xml_io")
TIO = importlib.import_module("eradiate-kernel_amd.texture_io")
FR = importlib.import_module("eradiate-kernel_amd.fresolver")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

RNG = np.random.default_rng(5)
RGB43 = RNG.random((3, 5, 3), dtype=np.float32)                   # 5 wide, 3 high
GREY44 = RNG.random((4, 4), dtype=np.float32)


def bitmap(data, **kw):
    return dict({"type": "bitmap", "data": data}, **kw)


def base(bsdf):
    d = scenes.c1_cornell(8, 8, 2)
    d["floor"]["bsdf"] = bsdf
    return d


def describe(d, **kw):
    return SD.build_scene_desc(d, **kw)


def refusal(d, **kw):
    with pytest.raises(RuntimeError) as e:
        describe(d, **kw)
    return str(e.value)


def bsdf_row(desc, i):
    return [desc.bsdf_textures[6 * i + k] for k in range(6)]


# ---------------------------------------------------------------- description building
def test_untextured_scene_keeps_a_zeroed_tail():
    desc, keep = describe(scenes.c1_cornell(8, 8, 2))
    assert desc.texture_count == 0 and not desc.textures and not desc.bsdf_textures


def test_diffuse_bitmap_record_and_table():
    to_uv = T.translate([0.25, -0.5, 7.0]) @ T.scale([2.0, 3.0, 5.0])
    desc, keep = describe(base({"type": "diffuse", "reflectance": bitmap(RGB43, filter_type="nearest", wrap_mode="mirror", to_uv=to_uv)}))
    assert desc.texture_count == 1
    t = desc.textures[0]
    assert (t.type, t.width, t.height, t.channels, t.filter_type, t.wrap_mode) == (A.TEXTURE_BITMAP, 5, 3, 3, A.FILTER_NEAREST, A.WRAP_MIRROR)
    # extract(): the upper-left 2x2, the translation's x and y in the third column (its z is dropped), identity's last row
    assert list(t.to_uv) == [2.0, 0.0, 0.25, 0.0, 3.0, -0.5, 0.0, 0.0, 1.0]
    assert np.array_equal(np.ctypeslib.as_array(t.data, shape=(3, 5, 3)), RGB43)
    rows = [bsdf_row(desc, i) for i in range(desc.bsdf_count)]
    assert sorted(rows) == [[-1] * 6] * (desc.bsdf_count - 1) + [[0, -1, -1, -1, -1, -1]]
    floor = desc.shapes[2]                                            # back, ceiling, floor, ...: children in key order
    assert bsdf_row(desc, floor.bsdf) == [0, -1, -1, -1, -1, -1]
    assert list(desc.bsdfs[floor.bsdf].reflectance) == [0.5, 0.5, 0.5]                      # the parameter's default: what a reader without textures sees


def test_defaults_are_the_reference_s():
    desc, keep = describe(base({"type": "diffuse", "reflectance": bitmap(GREY44)}))
    t = desc.textures[0]
    assert (t.filter_type, t.wrap_mode, t.channels) == (A.FILTER_BILINEAR, A.WRAP_REPEAT, 1)
    assert list(t.to_uv) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    desc, keep = describe(base({"type": "diffuse", "reflectance": {"type": "checkerboard"}}))
    t = desc.textures[0]
    assert t.type == A.TEXTURE_CHECKERBOARD and not t.data
    assert np.allclose(list(t.color0), 0.4) and np.allclose(list(t.color1), 0.2)


def test_rpv_and_bilambertian_slots():
    checker = {"type": "checkerboard", "color0": [0.1, 0.2, 0.3], "color1": 0.05, "to_uv": T.scale(4.0)}
    desc, keep = describe(base({"type": "rpv", "rho_0": bitmap(GREY44), "k": checker, "g": -0.2}))
    row = [r for r in (bsdf_row(desc, i) for i in range(desc.bsdf_count)) if r != [-1] * 6]
    assert row == [[-1, 0, 1, -1, 0, -1]]                        # rho_c defaults to rho_0 (rpv.cpp:75-79): the same texture
    desc, keep = describe(base({"type": "rpv", "rho_0": 0.1, "rho_c": bitmap(GREY44), "g": bitmap(RGB43)}))
    row = [r for r in (bsdf_row(desc, i) for i in range(desc.bsdf_count)) if r != [-1] * 6]
    assert row == [[-1, -1, -1, 0, 1, -1]]                       # colour parameters in the loader's order: rho_0, g, k, rho_c
    desc, keep = describe(base({"type": "bilambertian", "reflectance": checker, "transmittance": bitmap(RGB43)}))
    row = [r for r in (bsdf_row(desc, i) for i in range(desc.bsdf_count)) if r != [-1] * 6]
    assert row == [[0, -1, -1, -1, -1, 1]]
    assert list(desc.textures[0].color0) == pytest.approx([0.1, 0.2, 0.3]) and list(desc.textures[0].color1) == pytest.approx([0.05] * 3)


def test_luminance_in_mono():
    desc, keep = describe(base({"type": "diffuse", "reflectance": bitmap(RGB43)}), mono=True)
    t = desc.textures[0]
    assert t.channels == 1
    f = np.float32
    lum = (RGB43[..., 0] * f(0.212671) + RGB43[..., 1] * f(0.715160)) + RGB43[..., 2] * f(0.072169)
    assert np.array_equal(np.ctypeslib.as_array(t.data, shape=(3, 5)), lum)
    desc, keep = describe(base({"type": "diffuse", "reflectance": {"type": "checkerboard", "color0": [0.9, 0.1, 0.1]}}), mono=True)
    c = list(desc.textures[0].color0)
    assert c[0] == c[1] == c[2] == pytest.approx(0.9 * 0.212671 + 0.1 * 0.715160 + 0.1 * 0.072169)


def test_a_shared_texture_appears_once():
    d = base({"type": "diffuse", "reflectance": dict(bitmap(GREY44), id="albedo_map")})
    d["right"]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "ref", "id": "albedo_map"}}
    desc, keep = describe(d)
    assert desc.texture_count == 1
    assert sorted(bsdf_row(desc, i)[0] for i in range(desc.bsdf_count)) == [-1] * (desc.bsdf_count - 2) + [0, 0]
    # declared at the scene level, referenced from two BSDFs (keys sort before "back")
    d = scenes.c1_cornell(8, 8, 2)
    d["a_map"] = dict(bitmap(GREY44), id="m")
    for wall in ("floor", "left"):
        d[wall]["bsdf"] = {"type": "diffuse", "reflectance": {"type": "ref", "id": "m"}}
    desc, keep = describe(d)
    assert desc.texture_count == 1 and sum(bsdf_row(desc, i)[0] == 0 for i in range(desc.bsdf_count)) == 2
    p = PKG.ParameterMap(desc, keep)
    assert [k for k in p.keys() if k.endswith(".data")] == ["m.data"]           # listed once: a scene-level child goes by its id (scene.cpp:237-244)


def test_refusals():
    tex = bitmap(GREY44)
    grey = scenes.c3_heterogeneous(8, 8, 2, res=8)                    # a scene the spectral variant takes (no rgb colours) ...
    grey["ground"]["bsdf"]["reflectance"] = 0.5
    describe(grey, spectral=True)
    grey["ground"]["bsdf"]["reflectance"] = tex                      # ... until its ground carries a texture
    assert "not supported in the spectral variant" in refusal(grey, spectral=True)
    d = scenes.c1_cornell(8, 8, 2)
    d["light"]["emitter"]["radiance"] = tex
    assert "Textures on emitters are not supported" in refusal(d)
    d = base({"type": "diffuse", "reflectance": tex})
    d["integrator"] = {"type": "moment", "nested": d["integrator"]}
    assert "moment" in refusal(d)
    assert refusal(base({"type": "diffuse", "reflectance": bitmap(np.zeros((4, 4, 2), np.float32))})) == "Unsupported channel count: 2 (expected 1 or 3)"
    assert "at least 2x2" in refusal(base({"type": "diffuse", "reflectance": bitmap(np.zeros((4, 1), np.float32))}))
    assert "at least 2x2" in refusal(base({"type": "diffuse", "reflectance": bitmap(np.zeros((1, 4, 3), np.float32))}))
    assert refusal(base({"type": "diffuse", "reflectance": bitmap(GREY44, filter_type="trilinear")})) == \
        "Invalid filter type \"trilinear\", must be one of: \"nearest\", or \"bilinear\"!"
    assert refusal(base({"type": "diffuse", "reflectance": bitmap(GREY44, wrap_mode="black")})) == \
        "Invalid wrap mode \"black\", must be one of: \"repeat\", \"mirror\", or \"clamp\"!"
    msg = refusal(base({"type": "diffuse", "reflectance": {"type": "bitmap", "filename": "albedo.png"}}))
    assert "PFM" in msg and "\"data\"" in msg
    assert "nested texture" in refusal(base({"type": "diffuse", "reflectance": {"type": "checkerboard", "color0": bitmap(GREY44)}}))
    assert "unreferenced" in refusal(base({"type": "diffuse", "reflectance": bitmap(GREY44, gamma=2.2)}))
    assert "NaN" in refusal(base({"type": "diffuse", "reflectance": bitmap(np.full((2, 2), np.nan, np.float32))}))


# ---------------------------------------------------------------- PFM
def write_pfm(path, img, little):
    h, w = img.shape[:2]
    with open(path, "wb") as fh:
        fh.write(("%s\n%d %d\n%s\n" % ("PF" if img.ndim == 3 else "Pf", w, h, "-1.0" if little else "1.0")).encode())
        fh.write(np.ascontiguousarray(img[::-1]).astype("<f4" if little else ">f4").tobytes())      # a PFM stores the bottom row first


@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("img", [RGB43, GREY44[:3, :]], ids=["rgb", "grey"])
def test_pfm_round_trip(tmp_path, img, little):
    path = str(tmp_path / "map.pfm")
    write_pfm(path, img, little)
    assert np.array_equal(TIO.read_pfm(path), img)
    saved = FR.file_resolver()
    FR.set_file_resolver(FR.FileResolver([str(tmp_path)]))           # resolved like meshes and .vol files
    try:
        desc, keep = describe(base({"type": "diffuse", "reflectance": {"type": "bitmap", "filename": "map.pfm"}}))
    finally:
        FR.set_file_resolver(saved)
    t = desc.textures[0]
    assert (t.width, t.height, t.channels) == (img.shape[1], img.shape[0], 3 if img.ndim == 3 else 1)
    assert np.array_equal(np.ctypeslib.as_array(t.data, shape=img.shape), img)


def test_pfm_scale_and_bad_header(tmp_path):
    path = str(tmp_path / "scaled.pfm")
    with open(path, "wb") as fh:
        fh.write(b"Pf\n2 2\n-2.0\n" + np.arange(4, dtype="<f4").tobytes())
    assert np.array_equal(TIO.read_pfm(path), np.array([[4, 6], [0, 2]], np.float32))
    with open(path, "wb") as fh:
        fh.write(b"P6\n2 2\n255\n")
    with pytest.raises(RuntimeError, match="Invalid header"):
        TIO.read_pfm(path)


# ---------------------------------------------------------------- XML = dict
def test_xml_and_dict_give_the_same_description(tmp_path):
    write_pfm(str(tmp_path / "ground.pfm"), RGB43, True)
    xml = """<scene version="2.0.0">
      <path value="%s"/>
      <integrator type="path"><integer name="max_depth" value="3"/></integrator>
      <sensor type="perspective"><transform name="to_world"><lookat origin="0, 0, 5" target="0, 0, 0" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="2"/></sampler></sensor>
      <shape type="rectangle" id="ground"><bsdf type="diffuse">
        <texture type="bitmap" name="reflectance"><string name="filename" value="ground.pfm"/><string name="filter_type" value="nearest"/>
          <string name="wrap_mode" value="clamp"/><transform name="to_uv"><scale x="2" y="3"/><translate x="0.5"/></transform></texture></bsdf></shape>
      <shape type="rectangle" id="wall"><transform name="to_world"><scale value="2"/></transform><bsdf type="diffuse">
        <texture type="checkerboard" name="reflectance"><rgb name="color0" value="0.1, 0.2, 0.3"/><float name="color1" value="0.6"/>
          <transform name="to_uv"><scale value="4"/></transform></texture></bsdf></shape>
      <emitter type="directional" id="sun"><vector name="direction" x="0" y="0" z="-1"/></emitter>
    </scene>""" % tmp_path
    saved = FR.file_resolver()
    FR.set_file_resolver(FR.FileResolver(list(saved)))               # the <path> element prepends to the resolver: give it one of its own
    try:
        from_xml, keep_x = describe(XML.xml_to_dict(xml))
    finally:
        FR.set_file_resolver(saved)
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": 3},
         "sensor": {"type": "perspective", "to_world": T.look_at([0, 0, 5], [0, 0, 0], [0, 1, 0]),
                    "film": {"type": "hdrfilm", "width": 4, "height": 4, "rfilter": {"type": "box"}}, "sampler": {"type": "independent", "sample_count": 2}},
         "ground": {"type": "rectangle", "bsdf": {"type": "diffuse", "reflectance": bitmap(RGB43, filter_type="nearest", wrap_mode="clamp",
                                                                                          to_uv=T.translate([0.5, 0, 0]) @ T.scale([2, 3, 1]))}},
         "wall": {"type": "rectangle", "to_world": T.scale(2.0),
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "checkerboard", "color0": [0.1, 0.2, 0.3], "color1": 0.6, "to_uv": T.scale(4.0)}}},
         "sun": {"type": "directional", "direction": [0, 0, -1]}}
    from_dict, keep_d = describe(d)
    assert from_xml.texture_count == from_dict.texture_count == 2
    assert desc_digest(from_xml) == desc_digest(from_dict)
    for i in range(2):
        a, b = from_xml.textures[i], from_dict.textures[i]
        for name, _ in A.Texture._fields_:
            if name != "data":
                va, vb = getattr(a, name), getattr(b, name)
                assert (list(va) == list(vb)) if hasattr(va, "__len__") else (va == vb), name
    assert [from_xml.bsdf_textures[k] for k in range(12)] == [from_dict.bsdf_textures[k] for k in range(12)]


# ---------------------------------------------------------------- digest of the host scene
def desc_digest(desc):
    out = (C.c_uint64 * 8)()
    A.check(A.lib().mts_debug_desc_digest(C.byref(desc), out))
    return tuple(out)


def dict_digest(d, **kw):
    desc, keep = describe(d, **kw)                                   # `keep` owns what the description points to
    return desc_digest(desc)


def textured_c3(data=RGB43, to_uv=None, **kw):
    d = scenes.c3_heterogeneous(8, 8, 2, res=8)
    d["ground"]["bsdf"]["reflectance"] = bitmap(data, to_uv=T.scale([2.0, 3.0, 1.0]) if to_uv is None else to_uv, **kw)
    return d


def changed(a, b):
    return {k for k in range(8) if a[k] != b[k]}


def test_digest_repeats_and_tells_texels_from_records():
    first = dict_digest(textured_c3())
    assert first == dict_digest(textured_c3()) and all(first)
    texel = RGB43.copy()
    texel[1, 2, 0] += np.float32(0.125)
    assert changed(first, dict_digest(textured_c3(texel))) == {3}
    assert changed(first, dict_digest(textured_c3(to_uv=T.scale([2.0, 3.5, 1.0])))) == {0}
    assert changed(first, dict_digest(textured_c3(wrap_mode="clamp"))) == {0}
    # the textured scene against the plain one: records, texels, and the traits in the header (a textured scene promises nothing)
    plain = dict_digest(scenes.c3_heterogeneous(8, 8, 2, res=8))
    assert changed(first, plain) == {0, 3, 5}


def test_a_textured_scene_keeps_its_row_of_the_kernel_table_on_the_general_unit():
    L = A.lib()
    L.mts_debug_scene_traits.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    L.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    t, v = C.c_int32(-1), C.c_int32(-1)
    desc, keep = describe(textured_c3())
    A.check(L.mts_debug_scene_traits(C.byref(desc), C.byref(t)))
    A.check(L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)))
    assert t.value == 0 and v.value == 11024                      # ring 1024, general unit (the plain scene: 111024, lean unit a)
    d = base({"type": "diffuse", "reflectance": bitmap(GREY44)})
    desc, keep = describe(d)
    A.check(L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)))
    assert v.value == 1                                           # `path`: the flat row


# ---------------------------------------------------------------- traverse()
def rpv_scene():
    d = scenes.c4_atmosphere(8, 8, 2, layers=8)
    d["ground"]["bsdf"] = {"type": "rpv", "rho_0": bitmap(RGB43, to_uv=T.scale(2.0)), "k": {"type": "checkerboard", "color0": 0.7, "color1": [0.5, 0.6, 0.7]}, "g": -0.2}
    return d


def test_parameter_map_keys_and_read_only_rules():
    desc, keep = describe(rpv_scene())
    p = PKG.ParameterMap(desc, keep)
    ground = [k for k in p.keys() if k.startswith("ground.bsdf.")]
    assert ground == ["ground.bsdf.rho_0.data", "ground.bsdf.rho_0.resolution", "ground.bsdf.rho_0.transform", "ground.bsdf.g.value",
                      "ground.bsdf.k.transform", "ground.bsdf.k.color0.value", "ground.bsdf.k.color1.value"]
    assert np.array_equal(p["ground.bsdf.rho_0.data"], RGB43) and p["ground.bsdf.rho_0.data"].shape == (3, 5, 3)
    assert p["ground.bsdf.rho_0.resolution"] == (5, 3)
    assert np.array_equal(p["ground.bsdf.rho_0.transform"], np.diag([2, 2, 1]).astype(np.float32))
    assert np.allclose(p["ground.bsdf.k.color1.value"], [0.5, 0.6, 0.7])
    for key in ("ground.bsdf.rho_0.resolution", "ground.bsdf.rho_0.transform", "ground.bsdf.k.transform"):
        with pytest.raises(RuntimeError, match="read-only"):
            p[key] = 1
    # the key sets of untextured scenes are what they were
    plain = PKG.ParameterMap(*describe(scenes.c4_atmosphere(8, 8, 2, layers=8)))
    assert [k for k in plain.keys() if k.startswith("ground.bsdf.")] == ["ground.bsdf.rho_0.value", "ground.bsdf.g.value", "ground.bsdf.k.value"]


def test_update_rewrites_the_description_and_refuses_another_shape():
    d = rpv_scene()
    desc, keep = describe(d)
    p = PKG.ParameterMap(desc, keep)
    new = RNG.random((3, 5, 3), dtype=np.float32)
    p["ground.bsdf.rho_0.data"] = new
    p["ground.bsdf.k.color0.value"] = [0.2, 0.3, 0.4]
    p.update()
    e = copy.deepcopy(d)
    e["ground"]["bsdf"]["rho_0"]["data"] = new
    e["ground"]["bsdf"]["k"]["color0"] = [0.2, 0.3, 0.4]
    assert desc_digest(desc) == dict_digest(e)
    assert np.array_equal(p["ground.bsdf.rho_0.data"], new)
    before = desc_digest(desc)
    for wrong in (np.zeros((5, 3, 3), np.float32), np.zeros((3, 5), np.float32), np.zeros((3, 6, 3), np.float32)):
        p["ground.bsdf.rho_0.data"] = wrong
        with pytest.raises(RuntimeError, match="the topology of a scene is frozen"):
            p.update()
        assert desc_digest(desc) == before and np.array_equal(p["ground.bsdf.rho_0.data"], new)
    p["ground.bsdf.rho_0.data"] = np.full((3, 5, 3), np.nan, np.float32)
    with pytest.raises(RuntimeError, match="NaN"):
        p.update()
    assert desc_digest(desc) == before


# ---------------------------------------------------------------- the library's own refusals (host-only path of mts_scene_update)
def plan(before, after, items):
    L = A.lib()
    dirty = (A.Dirty * max(len(items), 1))()
    for r, (obj, idx) in zip(dirty, items):
        r.object, r.index, r.device_data = obj, idx, None
    t, v = C.c_int32(-1), C.c_int32(-1)
    rc = L.mts_debug_update_plan(C.byref(before), C.byref(after), dirty, len(items), C.byref(t), C.byref(v))
    return rc, (L.mts_last_error() or b"").decode(), t.value, v.value


def library_refusal(desc):
    with pytest.raises(RuntimeError) as e:
        desc_digest(desc)
    return str(e.value)


def test_library_refuses_what_the_loader_would():
    def poked(poke, d=None, **kw):
        desc, keep = describe(textured_c3() if d is None else d, **kw)
        poke(desc)
        return library_refusal(desc)
    assert poked(lambda s: setattr(s.textures[0], "channels", 2)) == "texture 0: Unsupported channel count: 2 (expected 1 or 3)"
    assert "at least 2x2" in poked(lambda s: setattr(s.textures[0], "width", 1))
    assert "Invalid filter type" in poked(lambda s: setattr(s.textures[0], "filter_type", 2))
    assert "Invalid wrap mode" in poked(lambda s: setattr(s.textures[0], "wrap_mode", 3))
    assert "unknown texture type" in poked(lambda s: setattr(s.textures[0], "type", 2))
    assert "bitmap without data" in poked(lambda s: setattr(s.textures[0], "data", A.fp()))
    assert "index out of range: bsdf" in poked(lambda s: s.bsdf_textures.__setitem__(0, 1))
    assert "index out of range: bsdf" in poked(lambda s: s.bsdf_textures.__setitem__(0, -2))
    assert "records missing" in poked(lambda s: setattr(s, "textures", C.POINTER(A.Texture)()))
    assert "to_uv" in poked(lambda s: s.textures[0].to_uv.__setitem__(4, float("nan")))
    assert "spectral variant" in poked(lambda s: setattr(s.integrator, "spectral", 1))
    assert "moment" in poked(lambda s: setattr(s.integrator, "moment", 1))
    assert "monochromatic scene takes single-channel" in poked(lambda s: setattr(s.integrator, "monochrome", 1))
    nan = RGB43.copy()
    nan[2, 4, 1] = np.nan
    desc, keep = describe(textured_c3())
    keep.keep.append(nan)
    desc.textures[0].data = nan.ctypes.data_as(A.fp)
    assert "contains NaN" in library_refusal(desc)
    # an index table without records: nothing but -1 is in range
    desc, keep = describe(scenes.c3_heterogeneous(8, 8, 2, res=8))
    table = (A.i32 * (6 * desc.bsdf_count))(*([-1] * (6 * desc.bsdf_count)))
    desc.bsdf_textures = table
    plain = desc_digest(desc)
    assert plain == dict_digest(scenes.c3_heterogeneous(8, 8, 2, res=8))
    table[0] = 0
    assert "index out of range: bsdf" in library_refusal(desc)


def test_update_plan_with_textures():
    da, ka = describe(textured_c3())
    texel = RGB43.copy()
    texel[0, 0, 0] = 0.75
    db, kb = describe(textured_c3(texel))
    rc, msg, traits, kernel = plan(da, db, [(A.OBJ_TEXTURE, 0)])
    assert rc == 0 and traits == 0 and kernel == 11024, msg
    for other, field in ((textured_c3(RGB43[:, :4].copy()), "'width'"), (textured_c3(RGB43[..., 0].copy()), "'channels'"),
                         (textured_c3(wrap_mode="clamp"), "'wrap_mode'"), (textured_c3(filter_type="nearest"), "'filter_type'"),
                         (textured_c3(to_uv=T.scale(2.0)), "'to_uv'")):
        dc, kc = describe(other)
        rc, msg, _, _ = plan(da, dc, [(A.OBJ_TEXTURE, 0)])
        assert rc != 0 and field in msg and "the topology of a scene is frozen" in msg, msg
    rc, msg, _, _ = plan(da, db, [(A.OBJ_TEXTURE, 1)])
    assert rc != 0 and "texture 1: index out of range" in msg
    # a BSDF's texture indices are topology
    dc, kc = describe(scenes.c3_heterogeneous(8, 8, 2, res=8))
    ground = [i for i in range(da.bsdf_count) if bsdf_row(da, i)[0] == 0][0]
    rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, ground)])
    assert rc != 0 and "record counts differ" in msg
    dd, kd = describe(textured_c3())
    dd.bsdf_textures[6 * ground] = -1
    rc, msg, _, _ = plan(da, dd, [(A.OBJ_BSDF, ground)])
    assert rc != 0 and "'bsdf_textures'" in msg


def test_abi_additions():
    L = A.lib()
    assert A.MTS_ABI_VERSION == L.mts_abi_version() == 12
    assert L.mts_abi_sizeof(b"mts_texture") == C.sizeof(A.Texture)
    assert L.mts_abi_sizeof(b"mts_scene_desc") == C.sizeof(A.SceneDesc) and L.mts_abi_sizeof(b"mts_stats") == C.sizeof(A.Stats)
    assert A.SceneDesc.textures.offset > A.SceneDesc.spectrum_count.offset           # appended: everything before keeps its offset
    assert A.Stats.textured.offset > A.Stats.calibration_ms.offset
    assert A.OBJ_TEXTURE == 6 and "mts_texture" in A.ABI_STRUCTS
