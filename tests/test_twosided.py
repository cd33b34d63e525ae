"""`twosided` (src/bsdfs/twosided.cpp) without a GPU: loading from dictionaries and XML, the order of the children, the description's
record (MTS_BSDF_TWOSIDED = 6 uses existing fields of mts_bsdf: the ABI stays 12, type 5 stays unknown), what loader and library
refuse, the keys of traverse() with an update through either name, the kernel routing, and the fixture of the independent
estimator's panel problem (tests/independent/problems_twosided.py) with the mutation it must reject, and the host side under
ASan / UBSan in a stand-alone program (tests/micro/twosided_host_asan.cpp)."""
import copy
import ctypes as C
import glob
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

from tests.independent import problems_twosided, surface
from tests.test_blendbsdf import DIFFUSE, RPV, blend, kernel_row, library_refusal
from tests.test_independent_pin import GOLDEN, z_test
from tests.test_independent_surface_pin import rejected
from tests.test_textures import base, bitmap, bsdf_row, desc_digest, describe, plan, refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = importlib.import_module("eradiate-kernel_amd._capi")
PKG = importlib.import_module("eradiate-kernel_amd")
XML = importlib.import_module("eradiate-kernel_amd.xml_io")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")

BILAMBERTIAN = {"type": "bilambertian", "reflectance": 0.4, "transmittance": 0.3}
TRANSMISSION = "Only materials without a transmission component can be nested!"


def two(*children, names=("first", "second", "third")):
    out = {"type": "twosided"}
    for name, child in zip(names, children):
        out[name] = copy.deepcopy(child)
    return out


def index_of(desc, kind=None):
    found = [i for i in range(desc.bsdf_count) if desc.bsdfs[i].type == (A.BSDF_TWOSIDED if kind is None else kind)]
    assert len(found) == 1
    return found[0]


def children_of(desc):
    rec = desc.bsdfs[index_of(desc)]
    return rec.spectrum[0], rec.spectrum[1]


# ---------------------------------------------------------------- loading
def test_record_of_two_children():
    desc, keep = describe(base(two(DIFFUSE, RPV)))
    i = index_of(desc)
    rec = desc.bsdfs[i]
    assert A.BSDF_TWOSIDED == 6 and rec.type == 6
    c0, c1 = children_of(desc)
    assert desc.bsdfs[c0].type == A.BSDF_DIFFUSE and desc.bsdfs[c1].type == A.BSDF_RPV and list(rec.spectrum[2:]) == [-1] * 4
    assert desc.texture_count == 0 and not desc.bsdf_textures
    assert [s for s in range(desc.shape_count) if desc.shapes[s].bsdf == i]     # the floor holds the adapter, not a child


def test_one_child_serves_both_sides():
    desc, keep = describe(base(two(RPV)))
    c0, c1 = children_of(desc)
    assert c0 == c1 and desc.bsdfs[c0].type == A.BSDF_RPV
    assert sum(1 for i in range(desc.bsdf_count) if desc.bsdfs[i].type == A.BSDF_RPV) == 1           # one record under both names


@pytest.mark.parametrize("names,first", [(("front", "back"), "back"), (("b", "a"), "a"), (("bsdf_10", "bsdf_2"), "bsdf_2"), (("_arg_1", "_arg_0"), "_arg_0"),
                                         (("a", "b"), "a")])
def test_children_are_taken_in_name_order(names, first):
    """props.objects() is the name order of Properties (twosided.cpp:64-68): {"front": A, "back": B} makes B the side cos_theta(wi) > 0"""
    desc, keep = describe(base(two(DIFFUSE, RPV, names=names)))
    c0, c1 = children_of(desc)
    kinds = (desc.bsdfs[c0].type, desc.bsdfs[c1].type)
    assert kinds == ((A.BSDF_RPV, A.BSDF_DIFFUSE) if first == names[1] else (A.BSDF_DIFFUSE, A.BSDF_RPV))


def test_ref_children_and_shared_children():
    d = base(two({"type": "ref", "id": "mat"}, {"type": "ref", "id": "mat"}))
    d["a_material"] = dict(DIFFUSE, id="mat")
    d["ceiling"]["bsdf"] = {"type": "ref", "id": "mat"}
    desc, keep = describe(d)
    c0, c1 = children_of(desc)
    assert c0 == c1 == desc.shapes[[s for s in range(desc.shape_count) if desc.shapes[s].bsdf == c0][0]].bsdf
    assert sum(1 for i in range(desc.bsdf_count) if np.allclose(list(desc.bsdfs[i].reflectance), [0.2, 0.4, 0.6])) == 1
    # an adapter declared at the scene level and referenced by a shape
    e = base({"type": "ref", "id": "leaf"})
    e["a_leaf"] = dict(two(DIFFUSE, RPV), id="leaf")
    desc, keep = describe(e)
    assert desc.shapes[[s for s in range(desc.shape_count) if desc.bsdfs[desc.shapes[s].bsdf].type == A.BSDF_TWOSIDED][0]].bsdf == index_of(desc)


def test_a_blend_child_and_textured_children():
    tex = bitmap(np.random.default_rng(3).random((4, 4, 3), dtype=np.float32))
    d = base(two(blend(bitmap(np.array([[0.0, 1.0], [0.5, 0.5]], np.float32)), a=DIFFUSE, b=RPV), {"type": "diffuse", "reflectance": tex}))
    desc, keep = describe(d)
    c0, c1 = children_of(desc)
    assert desc.bsdfs[c0].type == A.BSDF_BLEND and desc.bsdfs[c1].type == A.BSDF_DIFFUSE
    assert desc.texture_count == 2 and bsdf_row(desc, index_of(desc)) == [-1] * 6             # the adapter itself reads no texture slot
    assert bsdf_row(desc, c0)[0] >= 0 and bsdf_row(desc, c1)[0] >= 0 and bsdf_row(desc, c0)[0] != bsdf_row(desc, c1)[0]
    assert all(desc_digest(desc))                                                         # and the library takes it


XML_SCENE = """<scene version="2.0.0">
    <bsdf type="rpv" id="veg"><float name="k" value="0.6"/><float name="g" value="-0.2"/><spectrum name="rho_0" value="0.3"/></bsdf>
    <shape type="rectangle">
        <bsdf type="twosided">
            %s
        </bsdf>
    </shape>
    <emitter type="directional"><vector name="direction" x="0" y="0" z="-1"/></emitter>
    <sensor type="perspective"><film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="4"/></film></sensor>
</scene>"""
XML_DIFFUSE = '<bsdf type="diffuse"%s><rgb name="reflectance" value="0.2, 0.4, 0.6"/></bsdf>'


def test_xml_and_dict_give_the_same_description():
    as_dict = {"a": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.2, 0.4, 0.6]}}, "b": {"type": "ref", "id": "veg"}}
    for inner, expected, kinds in (
            (XML_DIFFUSE % "" + '<ref id="veg"/>', as_dict, (A.BSDF_DIFFUSE, A.BSDF_RPV)),                                           # unnamed: _arg_0, _arg_1
            (XML_DIFFUSE % ' name="front"' + '<ref id="veg" name="back"/>', as_dict, (A.BSDF_RPV, A.BSDF_DIFFUSE)),                  # named: "back" < "front"
            (XML_DIFFUSE % "", {"a": as_dict["a"]}, (A.BSDF_DIFFUSE, A.BSDF_DIFFUSE))):                                             # one child
        from_xml = XML.xml_to_dict(XML_SCENE % inner)
        dx, kx = describe(from_xml)
        c0, c1 = children_of(dx)
        assert (dx.bsdfs[c0].type, dx.bsdfs[c1].type) == kinds
        assert (c0 == c1) == (len(expected) == 1)
        if kinds[0] == A.BSDF_DIFFUSE:
            d = copy.deepcopy(from_xml)
            [v for v in d.values() if isinstance(v, dict) and v.get("type") == "rectangle"][0]["bsdf"] = dict({"type": "twosided"}, **copy.deepcopy(expected))
            dd, kd = describe(d)
            assert desc_digest(dx) == desc_digest(dd)


def test_constructor_errors_are_the_reference_s():
    """twosided.cpp:70,73,91, verbatim"""
    assert refusal(base({"type": "twosided"})) == "A nested one-sided material is required!"
    assert refusal(base(two(DIFFUSE, RPV, DIFFUSE))) == "At most two nested BSDFs can be specified!"
    for child in (BILAMBERTIAN, {"type": "null"}, blend(a=DIFFUSE, b=BILAMBERTIAN)):                  # Null is one of BSDFFlags::Transmission's bits
        assert refusal(base(two(child))) == TRANSMISSION
        assert refusal(base(two(DIFFUSE, child))) == TRANSMISSION
        assert refusal(base(two(child, RPV))) == TRANSMISSION


def test_refusals_of_the_loader():
    msg = refusal(base(two(DIFFUSE, two(RPV))))
    assert "\"twosided\" floor.bsdf" in msg and "\"second\"" in msg and "this backend" in msg, msg
    msg = refusal(base(blend(b=two(RPV))))
    assert "\"blendbsdf\" floor.bsdf" in msg and "\"second\"" in msg and "\"twosided\"" in msg and "this backend" in msg, msg
    spectral = scenes.c5_atmosphere_spectral(8, 8, 2, layers=8)
    spectral["ground"]["bsdf"] = two({"type": "diffuse", "reflectance": 0.5})
    msg = refusal(spectral, spectral=True)
    assert "\"twosided\"" in msg and "spectral variant" in msg and "ground.bsdf" in msg, msg
    d = base(two(DIFFUSE, RPV))
    d["integrator"] = {"type": "moment", "nested": d["integrator"]}
    msg = refusal(d)
    assert "\"twosided\"" in msg and "moment" in msg and "floor.bsdf" in msg, msg
    assert "Unknown / unsupported BSDF plugin \"plastic\"" in refusal(base(two({"type": "plastic"})))
    extra = two(DIFFUSE)
    extra["roughness"] = 0.1
    assert "unreferenced property" in refusal(base(extra))


# ---------------------------------------------------------------- the library's side of the ABI
def test_abi_is_unchanged():
    L = A.lib()
    assert A.MTS_ABI_VERSION == L.mts_abi_version() == 12
    for name, cls in A.ABI_STRUCTS.items():
        assert L.mts_abi_sizeof(name.encode()) == C.sizeof(cls), name
    assert C.sizeof(A.Bsdf) == 4 + 6 * 12 + 6 * 4                      # type, six colour triples, six spectrum indices: what it was


def test_refusals_of_the_library():
    def poked(poke, d=None):
        desc, keep = describe(base(two(DIFFUSE, RPV)) if d is None else d)
        poke(desc, index_of(desc))
        return library_refusal(desc)
    msg = poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(0, s.bsdf_count))
    assert msg.startswith("index out of range: bsdf") and "twosided: \"spectrum[0]\" (brdf_0)" in msg, msg
    assert "index out of range" in poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(1, -1))
    msg = poked(lambda s, i: s.bsdfs[i].spectrum.__setitem__(1, i))
    assert msg.startswith("bsdf ") and ": twosided: \"spectrum[1]\" (brdf_1) is the twosided itself" in msg, msg
    # a twosided child of a twosided, and of a blend
    pair = base(two(DIFFUSE, RPV))
    pair["ceiling"]["bsdf"] = two(RPV)
    desc, keep = describe(pair)
    first, second = [i for i in range(desc.bsdf_count) if desc.bsdfs[i].type == A.BSDF_TWOSIDED]
    desc.bsdfs[first].spectrum[1] = second
    msg = library_refusal(desc)
    assert msg.startswith("bsdf %d: twosided:" % first) and "nested twosided adapters are not supported by this backend" in msg, msg
    mixed = base(two(DIFFUSE, RPV))
    mixed["ceiling"]["bsdf"] = blend()
    for ceiling_first in (False, True):                                  # the blend before and behind the adapter it is pointed at
        if ceiling_first:
            mixed["floor"]["bsdf"], mixed["ceiling"]["bsdf"] = mixed["ceiling"]["bsdf"], mixed["floor"]["bsdf"]
        desc, keep = describe(mixed)
        desc.bsdfs[index_of(desc, A.BSDF_BLEND)].spectrum[0] = index_of(desc)
        msg = library_refusal(desc)
        assert "blendbsdf" in msg and "is a twosided" in msg and "not supported by this backend" in msg, msg

    # a transmissive child, decided from the resolved flags: a null, a bilambertian, and a blend that holds one -- the blend
    # standing before and behind the adapter
    def to_kind(kind):
        def poke(s, i):
            s.bsdfs[i].spectrum[1] = [k for k in range(s.bsdf_count) if s.bsdfs[k].type == kind and k != i][0]
        return poke
    for kind, other in ((A.BSDF_NULL, {"type": "null"}), (A.BSDF_BILAMBERTIAN, BILAMBERTIAN)):
        d = base(two(DIFFUSE, RPV))
        d["ceiling"]["bsdf"] = other
        msg = poked(to_kind(kind), d)
        assert msg.startswith("bsdf ") and "twosided: " + TRANSMISSION in msg, msg
    orders = set()
    for swap in (False, True):
        d = base(two(DIFFUSE, RPV))
        d["ceiling"]["bsdf"] = blend(a=DIFFUSE, b=BILAMBERTIAN)
        if swap:
            d["floor"]["bsdf"], d["ceiling"]["bsdf"] = d["ceiling"]["bsdf"], d["floor"]["bsdf"]
        desc, keep = describe(d)
        orders.add(index_of(desc, A.BSDF_BLEND) < index_of(desc))
        assert "twosided: " + TRANSMISSION in poked(to_kind(A.BSDF_BLEND), d)
    assert orders == {False, True}
    msg = poked(lambda s, i: setattr(s.integrator, "spectral", 1))
    assert "twosided is not supported in the spectral variant" in msg and msg.startswith("bsdf "), msg
    msg = poked(lambda s, i: setattr(s.integrator, "moment", 1))
    assert "twosided is not supported inside a moment integrator's scene" in msg, msg
    assert "unknown BSDF type" in poked(lambda s, i: setattr(s.bsdfs[i], "type", 5))
    assert "unknown BSDF type" in poked(lambda s, i: setattr(s.bsdfs[i], "type", 7))


# ---------------------------------------------------------------- host plan
def leafy_c3(front=DIFFUSE, back=RPV):
    d = scenes.c3_heterogeneous(8, 8, 2, res=8)
    d["ground"]["bsdf"] = two(front, back) if back is not None else two(front)
    return d


def test_traits_and_kernel_row():
    """a scene with a twosided and no texture presents no traits (the lean units promise nothing about it) and takes the general
    unit's row, where mts_render runs its TEX instantiation, as for a blend"""
    plain, keep = describe(scenes.c3_heterogeneous(8, 8, 2, res=8))
    assert kernel_row(plain)[0] != 0
    desc, keep = describe(leafy_c3(DIFFUSE, None))
    assert desc.texture_count == 0
    assert kernel_row(desc) == (0, 11024)
    desc, keep = describe(base(two(DIFFUSE, RPV)))
    assert kernel_row(desc) == (0, 1)                                  # `path`: the flat row
    d = leafy_c3()
    d["integrator"]["type"] = "volpathmis"
    desc, keep = describe(d)
    assert kernel_row(desc)[0] == 0


def test_digest_tells_the_children():
    from tests.test_textures import dict_digest
    first = dict_digest(leafy_c3())
    assert first == dict_digest(leafy_c3()) and all(first)
    assert dict_digest(leafy_c3(RPV, DIFFUSE))[0] != first[0]
    assert dict_digest(leafy_c3(DIFFUSE, None))[0] != first[0]


def test_update_plan_freezes_the_children():
    da, ka = describe(leafy_c3())
    i = index_of(da)
    db, kb = describe(leafy_c3())
    rc, msg, traits, kernel = plan(da, db, [(A.OBJ_BSDF, i)])
    assert rc == 0 and (traits, kernel) == (0, 11024), msg
    for c in (0, 1):
        dc, kc = describe(leafy_c3())
        dc.bsdfs[i].spectrum[c] = dc.bsdfs[i].spectrum[1 - c]
        rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, i)])
        assert rc != 0 and "'spectrum[%d] (brdf_%d)'" % (c, c) in msg and "the topology of a scene is frozen" in msg, msg
    dc, kc = describe(leafy_c3())
    dc.bsdfs[i].type = A.BSDF_DIFFUSE
    rc, msg, _, _ = plan(da, dc, [(A.OBJ_BSDF, i)])
    assert rc != 0 and "'type'" in msg
    child = da.bsdfs[i].spectrum[1]                                      # the children update as they do anywhere
    dc, kc = describe(leafy_c3(back=dict(RPV, k=0.8)))
    rc, msg, traits, kernel = plan(da, dc, [(A.OBJ_BSDF, child)])
    assert rc == 0 and kernel == 11024, msg


# ---------------------------------------------------------------- traverse()
def test_parameter_map_keys_and_updates_through_either_name():
    tex = np.random.default_rng(3).random((4, 4, 3), dtype=np.float32)
    d = leafy_c3({"type": "diffuse", "reflectance": bitmap(tex)}, RPV)
    desc, keep = describe(d)
    p = PKG.ParameterMap(desc, keep)
    assert [k for k in p.keys() if k.startswith("ground.bsdf.")] == [
        "ground.bsdf.brdf_0.reflectance.data", "ground.bsdf.brdf_0.reflectance.resolution", "ground.bsdf.brdf_0.reflectance.transform",
        "ground.bsdf.brdf_1.rho_0.value", "ground.bsdf.brdf_1.g.value", "ground.bsdf.brdf_1.k.value"]
    new = np.random.default_rng(4).random((4, 4, 3), dtype=np.float32)
    p["ground.bsdf.brdf_0.reflectance.data"] = new
    p["ground.bsdf.brdf_1.k.value"] = 0.8
    p.update()
    e = copy.deepcopy(d)
    e["ground"]["bsdf"]["first"]["reflectance"]["data"] = new
    e["ground"]["bsdf"]["second"]["k"] = 0.8
    fresh, keep_f = describe(e)                                         # (`keep` owns what a description points to)
    assert desc_digest(desc) == desc_digest(fresh)
    # one child: both names, one record
    one = leafy_c3(DIFFUSE, None)
    desc, keep = describe(one)
    q = PKG.ParameterMap(desc, keep)
    assert [k for k in q.keys() if k.startswith("ground.bsdf.")] == ["ground.bsdf.brdf_0.reflectance.value", "ground.bsdf.brdf_1.reflectance.value"]
    q["ground.bsdf.brdf_1.reflectance.value"] = [0.7, 0.1, 0.3]
    q.update()
    assert np.allclose(q["ground.bsdf.brdf_0.reflectance.value"], [0.7, 0.1, 0.3])
    assert np.allclose(list(desc.bsdfs[children_of(desc)[0]].reflectance), [0.7, 0.1, 0.3])
    fresh, keep_f = describe(leafy_c3(dict(DIFFUSE, reflectance=[0.7, 0.1, 0.3]), None))
    assert desc_digest(desc) == desc_digest(fresh)
    # scenes without an adapter list what they listed
    plain = PKG.ParameterMap(*describe(scenes.c3_heterogeneous(8, 8, 2, res=8)))
    assert [k for k in plain.keys() if k.startswith("ground.bsdf.")] == ["ground.bsdf.reflectance.value"]


# ---------------------------------------------------------------- the independent estimator's panel problem
def load_pin():
    z = np.load(os.path.join(GOLDEN, "indep_pin_surf_twosided_16x16.npz"))
    return z["mean"], z["var"]


def test_problem_is_well_posed():
    d, scene, cam, max_depth, vertices = problems_twosided.box_panel()
    mean, var = load_pin()
    assert mean.shape == (16, 16, 3) and np.all(mean > 0)
    assert surface.remainder_bound(scene, vertices) < 1e-4 * mean.mean()
    assert len(scene.prims) == 6 + 2
    front, back = scene.prims[-2], scene.prims[-1]
    # back to back, 1e-9 apart, the same corners; the camera looks at the front; the dictionary holds ONE rectangle with the adapter
    assert np.allclose(front.n, -back.n) and np.isclose((front.c - back.c) @ front.n, problems_twosided.GAP, rtol=1e-6) and front.area == back.area
    assert (np.array([0, -14, 3.5]) - front.c) @ front.n > 0
    assert max(problems_twosided.FRONT + problems_twosided.BACK) <= 0.8
    assert np.argmax(problems_twosided.FRONT) != np.argmax(problems_twosided.BACK)
    desc, keep = describe(d)
    c0, c1 = children_of(desc)
    assert np.allclose(list(desc.bsdfs[c0].reflectance), problems_twosided.FRONT) and np.allclose(list(desc.bsdfs[c1].reflectance), problems_twosided.BACK)
    # the loader's transform puts the rectangle where the hand-written corners are
    shape = desc.shapes[[s for s in range(desc.shape_count) if desc.shapes[s].bsdf == index_of(desc)][0]]
    m = np.array(list(shape.to_world.matrix), np.float64).reshape(4, 4)
    assert np.allclose(m[:3, 0], front.eu, atol=1e-6) and np.allclose(m[:3, 1], front.ev, atol=1e-6) and np.allclose(m[:3, 3], front.c, atol=1e-6)


def test_fixture_comes_from_the_committed_estimator():
    """A short live run of the estimator agrees with its fixture (same code, other seed, 64 walks per pixel)."""
    mean, var = load_pin()
    _, scene, cam, max_depth, vertices = problems_twosided.box_panel()
    m, v = surface.render(scene, cam, 64, 77, max_depth, vertices)
    for c in range(3):
        se = math.sqrt(v[..., c].sum() + var[..., c].sum()) / m[..., c].size
        assert abs(m[..., c].mean() - mean[..., c].mean()) < 4 * se
        tm, tv = m[..., c].reshape(4, 4, 4, 4).mean((1, 3)), v[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        fm, fv = mean[..., c].reshape(4, 4, 4, 4).mean((1, 3)), var[..., c].reshape(4, 4, 4, 4).sum((1, 3)) / 256
        p, alpha, _ = z_test(tm, tv, fm, fv)
        assert (p > alpha).all()


def test_fixture_rejects_the_exchanged_sides():
    """the pin's power: a short live run of the estimator on the mutated problem -- front and back exchanged -- is rejected"""
    mean, var = load_pin()
    _, scene, cam, max_depth, vertices = problems_twosided.box_panel(exchanged=True)
    m, v = surface.render(scene, cam, 64, 78, max_depth, vertices)
    assert rejected(mean, var, m, v, "estimator, sides exchanged (64 walks per pixel)")


# ---------------------------------------------------------------- host side under ASan / UBSan: a stand-alone program, nothing loaded into Python
def test_host_side_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) or not glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64*"):
        pytest.skip("hipcc or clang's sanitizer runtime not found")
    csrc = os.path.join(ROOT, "eradiate-kernel_amd", "csrc")
    exe = str(tmp_path / "twosided_host_asan")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DMTSAMD_HOST_ONLY",
                           "-Wall", "-Wno-unused-function", "-Wno-unused-result",
                           os.path.join(csrc, "scene_host.cpp"), os.path.join(csrc, "capi.cpp"), os.path.join(ROOT, "tests", "micro", "twosided_host_asan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert "twosided host sanitizer: 21 cases, 0 failed" in r.stdout, report
