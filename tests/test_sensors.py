"""Several sensors per scene, without a GPU: the loader keeps every sensor of a dictionary or an XML file in the order it visits them
(the first is mts_scene_desc.sensor, the others travel on the keepalive object as `extra_sensors`), a one-sensor scene is described
byte for byte as before (digest, sensor record), the ABI stays 12, the kernel choice is that of the (scene, sensor) pair
(mts_debug_sensor_choice against mts_debug_scene_traits / mts_debug_kernel_choice of the single-sensor description), what the library
refuses, and the host side under ASan / UBSan in a stand-alone program (tests/micro/sensors_host_asan.cpp)."""
import copy
import ctypes as C
import glob
import hashlib
import importlib
import json
import os
import subprocess

import pytest

from tests import sensor_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = importlib.import_module("eradiate-kernel_amd._capi")
SD = importlib.import_module("eradiate-kernel_amd.scene_dict")
pkg = importlib.import_module("eradiate-kernel_amd")
xml_io = importlib.import_module("eradiate-kernel_amd.xml_io")
scenes = importlib.import_module("eradiate-kernel_amd.scenes")
T = importlib.import_module("eradiate-kernel_amd.transform").ScalarTransform4f

SAMPLER = {"type": "independent", "sample_count": 2, "seed": 3}


@pytest.fixture(scope="module")
def L():
    importlib.import_module("eradiate-kernel_amd.build").build_backend(verbose=False)
    lib = A.lib()
    lib.mts_debug_scene_traits.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    lib.mts_debug_kernel_choice.argtypes = [C.POINTER(A.SceneDesc), C.POINTER(C.c_int32)]
    return lib


def sensor_keys(d):
    """the keys of a dictionary's sensors, in the order load() visits them"""
    return [k for k, v in SD.sorted_items(d) if isinstance(v, dict) and v.get("type") in SD.SENSOR_PLUGINS]


def with_only(d, key):
    """`d` with sensor `key` alone: the single-sensor scene a multi-sensor render is compared with"""
    drop = set(sensor_keys(d)) - {key}
    return {k: v for k, v in d.items() if k not in drop}


def extras_of(keep):
    return (A.Sensor * max(len(keep.extra_sensors), 1))(*keep.extra_sensors)


def sensor_choice(L, desc, keep, k):
    t, v = C.c_int32(-1), C.c_int32(-1)
    A.check(L.mts_debug_sensor_choice(C.byref(desc), extras_of(keep), len(keep.extra_sensors), k, C.byref(t), C.byref(v)))
    return t.value, v.value


def lone_choice(L, desc):
    t, v = C.c_int32(-1), C.c_int32(-1)
    A.check(L.mts_debug_scene_traits(C.byref(desc), C.byref(t)))
    A.check(L.mts_debug_kernel_choice(C.byref(desc), C.byref(v)))
    return t.value, v.value


# ---------------------------------------------------------------- single-sensor scenes are what they were
# sha256 of bytes(desc.sensor) as the loader built them before it took several sensors (records without pointers)
SENSOR_BYTES = {"perspective_crop_box_ppo": "081ac8fb39d4263cebd7421cd418c742b5e66d06982087c62592768abaeb870a",
                "distant_target_sphere": "82c8c1ad75dc5cb06293d33a4bbaa5114e68eddd0179f71c37ffaf7217477a61",
                "wavefront": "7036befe02364c692214f90c8f209a1829e4d185990306115edc3be2a28ea6af",
                "srf_uniform": "e1592df0c4b1b877978608ccf3f665460d48ba088c3631de2a60d88cf2a3d959"}


@pytest.mark.parametrize("case", sorted(SENSOR_BYTES))
def test_one_sensor_description_is_unchanged(L, case):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_digests_abi12.json")))
    builder, kw = sensor_cases.CASES[case]
    desc, keep = SD.build_scene_desc(builder(), **kw)
    assert keep.extra_sensors == [] and len(keep.sensor_pixel_formats) == 1 and keep.sensor_pixel_formats[0] == keep.film_pixel_format
    assert hashlib.sha256(bytes(desc.sensor)).hexdigest() == SENSOR_BYTES[case]
    out = (C.c_uint64 * 8)()
    A.check(L.mts_debug_desc_digest(C.byref(desc), out))
    assert [str(w) for w in out] == golden[case]
    # ... and sensor 0 of the debug entry without extras is the description's own choice
    assert sensor_choice(L, desc, keep, 0) == lone_choice(L, desc)


def test_abi_is_still_12(L):
    assert A.MTS_ABI_VERSION == 12 and L.mts_abi_version() == 12
    for name, cls in A.ABI_STRUCTS.items():
        assert L.mts_abi_sizeof(name.encode()) == C.sizeof(cls), name
    for name in ("mts_scene_add_sensor", "mts_scene_sensor_count", "mts_render_sensor"):
        assert hasattr(L, name) and name in A.ABI_SYMBOLS


# ---------------------------------------------------------------- four sensors: order, pixel formats, media
def four_sensors():
    """Keys chosen so that the visiting order (Properties' SortKey: alpha, sensor_2, sensor_10, zeta) is neither the insertion order
    nor the plain lexicographic one."""
    d = sensor_cases.scene(dict(sensor_cases.CAMERA, film=sensor_cases.film(6, 4, pixel_format="rgb"), sampler=dict(SAMPLER)),
                           {"type": "volpath", "max_depth": 5, "rr_depth": 3})
    d["zeta"] = d.pop("sensor")
    d["alpha"] = {"type": "distant", "direction": [0.25, 0, 1], "ray_target": dict(sensor_cases.SPHERE), "sampler": dict(SAMPLER),
                  "film": sensor_cases.film(5, 1, pixel_format="luminance")}
    d["sensor_10"] = {"type": "mdistant", "directions": sensor_cases.DIRECTIONS, "target": list(sensor_cases.POINT), "sampler": dict(SAMPLER),
                      "film": sensor_cases.film(3, 1, pixel_format="xyz")}
    d["fog"] = {"type": "homogeneous", "id": "fog", "sigma_t": 0.25, "albedo": 0.5}
    d["sensor_2"] = dict(sensor_cases.CAMERA, film=sensor_cases.film(8, 2), sampler=dict(SAMPLER), medium={"type": "ref", "id": "fog"})
    return d


FOUR_XML = """<scene version="2.0.0">
    <integrator type="volpath" name="integrator"><integer name="max_depth" value="5"/><integer name="rr_depth" value="3"/></integrator>
    <sensor type="perspective" name="zeta">
        <transform name="to_world"><lookat origin="0,-4,3" target="0,0,0" up="0,0,1"/></transform><float name="fov" value="35"/>
        <film type="hdrfilm"><integer name="width" value="6"/><integer name="height" value="4"/><string name="pixel_format" value="rgb"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="2"/><integer name="seed" value="3"/></sampler>
    </sensor>
    <sensor type="distant" name="alpha">
        <vector name="direction" value="0.25, 0, 1"/>
        <shape type="sphere" name="ray_target"><point name="center" value="0, 0.5, 1"/><float name="radius" value="0.75"/></shape>
        <film type="hdrfilm"><integer name="width" value="5"/><integer name="height" value="1"/><string name="pixel_format" value="luminance"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="2"/><integer name="seed" value="3"/></sampler>
    </sensor>
    <sensor type="mdistant" name="sensor_10">
        <string name="directions" value="0, 0, 1, 0.5, 0, 1, 0, -0.5, 1"/><point name="target" value="0.25, -0.5, 0.125"/>
        <film type="hdrfilm"><integer name="width" value="3"/><integer name="height" value="1"/><string name="pixel_format" value="xyz"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="2"/><integer name="seed" value="3"/></sampler>
    </sensor>
    <medium type="homogeneous" id="fog" name="fog"><float name="sigma_t" value="0.25"/><float name="albedo" value="0.5"/></medium>
    <sensor type="perspective" name="sensor_2">
        <transform name="to_world"><lookat origin="0,-4,3" target="0,0,0" up="0,0,1"/></transform><float name="fov" value="35"/>
        <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="2"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="2"/><integer name="seed" value="3"/></sampler>
        <ref id="fog" name="medium"/>
    </sensor>
    <shape type="rectangle" name="ground"><transform name="to_world"><scale value="2"/></transform><bsdf type="diffuse"><float name="reflectance" value="0.5"/></bsdf></shape>
    <emitter type="directional" name="sun"><vector name="direction" value="0.3, 0, -1"/><float name="irradiance" value="1"/></emitter>
</scene>"""


def summary(desc, keep):
    recs = [desc.sensor] + list(keep.extra_sensors)
    return [(r.type, r.film_width, r.film_height, r.sample_count, r.medium, r.multi_count, r.distant_target_type) for r in recs]


@pytest.mark.parametrize("source", ["dict", "xml"])
def test_four_sensors_in_visiting_order(source):
    d = four_sensors() if source == "dict" else xml_io.xml_to_dict(FOUR_XML)
    assert sensor_keys(d) == ["alpha", "sensor_2", "sensor_10", "zeta"] and list(k for k in d if k in sensor_keys(d)) != sensor_keys(d)
    desc, keep = SD.build_scene_desc(d)
    assert len(keep.extra_sensors) == 3
    assert summary(desc, keep) == [(A.SENSOR_DISTANT, 5, 1, 2, -1, 0, A.DISTANT_TARGET_SHAPE), (A.SENSOR_PERSPECTIVE, 8, 2, 2, 0, 0, 0),
                                   (A.SENSOR_MDISTANT, 3, 1, 2, -1, 3, A.DISTANT_TARGET_POINT), (A.SENSOR_PERSPECTIVE, 6, 4, 2, -1, 0, 0)]
    assert keep.sensor_pixel_formats == ["luminance", "rgba", "xyz", "rgb"] and keep.film_pixel_format == "luminance"
    assert desc.medium_count == 1                                   # the medium sensor_2 sits in is the scene's `fog`, present once
    # every record is, byte for byte, the one its single-sensor scene gets (records without pointers; the medium index aside)
    for k, key in enumerate(sensor_keys(d)):
        lone, lone_keep = SD.build_scene_desc(with_only(d, key))
        assert lone_keep.extra_sensors == []
        if key != "sensor_10":
            assert bytes(lone.sensor) == bytes(([desc.sensor] + keep.extra_sensors)[k]), key


def test_dict_and_xml_agree():
    a, ka = SD.build_scene_desc(four_sensors())
    b, kb = SD.build_scene_desc(xml_io.xml_to_dict(FOUR_XML))
    assert summary(a, ka) == summary(b, kb) and ka.sensor_pixel_formats == kb.sensor_pixel_formats


# ---------------------------------------------------------------- the kernel choice is the (scene, sensor) pair's
def cornell_with_a_sphere_target():
    d = scenes.c1_cornell(16, 16, 2)                                # no sphere among its shapes: alone it renders on a lean unit
    d["z_distant"] = {"type": "distant", "direction": [0.25, 0, 1], "ray_target": {"type": "sphere", "center": [0, 0, 3], "radius": 1.0},
                      "film": sensor_cases.film(4, 1), "sampler": dict(SAMPLER)}
    return d, {}


def wavefront_beside_scalar():
    d = scenes.c3_heterogeneous(16, 16, 2, res=8)
    d["a_wavefront"] = dict(copy.deepcopy(d["sensor"]), sampler={"type": "independent", "sample_count": 2, "wavefront": True})
    return d, {}


def srf_beside_none():
    d = sensor_cases.spectral(dict(sensor_cases.VOLPATH))
    d["with_srf"] = dict(sensor_cases.CAMERA, srf=dict(sensor_cases.SRF_DISCRETE), film=sensor_cases.film(4, 4), sampler=dict(SAMPLER))
    return d, {"spectral": True}


CHOICE_SCENES = {"cornell_sphere_target": cornell_with_a_sphere_target, "wavefront_beside_scalar": wavefront_beside_scalar, "srf_beside_none": srf_beside_none}


@pytest.mark.parametrize("name", sorted(CHOICE_SCENES))
def test_choice_is_the_single_sensor_scenes(L, name):
    d, kw = CHOICE_SCENES[name]()
    desc, keep = SD.build_scene_desc(d, **kw)
    keys = sensor_keys(d)
    assert len(keys) == 2 and len(keep.extra_sensors) == 1
    got = [sensor_choice(L, desc, keep, k) for k in range(2)]
    want = [lone_choice(L, SD.build_scene_desc(with_only(d, key), **kw)[0]) for key in keys]
    print(name, keys, got, want)
    assert got == want
    if name != "srf_beside_none":                                    # (without media both spectral perspectives take the nested kernel)
        assert got[0] != got[1]                                      # the two sensors do render on different kernels
    if name == "cornell_sphere_target":
        NO_SPHERE = lone_choice(L, SD.build_scene_desc(scenes.c1_cornell(16, 16, 2))[0])
        (lean, _), (general, _) = got[keys.index("sensor")], got[keys.index("z_distant")]
        assert (lean, got[keys.index("sensor")][1]) == NO_SPHERE and got[keys.index("sensor")][1] >= 100000      # the flat `path` row of a lean unit
        assert got[keys.index("z_distant")][1] < 100000 and lean & ~general != 0                                  # never sensor 0's unit


# ---------------------------------------------------------------- refusals of the library, each with its message
def base_desc(**kw):
    d = sensor_cases.scene(dict(sensor_cases.CAMERA), {"type": "volpath", "max_depth": 5, "rr_depth": 3, "samples_per_pass": 1})
    if kw.get("spectral"):
        d["sensor"]["srf"] = dict(sensor_cases.SRF_UNIFORM)
    return SD.build_scene_desc(d, **kw)


def refusal(L, desc, rec, n=1, sensor=0):
    t, v = C.c_int32(-1), C.c_int32(-1)
    ex = (A.Sensor * 1)(rec) if rec is not None else None
    assert L.mts_debug_sensor_choice(C.byref(desc), ex, n, sensor, C.byref(t), C.byref(v)) != 0
    assert (t.value, v.value) == (-1, -1)
    return L.mts_last_error().decode()


def camera_record(desc):
    rec = A.Sensor.from_buffer_copy(bytes(desc.sensor))
    rec.srf = 0
    return rec


def test_library_refusals(L):
    desc, keep = base_desc()
    assert "sensors missing" in refusal(L, desc, None)
    assert L.mts_scene_add_sensor(None, C.byref(camera_record(desc)), None) != 0 and b"scene is NULL" in L.mts_last_error()
    assert refusal(L, desc, camera_record(desc), sensor=2) == "sensor index 2 is out of range (the scene has 2 sensors)"
    assert "out of range" in refusal(L, desc, camera_record(desc), sensor=-1)
    rec = camera_record(desc); rec.medium = 0                      # the scene has no medium at all
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: index out of range: sensor medium"
    rec = camera_record(desc); rec.type = A.SENSOR_MRADIANCEMETER; rec.multi_count = 2
    mats = (C.c_float * 32)(); rec.multi_transforms = C.cast(mats, C.POINTER(C.c_float))
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: Film size must be [sensor_count, 1]."
    rec = camera_record(desc); rec.sampler_wavefront = 1           # samples_per_pass = 1 < sample_count = 2
    assert refusal(L, desc, rec) == ("mts_scene_add_sensor: wavefront streams (mts_sensor.sampler_wavefront): samples_per_pass must cover "
                                     "the whole sample_count (one pass)")
    rec = camera_record(desc); rec.crop_size[0] = 9
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: film: invalid size / crop window"


def test_library_refusals_of_an_srf(L):
    desc, keep = base_desc(spectral=True)
    assert desc.spectrum_count >= 1 and desc.sensor.srf >= 1
    rec = camera_record(desc); rec.srf = desc.spectrum_count + 1
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: index out of range: sensor srf"
    rec = camera_record(desc); rec.srf = -3
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: index out of range: sensor srf"
    rec = camera_record(desc); rec.srf = desc.sensor.srf; rec.type = A.SENSOR_DISTANT; rec.film_height = rec.crop_size[1] = 1
    assert refusal(L, desc, rec) == "mts_scene_add_sensor: srf: only perspective and radiancemeter sensors sample their wavelengths from a response function"
    rec = camera_record(desc); rec.srf = desc.sensor.srf         # and the same srf on a perspective is taken
    t, v = C.c_int32(), C.c_int32()
    A.check(L.mts_debug_sensor_choice(C.byref(desc), (A.Sensor * 1)(rec), 1, 1, C.byref(t), C.byref(v)))
    assert (t.value, v.value) == lone_choice(L, desc)


def test_a_sensor_of_another_scene_is_refused():
    """Integrator.render() finds the sensor among scene.sensors() before it touches the library: two Scene objects without handles."""
    def handleless(d):
        desc, keep = SD.build_scene_desc(d)
        s = object.__new__(pkg.Scene)
        s._desc, s._keep, s._device, s._handle = desc, keep, 0, None
        s._sensors = [pkg.Sensor(rec, fmt) for rec, fmt in zip([desc.sensor] + keep.extra_sensors, keep.sensor_pixel_formats)]
        s._integrator = pkg.Integrator(s)
        return s
    a, b = handleless(four_sensors()), handleless(four_sensors())
    assert len(a.sensors()) == 4 and [s.film().size() for s in a.sensors()] == [(5, 1), (8, 2), (3, 1), (6, 4)]
    assert [s.film()._pixel_format for s in a.sensors()] == [pkg.PixelFormat.Y, pkg.PixelFormat.RGBA, pkg.PixelFormat.XYZ, pkg.PixelFormat.RGB]
    with pytest.raises(RuntimeError, match="the sensor belongs to another scene"):
        a.integrator().render(a, b.sensors()[1])
    with pytest.raises(RuntimeError, match="sensor index 4 is out of range"):
        a.integrator().render(a, 4)
    with pytest.raises(RuntimeError, match="the integrator belongs to another scene"):
        a.integrator().render(b, b.sensors()[0])


# ---------------------------------------------------------------- host side under ASan / UBSan: a stand-alone program, nothing loaded into Python
def test_host_side_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc) or not glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64*"):
        pytest.skip("hipcc or clang's sanitizer runtime not found")
    csrc = os.path.join(ROOT, "eradiate-kernel_amd", "csrc")
    exe = str(tmp_path / "sensors_host_asan")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-mfma", "-ffp-contract=off", "-fno-fast-math",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DMTSAMD_HOST_ONLY",
                           "-Wall", "-Wno-unused-function", "-Wno-unused-result",
                           os.path.join(csrc, "scene_host.cpp"), os.path.join(csrc, "capi.cpp"), os.path.join(ROOT, "tests", "micro", "sensors_host_asan.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    report = r.stdout[-3000:] + r.stderr[-6000:]
    assert r.returncode == 0, report
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, report
    assert ", 0 failed" in r.stdout, report
