"""load_dict: Mitsuba-style scene dictionaries -> the flattened C-ABI scene description.

Mirrors the conventions of the reference's C++ `load_dict`
(/root/reference/src/libcore/python/xml_v.cpp:100-272): key "type" selects the plugin, "id" names an
instance, nested dicts recurse, {"type": "rgb" | "spectrum", "value": ...} become constant colours in
rgb variants (src/libcore/xml.cpp:1073-1111), {"type": "ref", "id": ...} references an earlier
instance, media attach to shapes under the keys "interior" / "exterior"
(src/librender/shape.cpp:58-68), and a property nobody queried is an error (xml_v.cpp:268-269).
Only the plugins of the path / volpath hot path are known.
"""
import ctypes as C
import math

import numpy as np

from . import _capi as A
from .transform import ScalarTransform4f, coordinate_system, normalize32
from .volume_io import read_volume
from .mesh_io import load_mesh
from .texture_io import read_pfm
from .fresolver import file_resolver


def _key_less(a, b):
    """Properties' SortKey (src/libcore/properties.cpp:41-63): lexicographic with numeric suffixes compared
    as numbers, so children named shape_2, shape_10 keep their numeric order."""
    i = 0
    while i < len(a) and i < len(b) and a[i] == b[i]:
        i += 1
    while i > 0 and a[i - 1].isdigit():
        i -= 1
    ta, tb = a[i:], b[i:]
    if ta[:1].isdigit() and tb[:1].isdigit() and ta.isdigit() and tb.isdigit():
        return int(ta) < int(tb)
    return ta < tb


def sorted_items(d):
    """Children in the order Properties::objects() yields them (std::map ordered by SortKey)."""
    import functools
    keys = sorted(d.keys(), key=functools.cmp_to_key(lambda a, b: -1 if _key_less(a, b) else (1 if _key_less(b, a) else 0)))
    return [(k, d[k]) for k in keys]


class Props:
    """Properties bag with 'queried' tracking (src/libcore/properties.cpp)."""

    def __init__(self, d, where):
        if not isinstance(d, dict) or "type" not in d:
            raise RuntimeError("Missing key 'type' in dictionary: %s" % where)
        self.d = d
        self.type = d["type"]
        self.where = where
        self.queried = {"type", "id"}

    def has(self, k):
        return k in self.d

    def get(self, k, default=None):
        self.queried.add(k)
        return self.d.get(k, default)

    def finish(self):
        left = [k for k in self.d if k not in self.queried]
        if left:
            raise RuntimeError("Error while loading \"%s\": unreferenced propert%s %s in plugin of type \"%s\""
                               % (self.where, "ies" if len(left) > 1 else "y", left, self.type))


def _xf(t):
    r = A.Transform()
    if t is None:
        t = ScalarTransform4f()
    if not isinstance(t, ScalarTransform4f):
        t = ScalarTransform4f(np.asarray(t, dtype=np.float32))
    r.matrix[:] = t.matrix.reshape(-1).tolist()
    r.inverse_transpose[:] = t.inverse_transpose.reshape(-1).tolist()
    return r


WAVELENGTH_MIN, WAVELENGTH_MAX = 280.0, 2400.0       # MTS_WAVELENGTH_MIN / MAX, include/mitsuba/core/spectrum.h:15-21


def spectrum_from_file(filename):
    """src/libcore/spectrum.cpp:9-39: `wavelength value` per line, empty lines and lines starting with '#' skipped, anything after the
    pair is an error; the name goes through the FileResolver."""
    import os
    path = file_resolver().resolve(filename)
    if not os.path.exists(path):
        raise RuntimeError("\"%s\": file does not exist!" % path)
    pairs = []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if len(line) == 0 or line[0] == "#":
                continue
            tok = line.split()
            if len(tok) > 2:
                raise RuntimeError("\"%s\": excess tokens after wavlengths-value pair in file:\n%s!" % (path, line))
            if len(tok) < 2:                                 # `iss >> value` fails: the reference keeps whatever the variables held; not reproduced
                raise RuntimeError("\"%s\": could not parse wavelength-value pair:\n%s" % (path, line))
            pairs.append((float(np.float32(tok[0])), float(np.float32(tok[1]))))
    return pairs


def _spectrum_pairs(v, where):
    """The wavelength:value pairs of a {"type": "spectrum"} dictionary (inline string / list, or a file), or None for a constant."""
    if "filename" in v:
        if "value" in v:
            raise RuntimeError("'spectrum' tag requires one of \"value\" or \"filename\" attributes")      # xml.cpp:815-816
        return spectrum_from_file(v["filename"])
    val = v.get("value", 1.0)
    if isinstance(val, str) and ":" in val:                                 # "400:0.1, 500:0.2, ..." (xml.cpp:823-846)
        try:
            return [tuple(float(x) for x in tok.split(":")) for tok in val.replace(",", " ").split()]
        except ValueError:
            raise RuntimeError("Could not parse wavelength:value pairs in %s" % where)
    if isinstance(val, (list, tuple, np.ndarray)):
        return [tuple(x) for x in np.asarray(val, np.float64).reshape(-1, 2)]
    return None


def _cie1931_xyz(x):
    """core/spectrum.h:148-178 in float32: linear interpolation of the 5 nm tables over 360 .. 830 nm, zero outside."""
    from .spectra_data import CIE_1931
    f = np.float32
    t = f(f(f(x) - f(360.0)) * f(f(94) / f(f(830.0) - f(360.0))))
    if not (x >= 360.0 and x <= 830.0):
        return np.zeros(3, np.float32)
    i0 = int(min(max(int(t), 0), 93)); i1 = i0 + 1
    w1 = f(t - f(i0)); w0 = f(f(1.0) - w1)
    return np.array([f(f(w0 * f(CIE_1931[c][i0])) + f(w1 * f(CIE_1931[c][i1]))) for c in range(3)], np.float32)       # fmadd(w0, v0, w1 * v1): differs in the last bit at most


def spectrum_to_rgb(wavelengths, values, bounded=True):
    """src/libcore/spectrum.cpp:41-89: pre-integration of a tabulated spectrum against the CIE 1931 curves (1000 steps over
    MTS_WAVELENGTH_MIN .. MAX = 280 .. 2400 nm, this fork's range), XYZ -> linear sRGB, clamped (to [0, 1] when `bounded`)."""
    f = np.float32
    wl = [f(w) for w in wavelengths]; vs = [f(v) for v in values]
    color = np.zeros(3, np.float32)
    steps = 1000
    for i in range(steps):
        x = f(f(WAVELENGTH_MIN) + f(f(i) / f(steps - 1)) * f(f(WAVELENGTH_MAX) - f(WAVELENGTH_MIN)))
        if x < wl[0] or x > wl[-1]:
            continue
        # math::find_interval(size, pred): the last index with pred true, clamped to [0, size - 2]
        index = 0
        for k in range(len(wl)):
            if wl[k] <= x:
                index = k
        index = min(max(index, 0), len(wl) - 2)
        x0, x1, y0, y1 = wl[index], wl[index + 1], vs[index], vs[index + 1]
        y = f(f(f(f(f(x * y0) - f(x1 * y0)) - f(x * y1)) + f(x0 * y1)) / f(x0 - x1))
        color = (color + _cie1931_xyz(x) * y).astype(np.float32)
    color = (color * f(f(f(WAVELENGTH_MAX) - f(WAVELENGTH_MIN)) / f(steps))).astype(np.float32)
    m = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], np.float32)   # xyz_to_srgb, spectrum.h:229-235
    color = (m @ color).astype(np.float32)
    color = np.clip(color, 0.0, 1.0) if bounded else np.maximum(color, 0.0)
    return tuple(float(c) for c in color)


CIE_Y_NORMALIZATION = 1.0 / 106.856895                     # MTS_CIE_Y_NORMALIZATION, core/spectrum.h:136
_UNBOUNDED_NAMES = ("eta", "k", "int_ior", "ext_ior")      # is_unbounded_spectrum, xml.cpp:142-144


def _luminance(c):
    """spectrum.h:246-248 over the last axis of an array of linear rgb, in float32: (r * 0.212671 + g * 0.715160) + b * 0.072169, every
    product and sum rounded to float32 -- one colour, the voxels of a grid or the texels of a bitmap under the *_mono variants."""
    f = np.float32
    c = np.asarray(c, dtype=np.float32)
    return (c[..., 0] * f(0.212671) + c[..., 1] * f(0.715160)) + c[..., 2] * f(0.072169)


def _color_rgb(v, where, default=None, emitter=False):
    if v is None:
        v = default
    if isinstance(v, dict):
        t = v.get("type")
        if t == "rgb":
            if len(v) != 2:
                raise RuntimeError("'rgb' dictionary should always contain 2 entries ('type' and 'value'), got %d." % len(v))
            c = np.asarray(v["value"], dtype=np.float32).reshape(-1)
            if c.size == 1:
                c = np.repeat(c, 3)
            return tuple(float(x) for x in c[:3])
        if t == "spectrum":
            pairs = _spectrum_pairs(v, where)
            if pairs is not None:
                # create_texture_from_spectrum in the non-spectral modes (xml.cpp:1113-1170): values x MTS_CIE_Y_NORMALIZATION, wavelengths
                # in increasing order, pre-integrated against the CIE curves -> `srgb` (bounded) / `srgb_d65` (emitters) colour
                f = np.float32
                wl = [p_[0] for p_ in pairs]
                if any(b_ - a_ < 0 for a_, b_ in zip(wl, wl[1:])):
                    raise RuntimeError("Wavelengths must be specified in increasing order!")
                if len(wl) < 2:
                    raise RuntimeError("a tabulated spectrum needs at least two wavelength:value pairs: %s" % where)
                name = where.rsplit(".", 1)[-1]
                return spectrum_to_rgb(wl, [f(f(p_[1]) * f(CIE_Y_NORMALIZATION)) for p_ in pairs], bounded=not (emitter or name in _UNBOUNDED_NAMES))
            return (float(v.get("value", 1.0)),) * 3
        if t == "uniform":
            val = v.get("value", 1.0)
            if isinstance(val, (list, tuple, str)):
                raise RuntimeError("'uniform' takes one value: %s" % where)
            return (float(val),) * 3
        if t in ("srgb", "srgb_d65"):
            c = np.asarray(v.get("color"), dtype=np.float32).reshape(-1)
            return tuple(float(x) for x in c[:3])
        if t in TEXTURE_PLUGINS:                                # textures are taken where a BSDF's colour parameter is (SceneBuilder.add_bsdf)
            if emitter:
                raise RuntimeError("Textures on emitters are not supported by this backend (\"%s\" in %s): give a constant" % (t, where))
            raise RuntimeError("A \"%s\" texture is not accepted in %s: textures are supported for the colour parameters of BSDFs only" % (t, where))
        raise RuntimeError("Unsupported texture / spectrum plugin \"%s\" in %s (rgb constants only)" % (t, where))
    c = np.asarray(v, dtype=np.float32).reshape(-1)
    if c.size == 1:
        return (float(c[0]),) * 3
    if c.size == 3:
        return tuple(float(x) for x in c)
    raise RuntimeError("Cannot interpret %r as a colour in %s" % (v, where))


# BSDFFlags (bsdf.h:38-124) that the twosided adapter's constructor reads; Transmission holds Null
_F_FRONT, _F_BACK, _F_TRANSMISSION = 0x8000, 0x10000, 0x4 | 0x10 | 0x40 | 0x100 | 0x1
_F_DELTA_REFLECTION, _F_DELTA_TRANSMISSION, _F_NON_SYMMETRIC = 0x20, 0x40, 0x4000

BSDF_PLUGINS = ("diffuse", "null", "rpv", "bilambertian", "blendbsdf", "twosided", "dielectric", "conductor")

# Indices of refraction by material name, at about 589 nm and standard conditions (the names a `dielectric` accepts for "int_ior" /
# "ext_ior"; the list order is the order the error message names them in)
IOR_TABLE = (
    ("vacuum", 1.0), ("helium", 1.000036), ("hydrogen", 1.000132), ("air", 1.000277), ("carbon dioxide", 1.00045),
    ("water", 1.3330), ("acetone", 1.36), ("ethanol", 1.361), ("carbon tetrachloride", 1.461), ("glycerol", 1.4729),
    ("benzene", 1.501), ("silicone oil", 1.52045), ("bromine", 1.661),
    ("water ice", 1.31), ("fused quartz", 1.458), ("pyrex", 1.470), ("acrylic glass", 1.49), ("polypropylene", 1.49),
    ("bk7", 1.5046), ("sodium chloride", 1.544), ("amber", 1.55), ("pet", 1.5750), ("diamond", 2.419))


def lookup_ior(v, default):
    """An index of refraction given as a number or as a material name, lower-cased before the lookup (ior.h:52-84) -> np.float32."""
    if v is None:
        v = default
    if isinstance(v, bool) or isinstance(v, dict):
        raise RuntimeError("An index of refraction is a float or a material name, got %r" % (v,))
    if isinstance(v, (int, float, np.floating, np.integer)):
        return np.float32(v)
    name = str(v).lower()
    for key, value in IOR_TABLE:
        if key == name:
            return np.float32(value)
    raise RuntimeError("Unable to find an IOR value for \"%s\"! Valid choices are:%s" % (name, ", ".join(k for k, _ in IOR_TABLE)))


def _weight(v, where):
    """The constant "weight" of a blendbsdf: what Texture::eval_1 gives (blendbsdf.cpp:162-164).  A float or a `uniform` spectrum is its
    value (uniform.cpp:71-75).  An rgb colour or a tabulated spectrum becomes an `srgb` texture in the rgb / mono variants (xml.cpp:1073-1170),
    and src/spectra/srgb.cpp does not override eval_1: the reference throws there, so it is refused here."""
    undefined = "eval_1 is not defined for an rgb colour (src/spectra/srgb.cpp implements eval only): give a float or a uniform spectrum"
    if isinstance(v, dict):
        t = v.get("type")
        if t == "uniform" or (t == "spectrum" and _spectrum_pairs(v, where) is None):
            val = v.get("value", 1.0)
            if isinstance(val, (list, tuple, np.ndarray)):
                raise RuntimeError("\"weight\" in %s takes one value" % where)
            return float(val)
        if t in ("rgb", "srgb", "srgb_d65", "spectrum"):
            raise RuntimeError("\"weight\" in %s: %s" % (where, undefined))
        raise RuntimeError("Unsupported texture / spectrum plugin \"%s\" in %s" % (t, where))
    c = np.asarray(v, dtype=np.float32).reshape(-1)
    if c.size != 1:
        raise RuntimeError("\"weight\" in %s: %s" % (where, undefined))
    return float(c[0])


def _check_weight_texture(d, rec, where):
    """A checkerboard under a blendbsdf's "weight" is read through eval_1 of its two colours (checkerboard.cpp:67-86): they must be
    floats or uniform spectra, as a constant weight (_weight).  A bitmap has eval_1 for one and three channels (bitmap.cpp:285-302)."""
    if rec.type != A.TEXTURE_CHECKERBOARD:
        return
    for key in ("color0", "color1"):
        if isinstance(d, dict) and d.get("type") == "checkerboard":
            if key in d:
                _weight(d[key], where + "." + key)
        elif not (getattr(rec, key)[0] == getattr(rec, key)[1] == getattr(rec, key)[2]):
            raise RuntimeError("\"weight\" in %s: eval_1 is not defined for the rgb colour \"%s\" of the referenced checkerboard" % (where, key))


def parse_fov(p, aspect):
    """src/librender/sensor.cpp:113-167."""
    if p.has("fov") and p.has("focal_length"):
        raise RuntimeError("Please specify either a focal length ('focal_length') or a field of view ('fov')!")
    if p.has("fov"):
        fov = float(p.get("fov"))
        axis = str(p.get("fov_axis", "x")).lower()
        if axis == "smaller":
            axis = "y" if aspect > 1 else "x"
        elif axis == "larger":
            axis = "x" if aspect > 1 else "y"
    else:
        f = str(p.get("focal_length", "50mm"))
        if f.endswith("mm"):
            f = f[:-2]
        value = float(f)
        fov = 2.0 * math.degrees(math.atan(math.sqrt(36 * 36 + 24 * 24) / (2.0 * value)))
        axis = "diagonal"
    if axis == "x":
        result = fov
    elif axis == "y":
        result = math.degrees(2.0 * math.atan(math.tan(0.5 * math.radians(fov)) * aspect))
    elif axis == "diagonal":
        diagonal = 2.0 * math.tan(0.5 * math.radians(fov))
        width = diagonal / math.sqrt(1.0 + 1.0 / (aspect * aspect))
        result = math.degrees(2.0 * math.atan(width * 0.5))
    else:
        raise RuntimeError("The 'fov_axis' parameter must be set to one of 'smaller', 'larger', 'diagonal', 'x', or 'y'!")
    if result <= 0.0 or result >= 180.0:
        raise RuntimeError("The horizontal field of view must be in the range [0, 180]!")
    return float(np.float32(result))


TEXTURE_PLUGINS = ("bitmap", "checkerboard")


def _to_uv(t):
    """props.transform("to_uv").extract() (bitmap.cpp:93, checkerboard.cpp:43; transform.h:327-348) as nine floats, row-major.
    enoki's coeff(i, j) is column i, row j: the loop copies the upper-left 2x2 and, as `coeff(2, i) = coeff(3, i)`, the first two
    entries of the 4x4's last COLUMN -- the x and y of a translation survive, its z is dropped; the 3x3's last row keeps the identity's
    zeros and takes the 4x4's corner.  transform_affine (transform.h:91-98) then never reads that row."""
    if t is None:
        t = ScalarTransform4f()
    if not isinstance(t, ScalarTransform4f):
        t = ScalarTransform4f(np.asarray(t, dtype=np.float32))
    m = np.asarray(t.matrix, np.float32).reshape(4, 4)
    return [float(x) for x in (m[0, 0], m[0, 1], m[0, 3], m[1, 0], m[1, 1], m[1, 3], 0.0, 0.0, m[3, 3])]


def _tab_values(vals):
    """tabphase "values": a string of numbers (tabphase.cpp:33-40) -> float32 array."""
    if not isinstance(vals, str):
        raise RuntimeError("'values' must be a string")
    return np.array([float(s) for s in vals.replace(",", " ").split()], dtype=np.float32)


SHAPE_PLUGINS = ("rectangle", "cube", "sphere", "mesh", "obj", "ply", "disk", "cone")


def _check_cone_transform(m, where):
    """What the library refuses of a cone's to_world (scene_host.cpp: build_shape), said where the cone is declared: the linear part must
    be R * diag(r, r, l) with R a rotation.  The reference (cone.cpp:87-104) only warns and goes on with a record that describes no cone."""
    c0, c1, c2 = (m[:3, k].astype(np.float64) for k in range(3))
    r0, r1, l = (float(np.linalg.norm(c)) for c in (c0, c1, c2))
    if not (r0 > 0 and r1 > 0 and l > 0):
        raise RuntimeError("cone \"%s\": 'to_world' must scale the x / y axes by a radius > 0 and the z axis by a length > 0" % where)
    if abs(c0 @ c1) > 1e-6 * r0 * r0 or abs(c0 @ c2) > 1e-6 * r0 * l or abs(c1 @ c2) > 1e-6 * r0 * l:
        raise RuntimeError("cone \"%s\": 'to_world' transform shouldn't contain any shearing! (refused by this backend: the axes of the cone must stay orthogonal)" % where)
    if abs(r0 - r1) > 1e-6 * r0:
        raise RuntimeError("cone \"%s\": 'to_world' transform shouldn't contain non-uniform scaling along the X and Y axes! (refused by this backend)" % where)
    if np.cross(c0, c1) @ c2 < 0:
        raise RuntimeError("cone \"%s\": 'to_world' transform shouldn't mirror the cone (negative determinant; refused by this backend)" % where)
SAMPLING_INTEGRATORS = {"path": A.INTEGRATOR_PATH, "volpath": A.INTEGRATOR_VOLPATH, "volpathmis": A.INTEGRATOR_VOLPATHMIS}


class SceneBuilder:
    """Accumulates plugin records; keeps every numpy buffer alive for the lifetime of the description."""

    def __init__(self, mono=False, spectral=False):
        """mono: the scene is built with the semantics of the *_mono variants (colours become their luminance, src/spectra/srgb.cpp);
        spectral: with those of scalar_spectral (colours become spectrum records, collected in `spectra`).  Fixed for the builder's life."""
        self.mono, self.spectral = bool(mono), bool(spectral)
        self.volumes, self.phases, self.media, self.bsdfs, self.shapes, self.emitters = [], [], [], [], [], []
        # the sensors in the order load() visits them: `sensor` is the first (mts_scene_desc.sensor, sensor 0), `extra_sensors` the others
        # (Scene hands them to mts_scene_add_sensor in this order); sensor_pixel_formats: each one's film "pixel_format", in that order
        self.sensor = None
        self.extra_sensors, self.sensor_pixel_formats = [], []
        self.sensor_dict = None
        self.integrator = None
        self.keep = []
        self.instances = {}      # id -> (kind, index)
        self.info = {}
        self.spectra, self.spectrum_plugins = [], []
        # traverse() (params.py): what each record exposes, written down while it is built.  nodes[(kind, index)] lists, in the order of
        # the reference plugin's traverse(), ("param", name, what, field) and ("object", name, node) entries; a colour is a node of its
        # own (`srgb` / `uniform` texture): ("colour", kind, index, field, where, emitter) in rgb / mono, ("spectrum", index) in spectral.
        # ("alias", name, node): a one-child twosided's brdf_1, the node listed under brdf_0 just before -- its keys again, under this name
        self.nodes = {}
        self.children = []       # the scene's own children: (key, node)
        self.grids, self.grid_mono_max, self.tabs = {}, {}, {}
        self.spectrum_arrays = {}    # (spectrum, field) -> the array an update put there (one live array per record; load's own are in `keep`)
        # textures behind BSDF colour parameters (rgb / mono): the records, six indices per BSDF (-1: the constant), each bitmap's
        # live (height, width, channels) array
        self.textures, self.bsdf_textures, self.bitmaps = [], [], {}
        self.blends = []         # where each blendbsdf sits (what a refusal of the whole scene names)
        self.twosided = []       # and each twosided
        self.specular = []       # and each dielectric / conductor
        self.groups, self.instanced = [], []     # where each shapegroup / instance sits
        self.cones = []          # and each cone

    def _colour_node(self, kind, index, field, where, spectrum=-1, emitter=False):
        return ("spectrum", spectrum) if self.spectral else ("colour", kind, index, field, where, emitter)

    # ------------------------------------------------------------ conversions that depend on the variant (load and ParameterMap.update)
    def _color(self, v, where, default=None, emitter=False):
        """float | [r,g,b] | {"type":"rgb","value":..} | {"type":"spectrum"/"uniform","value":x} -> (r,g,b)."""
        c = _color_rgb(v, where, default, emitter)
        if self.mono and not (c[0] == c[1] == c[2]):
            return (float(_luminance(c)),) * 3
        return c

    def _spectrum(self, v, where, default=None, emitter=False):
        """Spectral variant: a colour parameter -> index of its spectrum record (mts_spectrum).
        float -> `uniform` (Properties::texture, properties.h:275-296); {"type": "uniform" | "regular" | "d65"} -> the plugin of that
        name (src/spectra/*.cpp; d65 expands to regular, d65.cpp:52-71); {"type": "spectrum", "value": c} -> uniform, or d65 scaled by c
        inside an emitter (create_texture_from_spectrum, xml.cpp:1087-1111); a missing emitter spectrum is D65 (directional.cpp:49,
        area.cpp:39, constant.cpp:33, point.cpp:47).  rgb colours need the sRGB upsampling model, whose data (ext/rgb2spec) is absent."""
        if v is None:
            v = {"type": "d65"} if (emitter and default is None) else default
        rec = A.Spectrum()
        rec.lambda_min, rec.lambda_max = WAVELENGTH_MIN, WAVELENGTH_MAX
        if isinstance(v, dict):
            p = Props(v, where)
            t = p.type
            if t == "spectrum":
                val = _spectrum_pairs(v, where)                                 # inline pairs or spectrum_from_file (xml.cpp:823-851)
                if p.has("filename"):
                    p.get("filename")
                if val is None:
                    val = p.get("value", 1.0)
                elif p.has("value"):
                    p.get("value")
                if isinstance(val, (list, tuple)):
                    # create_texture_from_spectrum, xml.cpp:1113-1150 (spectral mode): values scaled by MTS_CIE_Y_NORMALIZATION inside an
                    # emitter; `regular` when the wavelengths are equidistant (to math::Epsilon), `irregular` otherwise
                    pairs = np.asarray(val, np.float64).reshape(-1, 2)
                    f = np.float32
                    wl = pairs[:, 0].astype(np.float32)
                    vals = (pairs[:, 1].astype(np.float32) * (f(1.0 / 106.7502593994140625) if emitter else f(1.0))).astype(np.float32)
                    dist = np.diff(wl)
                    if (dist < 0).any():
                        raise RuntimeError("Wavelengths must be specified in increasing order!")
                    p.finish()
                    if wl.size >= 2 and (np.abs(dist - dist[0]) <= 2.0 ** -24).all():
                        return self._spectrum({"type": "regular", "lambda_min": float(wl[0]), "lambda_max": float(wl[-1]), "values": vals}, where)
                    return self._spectrum({"type": "irregular", "wavelengths": wl, "values": vals}, where)
                p.finish()
                return self._spectrum({"type": "d65", "scale": float(val)} if emitter else {"type": "uniform", "value": float(val)}, where)
            if t == "uniform":
                rec.type = A.SPECTRUM_UNIFORM
                rec.value = float(p.get("value", 1.0))
                if p.has("lambda_min"):
                    rec.lambda_min = max(float(p.get("lambda_min")), WAVELENGTH_MIN)
                if p.has("lambda_max"):
                    rec.lambda_max = min(float(p.get("lambda_max")), WAVELENGTH_MAX)
                if not rec.lambda_min < rec.lambda_max:
                    raise RuntimeError("UniformSpectrum: 'lambda_min' must be less than 'lambda_max'")
            elif t in ("regular", "d65"):
                rec.type = A.SPECTRUM_REGULAR
                if t == "d65":
                    from .spectra_data import D65, D65_NORMALIZATION
                    f = np.float32
                    scale = f(f(p.get("scale", 1.0)) * f(D65_NORMALIZATION))                  # d65.cpp:56-57: m_scale *= 1.f / 10568.f
                    values = (np.asarray(D65, np.float32) * scale).astype(np.float32)         # :64-65
                    rec.lambda_min, rec.lambda_max = 360.0, 830.0
                else:
                    if not (p.has("lambda_min") and p.has("lambda_max")):
                        raise RuntimeError("Property \"lambda_min\" has not been specified!" if not p.has("lambda_min") else "Property \"lambda_max\" has not been specified!")
                    rec.lambda_min, rec.lambda_max = float(p.get("lambda_min")), float(p.get("lambda_max"))
                    vals = p.get("values")
                    if isinstance(vals, str):
                        vals = [float(x) for x in vals.replace(",", " ").split()]
                    values = np.asarray(vals, np.float32).reshape(-1)
                values = np.ascontiguousarray(values, np.float32)
                self.keep.append(values)
                rec.values = values.ctypes.data_as(A.fp)
                rec.count = int(values.size)
            elif t in ("irregular", "discrete"):
                # spectra/irregular.cpp:33-63 (strings of comma-separated numbers, or arrays), spectra/discrete.cpp:45-100
                def numbers(key, default=None):
                    x = p.get(key, default)
                    if x is None:
                        raise RuntimeError("Property \"%s\" has not been specified!" % key)
                    if isinstance(x, str):
                        try:
                            x = [float(tok) for tok in x.replace(",", " ").split()]
                        except ValueError as e:
                            raise RuntimeError("Could not parse floating point value '%s'" % str(e).split("'")[-2])
                    return np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1), np.float32)
                wl = numbers("wavelengths")
                if t == "irregular":
                    rec.type = A.SPECTRUM_IRREGULAR
                    values = numbers("values")
                    if values.size != wl.size:
                        raise RuntimeError("IrregularSpectrum: 'wavelengths' and 'values' parameters must have the same size!")
                    pmf = None
                else:
                    rec.type = A.SPECTRUM_DISCRETE
                    values, pmf = numbers("values", "1"), numbers("pmf", "1")
                    if values.size == 1:
                        values = np.full(wl.size, values[0], np.float32)
                    if pmf.size == 1:
                        pmf = np.full(wl.size, pmf[0], np.float32)
                    if values.size != wl.size:
                        raise RuntimeError("DiscreteSpectrum: 'wavelengths' and 'values' parameters must have the same size!")
                    if pmf.size != wl.size:
                        raise RuntimeError("DiscreteSpectrum: 'wavelengths' and 'pmf' parameters must have the same size!")
                    self.keep.append(pmf)
                    rec.pmf = pmf.ctypes.data_as(A.fp)
                self.keep.append(wl); self.keep.append(values)
                rec.wavelengths = wl.ctypes.data_as(A.fp)
                rec.values = values.ctypes.data_as(A.fp)
                rec.count = int(wl.size)
            elif t in ("rgb", "srgb", "srgb_d65"):
                raise RuntimeError("rgb colours cannot be used in the spectral variant: the sRGB upsampling model needs the coefficient data of "
                                   "ext/rgb2spec, absent here; give a 'uniform' or 'regular' spectrum instead (%s)" % where)
            else:
                raise RuntimeError("Unsupported spectrum plugin \"%s\" in %s" % (t, where))
            p.finish()
        else:
            c = np.asarray(v, dtype=np.float32).reshape(-1)
            if c.size != 1:
                raise RuntimeError("Cannot interpret %r as a spectrum in %s (spectral variant)" % (v, where))
            rec.type = A.SPECTRUM_UNIFORM
            rec.value = float(c[0])
        self.spectra.append(rec)
        self.spectrum_plugins.append(v.get("type") if isinstance(v, dict) else "uniform")      # traverse(): the keys of that plugin
        return len(self.spectra) - 1

    def _grid_data(self, data):
        """A grid's values as the description holds them: float32, C order, (nz, ny, nx, channels).  Returns (array, mono_max): under the
        *_mono variants a colour grid becomes its luminance per voxel and keeps the file's maximum as its majorant (grid3d.cpp:157-179)."""
        data = np.asarray(data, dtype=np.float32)
        if data.ndim == 3:
            data = data[..., None]
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim != 4:
            raise RuntimeError("gridvolume: data must have shape (nz, ny, nx, channels)")
        mono_max = None
        if self.mono and data.shape[3] == 3:
            # grid3d.cpp:178-179: *_mono variants return the luminance of the interpolated colour. Luminance is
            # linear, so it is applied per voxel here; the majorant stays the file's maximum (volume metadata).
            mono_max = float(data.max()) if data.size else 0.0
            data = np.ascontiguousarray(_luminance(data)[..., None], dtype=np.float32)
        return data, mono_max

    def _bitmap_data(self, data):
        """A bitmap's texels as the description holds them: float32, C order, (height, width, channels), channels 1 or 3.  Under the
        *_mono variants rgb texels become their luminance (bitmap.cpp:278-279; luminance is linear, so it commutes with the filter)."""
        data = np.asarray(data, dtype=np.float32)
        if data.ndim == 2:
            data = data[..., None]
        if data.ndim != 3:
            raise RuntimeError("bitmap: data must have shape (height, width) or (height, width, channels)")
        if data.shape[2] not in (1, 3):
            raise RuntimeError("Unsupported channel count: %d (expected 1 or 3)" % data.shape[2])                  # bitmap.cpp:196
        if data.shape[0] < 2 or data.shape[1] < 2:
            # bitmap.cpp:155-161 up-samples such an image with a tent filter, which this backend has not got
            raise RuntimeError("bitmap: Image must be at least 2x2 pixels in size (got %dx%d; this backend does not up-sample)" % (data.shape[1], data.shape[0]))
        if np.isnan(data).any():
            raise RuntimeError("bitmap: data contains NaN")
        if self.mono and data.shape[2] == 3:
            data = _luminance(data)[..., None]
        return np.ascontiguousarray(data, dtype=np.float32)

    def _emitter_colour(self, e, v, where):
        e.radiance_spectrum = -1
        if self.spectral:
            e.radiance_spectrum = self._spectrum(v, where, emitter=True)
        else:
            e.radiance[:] = self._color(v, where, default=1.0, emitter=True)

    # ------------------------------------------------------------ helpers
    def _register(self, d, kind, index):
        if isinstance(d, dict) and "id" in d:
            self.instances[d["id"]] = (kind, index)

    def _resolve_ref(self, d, kind):
        if isinstance(d, dict) and d.get("type") == "ref":
            for k in d:
                if k not in ("type", "id"):
                    raise RuntimeError("Unexpected key in ref dictionary: %s" % k)
            rid = d.get("id")
            if rid not in self.instances:
                raise RuntimeError("Referenced id \"%s\" not found" % rid)
            k, i = self.instances[rid]
            if k != kind:
                raise RuntimeError("Referenced id \"%s\" is a %s, expected a %s" % (rid, k, kind))
            return i
        return None

    # ------------------------------------------------------------ volumes
    def add_volume(self, v, where, default=None):
        r = self._resolve_ref(v, "volume")
        if r is not None:
            return r
        rec = A.Volume()
        rec.to_world = _xf(None)
        rec.filter_type = A.FILTER_TRILINEAR
        rec.wrap_mode = A.WRAP_CLAMP
        if v is None:
            v = default
        rec.value_spectrum = -1
        if isinstance(v, dict) and v.get("type") in ("gridvolume", "constvolume", "gridvolume_spectral"):
            p = Props(v, where)
            rec.to_world = _xf(p.get("to_world"))
            if p.type == "constvolume":
                rec.type = A.VOLUME_CONST
                # constant3d.cpp: "color" texture; load_dict users pass "value" (xml.cpp spectrum shorthand)
                val = p.get("value", p.get("color", 1.0))
                if self.spectral:
                    rec.value_spectrum = self._spectrum(val, where)
                else:
                    rec.value[:] = self._color(val, where)
            else:
                rec.type = A.VOLUME_GRID
                if p.type == "gridvolume_spectral":                      # src/textures/gridvolume_spectral.cpp:84-135,186-190
                    if not self.spectral:
                        raise RuntimeError("This volume data source can only be used with a spectral variant!")
                    rec.type = A.VOLUME_GRID_SPECTRAL
                    st = str(p.get("spectrum_type", "regular"))
                    if st != "regular":
                        raise RuntimeError("Invalid spectrum type \"%s\", must be \"regular\"!" % st)
                    if not p.has("lambda_min"):
                        raise RuntimeError("Property \"lambda_min\" has not been specified!")
                    if not p.has("lambda_max"):
                        raise RuntimeError("Property \"lambda_max\" has not been specified!")
                    rec.lambda_min, rec.lambda_max = float(p.get("lambda_min")), float(p.get("lambda_max"))
                if p.has("filename"):
                    data, meta = read_volume(file_resolver().resolve(p.get("filename")))
                    rec.file_bbox_min[:] = meta["bbox_min"]
                    rec.file_bbox_max[:] = meta["bbox_max"]
                elif p.has("data"):
                    # in-memory grid: array of shape (nz, ny, nx[, channels]) (extension; the reference reads a file)
                    data = p.get("data")
                    rec.file_bbox_min[:] = (0.0, 0.0, 0.0)
                    rec.file_bbox_max[:] = (1.0, 1.0, 1.0)
                else:
                    raise RuntimeError("gridvolume: property \"filename\" has not been specified!")
                data, mono_max = self._grid_data(data)
                self.keep.append(data)
                self.grids[len(self.volumes)] = data                     # traverse(): "data"; mono_max follows an update unless "max_value" is set
                self.grid_mono_max[len(self.volumes)] = mono_max is not None and not p.has("max_value")
                rec.data = data.ctypes.data_as(A.fp)
                rec.nz, rec.ny, rec.nx, rec.channels = data.shape
                ft = str(p.get("filter_type", "trilinear"))
                if p.type == "gridvolume_spectral" and ft != "trilinear":
                    raise RuntimeError("Invalid filter type \"%s\", must be \"trilinear\"!" % ft)
                if ft not in ("nearest", "trilinear"):
                    raise RuntimeError("Invalid filter type \"%s\", must be one of: \"nearest\" or \"trilinear\"!" % ft)
                rec.filter_type = A.FILTER_NEAREST if ft == "nearest" else A.FILTER_TRILINEAR
                wm = str(p.get("wrap_mode", "clamp"))
                if wm not in ("repeat", "mirror", "clamp"):
                    raise RuntimeError("Invalid wrap mode \"%s\", must be one of: \"repeat\", \"mirror\", or \"clamp\"!" % wm)
                rec.wrap_mode = {"repeat": A.WRAP_REPEAT, "mirror": A.WRAP_MIRROR, "clamp": A.WRAP_CLAMP}[wm]
                rec.use_grid_bbox = int(bool(p.get("use_grid_bbox", False)))
                p.get("raw", False)
                if p.has("max_value"):
                    rec.has_max_value = 1
                    rec.max_value = float(p.get("max_value"))
                elif mono_max is not None:
                    rec.has_max_value = 1
                    rec.max_value = mono_max
            p.finish()
        else:
            # float / rgb given where a volume is expected -> constvolume (properties.h:319-366)
            rec.type = A.VOLUME_CONST
            if self.spectral:
                rec.value_spectrum = self._spectrum(v, where)
            else:
                rec.value[:] = self._color(v, where)
        if rec.type == A.VOLUME_CONST:                                   # constant3d.cpp:39-41
            self.nodes[("volume", len(self.volumes))] = [("object", "color", self._colour_node("volume", len(self.volumes), "value", where, rec.value_spectrum))]
        else:                                                            # grid3d.cpp:366-369, gridvolume_spectral.cpp:388-392
            self.nodes[("volume", len(self.volumes))] = [("param", "data", "grid", "data"), ("param", "size", "size", None)]
        self.volumes.append(rec)
        self._register(v, "volume", len(self.volumes) - 1)
        return len(self.volumes) - 1

    # ------------------------------------------------------------ phase functions
    def add_phase(self, d, where):
        r = self._resolve_ref(d, "phase")
        if r is not None:
            return r
        rec = A.Phase()
        rec.child[:] = (-1, -1)
        rec.weight_volume = -1
        if d is None:
            rec.type = A.PHASE_ISOTROPIC
        else:
            p = Props(d, where)
            if p.type == "isotropic":
                rec.type = A.PHASE_ISOTROPIC
            elif p.type == "hg":
                rec.type = A.PHASE_HG
                rec.g = float(p.get("g", 0.8))
            elif p.type == "rayleigh":
                rec.type = A.PHASE_RAYLEIGH
            elif p.type == "tabphase":
                rec.type = A.PHASE_TABULATED
                arr = _tab_values(p.get("values"))
                self.keep.append(arr)
                rec.tab_values = arr.ctypes.data_as(A.fp)
                rec.tab_count = arr.size
            elif p.type == "blendphase":
                rec.type = A.PHASE_BLEND
                children = []
                for k, v in sorted_items(d):  # nested phase functions in Properties order (blendphase.cpp:33-43)
                    if isinstance(v, dict) and v.get("type") in ("isotropic", "hg", "rayleigh", "tabphase", "blendphase", "ref") and k != "weight":
                        p.queried.add(k)
                        children.append(self.add_phase(v, where + "." + k))
                if len(children) != 2:
                    raise RuntimeError("BlendPhase: Two child phase functions must be specified!")
                rec.child[:] = children
                if not p.has("weight"):
                    raise RuntimeError("Property \"weight\" has not been specified!")
                rec.weight_volume = self.add_volume(p.get("weight"), where + ".weight")
            else:
                raise RuntimeError("Unknown / unsupported phase function plugin \"%s\"" % p.type)
            p.finish()
        node = []
        if rec.type == A.PHASE_HG:                                       # hg.cpp:86-88
            node = [("param", "g", "float", "g")]
        elif rec.type == A.PHASE_TABULATED:                              # tabphase.cpp:97-99
            node = [("param", "values", "tab", "tab_values")]
            self.tabs[len(self.phases)] = arr
        elif rec.type == A.PHASE_BLEND:                                  # blendphase.cpp:141-145
            node = [("object", "weight", ("volume", rec.weight_volume)), ("object", "phase_0", ("phase", rec.child[0])), ("object", "phase_1", ("phase", rec.child[1]))]
        self.nodes[("phase", len(self.phases))] = node
        self.phases.append(rec)
        self._register(d, "phase", len(self.phases) - 1)
        return len(self.phases) - 1

    # ------------------------------------------------------------ media
    def add_medium(self, d, where):
        r = self._resolve_ref(d, "medium")
        if r is not None:
            return r
        p = Props(d, where)
        rec = A.Medium()
        if p.type == "homogeneous":
            rec.type = A.MEDIUM_HOMOGENEOUS
        elif p.type == "heterogeneous":
            rec.type = A.MEDIUM_HETEROGENEOUS
        else:
            raise RuntimeError("Unknown / unsupported medium plugin \"%s\"" % p.type)
        rec.albedo_volume = self.add_volume(p.get("albedo"), where + ".albedo", default=0.75)
        rec.sigma_t_volume = self.add_volume(p.get("sigma_t"), where + ".sigma_t", default=1.0)
        rec.scale = float(p.get("scale", 1.0))
        rec.has_spectral_extinction = int(bool(p.get("has_spectral_extinction", True)))
        rec.sample_emitters = int(bool(p.get("sample_emitters", True)))
        phase = None
        for k, v in sorted_items(d):         # any nested phase function (medium.cpp:13-22)
            if isinstance(v, dict) and v.get("type") in ("isotropic", "hg", "rayleigh", "tabphase", "blendphase") \
                    or (isinstance(v, dict) and v.get("type") == "ref" and self.instances.get(v.get("id"), ("",))[0] == "phase"):
                if phase is not None:
                    raise RuntimeError("Only a single phase function can be specified per medium")
                p.queried.add(k)
                phase = self.add_phase(v, where + "." + k)
        rec.phase = phase if phase is not None else self.add_phase(None, where + ".phase")
        p.finish()
        # homogeneous.cpp / heterogeneous.cpp:56-61; the phase function under the name Medium::traverse gives it upstream (this fork's Medium
        # does not list it: without the name the phase parameters of a medium could not be reached)
        self.nodes[("medium", len(self.media))] = [("param", "scale", "float", "scale"), ("object", "albedo", ("volume", rec.albedo_volume)),
                                                   ("object", "sigma_t", ("volume", rec.sigma_t_volume)), ("object", "phase_function", ("phase", rec.phase))]
        self.media.append(rec)
        self._register(d, "medium", len(self.media) - 1)
        return len(self.media) - 1

    # ------------------------------------------------------------ textures
    def _is_texture(self, v):
        if not isinstance(v, dict):
            return False
        if v.get("type") == "ref":
            return self.instances.get(v.get("id"), (None,))[0] == "texture"
        return v.get("type") in TEXTURE_PLUGINS

    def add_texture(self, d, where):
        """src/textures/bitmap.cpp:92-206, src/textures/checkerboard.cpp:40-44 -> index of the mts_texture record"""
        r = self._resolve_ref(d, "texture")
        if r is not None:
            return r
        if self.spectral:
            raise RuntimeError("Textures are not supported in the spectral variant (\"%s\" in %s): rgb texels need the sRGB upsampling "
                               "model, whose data this backend has not got" % (d.get("type"), where))
        p = Props(d, where)
        rec = A.Texture()
        index = len(self.textures)
        rec.to_uv[:] = _to_uv(p.get("to_uv"))
        if p.type == "checkerboard":
            rec.type = A.TEXTURE_CHECKERBOARD
            node = [("param", "transform", "to_uv", "to_uv")]                # checkerboard.cpp:92-96
            for key, default in (("color0", 0.4), ("color1", 0.2)):
                v = p.get(key, default)
                if isinstance(v, dict) and v.get("type") in TEXTURE_PLUGINS + ("ref",):
                    raise RuntimeError("checkerboard: \"%s\" must be a constant (a float or rgb) in this backend, not a nested texture: %s" % (key, where))
                getattr(rec, key)[:] = self._color(v, where + "." + key)
                node.append(("object", key, ("colour", "texture", index, key, where + "." + key, False)))
        else:
            rec.type = A.TEXTURE_BITMAP
            if p.has("filename") == p.has("data"):
                raise RuntimeError("bitmap: give either \"filename\" (a .pfm file) or \"data\" (an array): %s" % where)
            if p.has("filename"):
                name = str(p.get("filename"))
                if not name.lower().endswith(".pfm"):
                    raise RuntimeError("bitmap: cannot read \"%s\": this backend reads PFM files (.pfm) only; pass other images as "
                                       "\"data\" (a linear float32 array of shape (height, width) or (height, width, 3))" % name)
                data = read_pfm(file_resolver().resolve(name))
            else:
                data = p.get("data")
            ft = str(p.get("filter_type", "bilinear"))
            if ft not in ("nearest", "bilinear"):
                raise RuntimeError("Invalid filter type \"%s\", must be one of: \"nearest\", or \"bilinear\"!" % ft)      # bitmap.cpp:100-107
            wm = str(p.get("wrap_mode", "repeat"))
            if wm not in ("repeat", "mirror", "clamp"):
                raise RuntimeError("Invalid wrap mode \"%s\", must be one of: \"repeat\", \"mirror\", or \"clamp\"!" % wm)   # bitmap.cpp:109-118
            p.get("raw", False)                                          # linear float data either way: nothing to undo
            data = self._bitmap_data(data)
            self.keep.append(data)
            self.bitmaps[index] = data
            rec.data = data.ctypes.data_as(A.fp)
            rec.height, rec.width, rec.channels = data.shape
            rec.filter_type = A.FILTER_NEAREST if ft == "nearest" else A.FILTER_BILINEAR
            rec.wrap_mode = {"repeat": A.WRAP_REPEAT, "mirror": A.WRAP_MIRROR, "clamp": A.WRAP_CLAMP}[wm]
            node = [("param", "data", "texels", "data"), ("param", "resolution", "resolution", None), ("param", "transform", "to_uv", "to_uv")]      # bitmap.cpp:561-565
        p.finish()
        self.nodes[("texture", index)] = node
        self.textures.append(rec)
        self._register(d, "texture", index)
        return index

    # ------------------------------------------------------------ BSDFs
    def add_bsdf(self, d, where):
        r = self._resolve_ref(d, "bsdf")
        if r is not None:
            return r
        p = Props(d, where)
        rec = A.Bsdf()
        rec.spectrum[:] = [-1] * 6
        spectral = self.spectral
        node = []
        textures = [-1] * 6                                              # per colour parameter: its texture record, -1 = the constant
        def colour(field, slot, key, default):                           # rgb triple, or (spectral variant) the index of the spectrum
            if self._is_texture(p.d.get(key)):                           # a bitmap / checkerboard; the record's own constant (what a reader that
                textures[slot] = self.add_texture(p.get(key), where + "." + key)      # knows no textures sees) is the parameter's default
                getattr(rec, field)[:] = self._color(default, where) if default is not None else tuple(rec.rho_0)
                node.append(("object", key, ("texture", textures[slot])))
                return
            if spectral:
                rec.spectrum[slot] = self._spectrum(p.get(key), where + "." + key, default=default)
            else:
                getattr(rec, field)[:] = self._color(p.get(key), where, default=default)
            node.append(("object", key, self._colour_node("bsdf", len(self.bsdfs), field, where, rec.spectrum[slot])))
        if p.type == "diffuse":
            rec.type = A.BSDF_DIFFUSE
            colour("reflectance", 0, "reflectance", 0.5)
        elif p.type == "null":
            rec.type = A.BSDF_NULL
        elif p.type == "bilambertian":                                   # src/bsdfs/bilambertian.cpp:51-60
            rec.type = A.BSDF_BILAMBERTIAN
            colour("reflectance", 0, "reflectance", 0.5)
            colour("transmittance", 5, "transmittance", 0.5)
        elif p.type == "rpv":
            rec.type = A.BSDF_RPV
            colour("rho_0", 1, "rho_0", 0.1)
            colour("g", 3, "g", 0.0)
            colour("k", 2, "k", 0.1)
            if p.has("rho_c"):
                colour("rho_c", 4, "rho_c", None)
            elif spectral:
                rec.spectrum[4] = rec.spectrum[1]                        # rpv.cpp:75-79: rho_c defaults to rho_0
            else:
                rec.rho_c[:] = tuple(rec.rho_0)                          # (one texture under two names: traverse() lists it once, an update of rho_0 reaches both)
                textures[4] = textures[1]
                if textures[1] < 0:
                    node[0] = ("object", "rho_0", ("colour", "bsdf", len(self.bsdfs), "rho_0+rho_c", where, False))
        elif p.type == "blendbsdf":                                      # src/bsdfs/blendbsdf.cpp:59-81
            rec.type = A.BSDF_BLEND
            if spectral:
                raise RuntimeError("\"blendbsdf\" is not supported in the spectral variant (%s): refused where textures are, its weight is one" % where)
            children = []
            for k, v in sorted_items(d):                                 # the nested BSDFs in Properties order (:61-69), whatever they are called
                if k in ("type", "id", "weight") or not isinstance(v, dict):
                    continue
                if v.get("type") == "ref" and self.instances.get(v.get("id"), ("bsdf",))[0] != "bsdf":
                    continue
                if len(children) == 2:
                    raise RuntimeError("BlendBSDF: Cannot specify more than two child BSDFs")
                p.queried.add(k)
                child = self.add_bsdf(v, where + "." + k)
                for plugin, kind in (("null", A.BSDF_NULL), ("blendbsdf", A.BSDF_BLEND), ("twosided", A.BSDF_TWOSIDED)):
                    if self.bsdfs[child].type == kind:
                        raise RuntimeError("\"blendbsdf\" %s: the nested BSDF \"%s\" is a \"%s\", which this backend cannot nest in a blend (a null or "
                                           "nested child needs the component flags the integrators read)" % (where, k, plugin))
                for plugin, kind in (("dielectric", A.BSDF_DIELECTRIC), ("conductor", A.BSDF_CONDUCTOR)):
                    if self.bsdfs[child].type == kind:
                        raise RuntimeError("\"blendbsdf\" %s: the nested BSDF \"%s\" is a \"%s\": specular children are not supported in a blend "
                                           "by this backend" % (where, k, plugin))
                children.append(child)
            if not p.has("weight"):
                raise RuntimeError("Property \"weight\" has not been specified!")        # props.texture("weight"), :71
            wv, wwhere = p.get("weight"), where + ".weight"
            if len(children) != 2:
                raise RuntimeError("BlendBSDF: Two child BSDFs must be specified!")
            rec.spectrum[0], rec.spectrum[1] = children                  # mtsamd.h: a blend's use of the record
            if self._is_texture(wv):
                textures[0] = self.add_texture(wv, wwhere)
                _check_weight_texture(wv, self.textures[textures[0]], wwhere)
                rec.reflectance[:] = (0.5, 0.5, 0.5)                     # (what a reader that knows no textures sees)
                node.append(("object", "weight", ("texture", textures[0])))
            else:
                rec.reflectance[:] = (_weight(wv, wwhere),) * 3
                node.append(("object", "weight", ("uniform", "bsdf", len(self.bsdfs), "reflectance", wwhere)))
            node += [("object", "bsdf_0", ("bsdf", children[0])), ("object", "bsdf_1", ("bsdf", children[1]))]      # :166-170
            self.blends.append(where)
        elif p.type == "twosided":                                       # src/bsdfs/twosided.cpp:63-92
            rec.type = A.BSDF_TWOSIDED
            if spectral:
                raise RuntimeError("\"twosided\" is not supported in the spectral variant (%s): it renders in the kernels of textured scenes, "
                                   "which that variant has not got" % where)
            children = []
            for k, v in sorted_items(d):                                 # the nested BSDFs in Properties order (:64-70), whatever they are called
                if k in ("type", "id") or not isinstance(v, dict):
                    continue
                if v.get("type") == "ref" and self.instances.get(v.get("id"), ("bsdf",))[0] != "bsdf":
                    continue
                if len(children) == 2:
                    raise RuntimeError("At most two nested BSDFs can be specified!")
                p.queried.add(k)
                child = self.add_bsdf(v, where + "." + k)
                if self.bsdfs[child].type == A.BSDF_TWOSIDED:
                    raise RuntimeError("\"twosided\" %s: the nested BSDF \"%s\" is a \"twosided\", which this backend cannot nest in another" % (where, k))
                children.append(child)
            if not children:
                raise RuntimeError("A nested one-sided material is required!")
            if len(children) == 1:
                children.append(children[0])                             # :74-75
            flags = ((self._bsdf_flags(children[0]) & ~_F_BACK) | _F_FRONT) | ((self._bsdf_flags(children[1]) & ~_F_FRONT) | _F_BACK)     # :78-88
            if flags & _F_TRANSMISSION:
                raise RuntimeError("Only materials without a transmission component can be nested!")
            rec.spectrum[0], rec.spectrum[1] = children                  # mtsamd.h: a twosided's use of the record
            # :183-186.  One child under both names: brdf_1 lists the keys of brdf_0 again, and an update through either rewrites the one record
            node += [("object", "brdf_0", ("bsdf", children[0])),
                     ("alias" if children[0] == children[1] else "object", "brdf_1", ("bsdf", children[1]))]
            self.twosided.append(where)
        elif p.type in ("dielectric", "conductor"):                      # src/bsdfs/dielectric.cpp:174-199, src/bsdfs/conductor.cpp:200-215
            if spectral:
                raise RuntimeError("\"%s\" is not supported in the spectral variant (%s): it renders in the kernels of textured scenes, "
                                   "which that variant has not got" % (p.type, where))
            if p.type == "dielectric":
                rec.type = A.BSDF_DIELECTRIC
                int_ior, ext_ior = lookup_ior(p.get("int_ior"), "bk7"), lookup_ior(p.get("ext_ior"), "air")
                if int_ior < 0 or ext_ior < 0:
                    raise RuntimeError("The interior and exterior indices of refraction must be positive!")
                with np.errstate(divide="ignore", invalid="ignore"):
                    eta = float(np.float32(int_ior) / np.float32(ext_ior))
                if not (math.isfinite(eta) and eta > 0):
                    raise RuntimeError("\"dielectric\" %s: eta = int_ior / ext_ior = %r must be finite and positive" % (where, eta))
                rec.rho_0[:] = (eta,) * 3
                node.append(("param", "eta", "eta", "rho_0"))            # :322-328: eta, and the two colours only if the scene gave them
                rec.reflectance[:] = (1.0,) * 3
                rec.transmittance[:] = (1.0,) * 3
                if p.has("specular_reflectance"):
                    colour("reflectance", 0, "specular_reflectance", 1.0)
                if p.has("specular_transmittance"):
                    colour("transmittance", 5, "specular_transmittance", 1.0)
            else:
                rec.type = A.BSDF_CONDUCTOR
                colour("reflectance", 0, "specular_reflectance", 1.0)    # :282-286: specular_reflectance, eta, k
                material = str(p.get("material", "none"))
                if not (p.has("eta") or material == "none"):
                    raise RuntimeError("\"conductor\" %s: the material preset \"%s\" is not supported by this backend (the measured indices of "
                                       "refraction behind the names are not shipped): give \"eta\" and \"k\"" % (where, material))
                if material != "none":
                    raise RuntimeError("Should specify either (eta, k) or material, not both.")
                for field, key, default in (("rho_0", "eta", 0.0), ("k", "k", 1.0)):
                    if self._is_texture(p.d.get(key)):
                        raise RuntimeError("\"conductor\" %s: a texture on \"%s\" is not supported by this backend: give a float, an rgb colour "
                                           "or a uniform spectrum" % (where, key))
                    c = self._color(p.get(key), where + "." + key, default=default)
                    if not all(math.isfinite(x) for x in c):
                        raise RuntimeError("\"conductor\" %s: \"%s\" must be finite" % (where, key))
                    getattr(rec, field)[:] = c
                    node.append(("object", key, ("colour", "bsdf", len(self.bsdfs), field, where + "." + key, False)))
            self.specular.append(where)
        else:
            raise RuntimeError("Unknown / unsupported BSDF plugin \"%s\"" % p.type)
        p.finish()
        self.nodes[("bsdf", len(self.bsdfs))] = node
        self.bsdf_textures.append(textures)
        self.bsdfs.append(rec)
        self._register(d, "bsdf", len(self.bsdfs) - 1)
        return len(self.bsdfs) - 1

    def _bsdf_flags(self, i):
        """BSDFFlags of record i as the library computes them (scene_host.cpp: bsdf_flags, resolve_blend, resolve_twosided)."""
        rec = self.bsdfs[i]
        if rec.type in (A.BSDF_BLEND, A.BSDF_TWOSIDED):
            return self._bsdf_flags(rec.spectrum[0]) | self._bsdf_flags(rec.spectrum[1])
        return {A.BSDF_DIFFUSE: 0x2 | _F_FRONT, A.BSDF_NULL: 0x1 | _F_FRONT | _F_BACK, A.BSDF_RPV: 0x8 | _F_FRONT,
                A.BSDF_BILAMBERTIAN: 0x2 | 0x4 | _F_FRONT | _F_BACK,
                A.BSDF_DIELECTRIC: _F_DELTA_REFLECTION | _F_DELTA_TRANSMISSION | _F_FRONT | _F_BACK | _F_NON_SYMMETRIC,
                A.BSDF_CONDUCTOR: _F_DELTA_REFLECTION | _F_FRONT}[rec.type]

    # ------------------------------------------------------------ shapes
    def make_shape(self, d, where, in_scene=True):
        p = Props(d, where)
        rec = A.Shape()
        rec.bsdf = rec.interior_medium = rec.exterior_medium = rec.emitter = -1
        rec.radius = 1.0
        rec.to_world = _xf(p.get("to_world"))
        if p.type == "rectangle":
            rec.type = A.SHAPE_RECTANGLE
            rec.flip_normals = int(bool(p.get("flip_normals", False)))
        elif p.type == "disk":                                           # src/shapes/disk.cpp:74-81
            rec.type = A.SHAPE_DISK
            rec.flip_normals = int(bool(p.get("flip_normals", False)))
        elif p.type == "cube":
            rec.type = A.SHAPE_CUBE
        elif p.type == "sphere":
            rec.type = A.SHAPE_SPHERE
            rec.flip_normals = int(bool(p.get("flip_normals", False)))
            rec.center[:] = tuple(float(x) for x in np.asarray(p.get("center", (0, 0, 0)), dtype=np.float32))
            rec.radius = float(p.get("radius", 1.0))
        elif p.type == "cone":                                           # src/shapes/cone.cpp:79-85: to_world and flip_normals, nothing else --
            rec.type = A.SHAPE_CONE                                      # "p0", "p1" and "radius" of its documentation are never queried
            rec.flip_normals = int(bool(p.get("flip_normals", False)))
            _check_cone_transform(np.array(list(rec.to_world.matrix), np.float32).reshape(4, 4), where)
            self.cones.append(where)
        elif p.type in ("mesh", "obj", "ply"):
            # "mesh": in-memory triangle mesh (extension); "obj" / "ply": src/shapes/obj.cpp, src/shapes/ply.cpp via mesh_io.py,
            # which applies to_world at load time like the reference's loaders
            rec.type = A.SHAPE_MESH
            if p.type == "mesh":
                arrays = {k: p.get(k) for k in ("vertex_positions", "faces", "vertex_normals", "vertex_texcoords") if p.has(k)}
            else:
                arrays = load_mesh(p.type, file_resolver().resolve(p.get("filename")), p.get("to_world"), bool(p.get("face_normals", False)),
                                   bool(p.get("flip_tex_coords", True)) if p.type == "obj" else True)
                rec.to_world = _xf(None)

            class _Arr:                                                    # the parsed arrays, read like properties below
                def has(self, k): return k in arrays
                def get(self, k): return arrays[k]
            p_arr = _Arr()
            pos = np.ascontiguousarray(arrays["vertex_positions"], dtype=np.float32).reshape(-1, 3)
            faces = np.ascontiguousarray(arrays["faces"], dtype=np.uint32).reshape(-1, 3)
            self.keep += [pos, faces]
            rec.vertex_positions = pos.ctypes.data_as(A.fp)
            rec.faces = faces.ctypes.data_as(C.POINTER(C.c_uint32))
            rec.vertex_count, rec.face_count = pos.shape[0], faces.shape[0]
            if p_arr.has("vertex_normals"):
                nor = np.ascontiguousarray(p_arr.get("vertex_normals"), dtype=np.float32).reshape(-1, 3)
                self.keep.append(nor)
                rec.vertex_normals = nor.ctypes.data_as(A.fp)
            if p_arr.has("vertex_texcoords"):
                uv = np.ascontiguousarray(p_arr.get("vertex_texcoords"), dtype=np.float32).reshape(-1, 2)
                self.keep.append(uv)
                rec.vertex_texcoords = uv.ctypes.data_as(A.fp)
        else:
            raise RuntimeError("Unknown / unsupported shape plugin \"%s\"" % p.type)
        emitter_dict = None
        for k, v in sorted_items(d):
            if k in p.queried or not isinstance(v, dict):
                continue
            t = v.get("type")
            kind = self.instances.get(v.get("id"), ("",))[0] if t == "ref" else None
            if t in BSDF_PLUGINS or kind == "bsdf":
                if rec.bsdf >= 0:
                    raise RuntimeError("Only a single BSDF child object can be specified per shape.")
                p.queried.add(k)
                rec.bsdf = self.add_bsdf(v, where + "." + k)
            elif t in ("homogeneous", "heterogeneous") or kind == "medium":
                p.queried.add(k)
                if k == "interior":
                    rec.interior_medium = self.add_medium(v, where + "." + k)
                elif k == "exterior":
                    rec.exterior_medium = self.add_medium(v, where + "." + k)
                else:
                    self.add_medium(v, where + "." + k)   # shape.cpp:58-68: other names are ignored
            elif t == "area":
                if emitter_dict is not None:
                    raise RuntimeError("Only a single Emitter child object can be specified per shape.")
                p.queried.add(k)
                emitter_dict = v
        p.finish()
        if not in_scene:
            return rec, None
        return rec, emitter_dict

    def add_shape(self, d, where):
        rec, emitter_dict = self.make_shape(d, where)
        if emitter_dict is not None and rec.type == A.SHAPE_CONE:
            raise RuntimeError("\"%s\": an \"area\" emitter on a cone is not supported by this backend (the cone's sample_position is not built)" % where)
        self.shapes.append(rec)
        idx = len(self.shapes) - 1
        if emitter_dict is not None:
            ep = Props(emitter_dict, where + ".emitter")
            e = A.Emitter()
            e.type = A.EMITTER_AREA
            e.to_world = _xf(None)
            self._emitter_colour(e, ep.get("radiance"), where)
            e.shape = idx
            ep.finish()
            self.nodes[("emitter", len(self.emitters))] = [("object", "radiance", self._colour_node("emitter", len(self.emitters), "radiance", where, e.radiance_spectrum, True))]
            self.emitters.append(e)
            self.shapes[idx].emitter = len(self.emitters) - 1
        # shape.cpp:398-413 (+ mesh.cpp:836-848); a shape without a BSDF of its own gets the default one, which the description does not hold
        node = [("param", "to_world", "geometry", "to_world")]
        if rec.type == A.SHAPE_MESH:
            node += [("param", "vertex_count", "geometry", "vertex_count"), ("param", "face_count", "geometry", "face_count"), ("param", "faces_buf", "geometry", "faces"),
                     ("param", "vertex_positions_buf", "geometry", "vertex_positions")]
            node += [("param", "vertex_normals_buf", "geometry", "vertex_normals")] if rec.vertex_normals else []
            node += [("param", "vertex_texcoords_buf", "geometry", "vertex_texcoords")] if rec.vertex_texcoords else []
        for name, kind, i in (("bsdf", "bsdf", rec.bsdf), ("emitter", "emitter", rec.emitter), ("interior_medium", "medium", rec.interior_medium),
                              ("exterior_medium", "medium", rec.exterior_medium)):
            if i >= 0:
                node.append(("object", name, (kind, i)))
        self.nodes[("shape", idx)] = node
        self._register(d, "shape", idx)
        return idx

    # ------------------------------------------------------------ instanced geometry (src/shapes/shapegroup.cpp, instance.cpp; librender/shapegroup.cpp)
    def add_shapegroup(self, d, where):
        """A shapegroup: its record (mtsamd.h: MTS_SHAPE_SHAPEGROUP, face_count = the number of members) and, directly behind it, its
        members' records -- shapes that are NOT part of the scene's geometry (scene.cpp:36-41).  The reference's ShapeGroup does not
        traverse into its members, so the node lists nothing; what members reference by id is listed where it was declared."""
        p = Props(d, where)
        grp = A.Shape()
        grp.type = A.SHAPE_SHAPEGROUP
        grp.bsdf = grp.interior_medium = grp.exterior_medium = grp.emitter = -1
        grp.to_world = _xf(None)
        self.shapes.append(grp)
        gidx = len(self.shapes) - 1
        members = 0
        for k, v in sorted_items(d):                                     # librender/shapegroup.cpp:15-40, in props.objects() order
            if k in p.queried or not isinstance(v, dict):
                continue
            p.queried.add(k)
            t = v.get("type")
            kind = self.instances.get(v.get("id"), ("",))[0] if t == "ref" else None
            if t == "instance" or kind == "instance":
                if t == "instance":
                    self._instance_group(v, where + "." + k)             # the child is constructed first: its own errors come first
                raise RuntimeError("Nested instancing is not permitted")
            if t == "shapegroup" or kind == "shapegroup":
                raise RuntimeError("Nested ShapeGroup is not permitted")
            if kind == "shape":
                raise RuntimeError("\"%s\": a shapegroup member given by reference is not supported by this backend (declare the shape inside the group)" % (where + "." + k))
            if t not in SHAPE_PLUGINS:
                raise RuntimeError("Tried to add an unsupported object of type \"%s\" (key \"%s\" of shapegroup \"%s\")" % (t, k, where))
            rec, emitter_dict = self.make_shape(v, where + "." + k)
            if emitter_dict is not None:
                raise RuntimeError("Instancing of emitters is not supported")
            for key, medium in (("interior", rec.interior_medium), ("exterior", rec.exterior_medium)):
                if medium >= 0:
                    raise RuntimeError("\"%s\": an \"%s\" medium on a shapegroup member is not supported by this backend" % (where + "." + k, key))
            self.shapes.append(rec)
            members += 1
        p.finish()
        self.shapes[gidx].face_count = members
        self.nodes[("shape", gidx)] = []
        if isinstance(d, dict) and "id" in d:
            self.instances[d["id"]] = ("shapegroup", gidx)
        self.groups.append(where)
        return gidx

    def _instance_group(self, d, where):
        """The one shapegroup of an instance (instance.cpp:66-78): inline, or a reference to one declared before."""
        group = None
        for k, v in sorted_items(d):
            if k in ("type", "id", "to_world") or not isinstance(v, dict):
                continue
            t = v.get("type")
            kind = self.instances.get(v.get("id"), ("",))[0] if t == "ref" else None
            if t == "ref" and v.get("id") not in self.instances:
                raise RuntimeError("Referenced id \"%s\" not found" % v.get("id"))
            if t == "shapegroup" or kind == "shapegroup":
                if group is not None:
                    raise RuntimeError("Only a single shapegroup can be specified per instance.")
                group = self.add_shapegroup(v, where + "." + k) if t == "shapegroup" else self.instances[v["id"]][1]
            else:
                if t == "instance":                                      # a child is constructed before its parent: its own errors come first
                    self._instance_group(v, where + "." + k)
                raise RuntimeError("Only a shapegroup can be specified in an instance.")
        if group is None:
            raise RuntimeError("A reference to a 'shapegroup' must be specified!")
        return group

    def add_instance(self, d, where):
        """An instance (mtsamd.h: MTS_SHAPE_INSTANCE): to_world and, in vertex_count, the index of its group's record."""
        p = Props(d, where)
        rec = A.Shape()
        rec.type = A.SHAPE_INSTANCE
        rec.bsdf = rec.interior_medium = rec.exterior_medium = rec.emitter = -1
        rec.to_world = _xf(p.get("to_world"))
        for k, v in d.items():
            if isinstance(v, dict) and k != "to_world":
                p.queried.add(k)
        group = self._instance_group(d, where)
        p.finish()
        rec.vertex_count = group
        self.shapes.append(rec)
        idx = len(self.shapes) - 1
        self.nodes[("shape", idx)] = [("param", "to_world", "geometry", "to_world")]
        if isinstance(d, dict) and "id" in d:
            self.instances[d["id"]] = ("instance", idx)
        self.instanced.append(where)
        return idx

    # ------------------------------------------------------------ emitters
    def add_emitter(self, d, where):
        p = Props(d, where)
        e = A.Emitter()
        e.shape = -1
        if p.type == "directional":
            e.type = A.EMITTER_DIRECTIONAL
            if p.has("direction"):
                if p.has("to_world"):
                    raise RuntimeError("Only one of the parameters 'direction' and 'to_world' can be specified at the same time!'")
                direction = np.asarray(p.get("direction"), dtype=np.float32)
                direction = normalize32(direction)
                up, _ = coordinate_system(direction)                       # directional.cpp:55-60
                e.to_world = _xf(ScalarTransform4f.look_at([0, 0, 0], direction, up))
            else:
                e.to_world = _xf(p.get("to_world"))
            self._emitter_colour(e, p.get("irradiance"), where)
        elif p.type == "constant":
            e.type = A.EMITTER_CONSTANT
            e.to_world = _xf(None)
            self._emitter_colour(e, p.get("radiance"), where)
        elif p.type == "point":                                             # point.cpp:45-58
            e.type = A.EMITTER_POINT
            if p.has("position"):
                if p.has("to_world"):
                    raise RuntimeError("Only one of the parameters 'position' and 'to_world' can be specified at the same time!'")
                e.to_world = _xf(ScalarTransform4f.translate(np.asarray(p.get("position"), dtype=np.float32)))
            else:
                e.to_world = _xf(p.get("to_world"))
            self._emitter_colour(e, p.get("intensity"), where)
        elif p.type == "area":
            raise RuntimeError("Can't sample from an area emitter without an associated Shape.")
        else:
            raise RuntimeError("Unknown / unsupported emitter plugin \"%s\"" % p.type)
        p.finish()
        key = {A.EMITTER_DIRECTIONAL: "irradiance", A.EMITTER_CONSTANT: "radiance", A.EMITTER_POINT: "intensity"}[e.type]
        self.nodes[("emitter", len(self.emitters))] = [("object", key, self._colour_node("emitter", len(self.emitters), "radiance", where, e.radiance_spectrum, True))]
        self.emitters.append(e)
        return len(self.emitters) - 1

    # ------------------------------------------------------------ sensor
    def set_sensor(self, d, where):
        p = Props(d, where)
        s = A.Sensor()
        s.medium = -1
        for shape in (s.distant_target_shape, s.distant_origin_shape):
            shape.bsdf = shape.interior_medium = shape.exterior_medium = shape.emitter = -1
        self._film(p, s, where)
        self._sampler(p, s, where)
        shutter_open, shutter_close = float(p.get("shutter_open", 0.0)), float(p.get("shutter_close", 0.0))      # sensor.cpp:20-27
        if shutter_close < shutter_open:
            raise RuntimeError("Shutter opening time must be less than or equal to the shutter closing time!")
        s.shutter_open_time = shutter_close - shutter_open
        if p.has("medium"):
            s.medium = self.add_medium(p.get("medium"), where + ".medium")
        if p.type not in SENSOR_PLUGINS:
            raise RuntimeError("Unknown / unsupported sensor plugin \"%s\"" % p.type)
        SENSOR_PLUGINS[p.type](self, p, s, where)
        p.finish()
        self.sensor_pixel_formats.append(self._pixel_format)
        if self.sensor is None:
            self.sensor = s
            self.film_pixel_format = self._pixel_format                   # sensor 0's, as ever
        else:
            self.extra_sensors.append(s)

    def _film(self, p, s, where):
        """film (src/librender/film.cpp:14-50, src/films/hdrfilm.cpp) and its reconstruction filter"""
        fp_ = Props(p.get("film", {"type": "hdrfilm"}), where + ".film")
        if fp_.type != "hdrfilm":
            raise RuntimeError("Unknown / unsupported film plugin \"%s\"" % fp_.type)
        s.film_width, s.film_height = int(fp_.get("width", 768)), int(fp_.get("height", 576))
        s.crop_offset[:] = (int(fp_.get("crop_offset_x", 0)), int(fp_.get("crop_offset_y", 0)))
        s.crop_size[:] = (int(fp_.get("crop_width", s.film_width)), int(fp_.get("crop_height", s.film_height)))
        if (s.crop_offset[0] < 0 or s.crop_offset[1] < 0 or s.crop_size[0] <= 0 or s.crop_size[1] <= 0 or
                s.crop_offset[0] + s.crop_size[0] > s.film_width or s.crop_offset[1] + s.crop_size[1] > s.film_height):
            raise RuntimeError("Invalid crop window specification!")
        # hdrfilm.cpp:100-151: the format strings are validated even though only Film.bitmap() consumes the pixel format here
        ff = str(fp_.get("file_format", "openexr")).lower()
        if ff not in ("openexr", "exr", "rgbe", "pfm"):
            raise RuntimeError("The \"file_format\" parameter must either be equal to \"openexr\", \"pfm\", or \"rgbe\", found %s instead." % ff)
        pf = str(fp_.get("pixel_format", "rgba")).lower()
        if pf not in ("luminance", "luminance_alpha", "rgb", "rgba", "xyz", "xyza"):
            raise RuntimeError("The \"pixel_format\" parameter must either be equal to \"luminance\", \"luminance_alpha\", \"rgb\", "
                               "\"rgba\",  \"xyz\", \"xyza\". Found %s." % pf)
        cf = str(fp_.get("component_format", "float16")).lower()
        if cf not in ("float16", "float32", "uint32"):
            raise RuntimeError("The \"component_format\" parameter must either be equal to \"float16\", \"float32\", or \"uint32\". "
                               "Found %s instead." % cf)
        if ff in ("rgbe", "pfm") and not (ff == "pfm" and pf == "luminance"):
            pf = "rgb"                                                     # hdrfilm.cpp:153-176
        self._pixel_format = "luminance" if self.mono else pf                 # hdrfilm.cpp:122-128 (set_sensor files it under its sensor)
        fp_.get("high_quality_edges"); fp_.get("filename")
        rp = Props(fp_.get("rfilter", {"type": "gaussian"}), where + ".film.rfilter")
        s.rfilter_radius, s.rfilter_stddev = 0.5, 0.5
        if rp.type == "box":
            s.rfilter_type = A.RFILTER_BOX
            s.rfilter_radius = float(rp.get("radius", 0.5))
        elif rp.type == "gaussian":
            s.rfilter_type = A.RFILTER_GAUSSIAN
            s.rfilter_stddev = float(rp.get("stddev", 0.5))
        else:
            raise RuntimeError("Unknown / unsupported reconstruction filter plugin \"%s\"" % rp.type)
        rp.finish()
        fp_.finish()

    def _sampler(self, p, s, where):
        """sampler (src/librender/sensor.cpp:44-49, src/librender/sampler.cpp:11-18)"""
        sp = Props(p.get("sampler", {"type": "independent", "sample_count": 4}), where + ".sampler")
        if sp.type != "independent":
            raise RuntimeError("Unknown / unsupported sampler plugin \"%s\" (parity target is 'independent')" % sp.type)
        s.sample_count, s.sampler_seed = int(sp.get("sample_count", 4)), int(sp.get("seed", 0))
        # Extension of this backend (the reference picks the seeding by variant): "wavefront": True gives the streams of the gpu_* variants --
        # one TEA-seeded PCG32 per (pixel, sample), librender/sampler.cpp:89-92 -- instead of scalar_rgb's one stream per pixel
        s.sampler_wavefront = int(bool(sp.get("wavefront", False)))
        sp.finish()

    def _ray_target(self, p, key, s, where):
        """`ray_target` of distant, `target` of distantflux and mdistant: a shape (a dictionary) or a point"""
        s.distant_target_type = A.DISTANT_TARGET_NONE
        if not p.has(key):
            return
        target = p.get(key)
        if isinstance(target, dict):
            s.distant_target_type = A.DISTANT_TARGET_SHAPE
            s.distant_target_shape, _ = self.make_shape(target, where + "." + key, in_scene=False)
        else:
            s.distant_target_type = A.DISTANT_TARGET_POINT
            s.distant_target_point[:] = tuple(float(x) for x in np.asarray(target, dtype=np.float32))

    def _ray_origin(self, p, key, s, where):
        """`ray_origin` of distant (distant.cpp:280-289), `origin` of distantflux (distantflux.cpp:172-184): a shape the rays start from"""
        if not p.has(key):
            return
        origin = p.get(key)
        if not isinstance(origin, dict) or origin.get("type") not in SHAPE_PLUGINS:
            raise RuntimeError("Invalid parameter %s, must be a Shape." % key)
        s.distant_origin_type = 1
        s.distant_origin_shape, _ = self.make_shape(origin, where + "." + key, in_scene=False)

    def _multi_transforms(self, s, mats):
        """The sub-sensors of radiancemeter / mradiancemeter / mdistant: a (count, 4, 4) float32 array of their to_world matrices"""
        buf = np.ascontiguousarray(mats.reshape(-1), dtype=np.float32)
        self.keep.append(buf)
        s.multi_transforms = buf.ctypes.data_as(C.POINTER(C.c_float))
        s.multi_count = mats.shape[0]
        s.to_world = _xf(ScalarTransform4f())
        s.distant_target_type = A.DISTANT_TARGET_NONE

    def _perspective(self, p, s, where):
        s.type = A.SENSOR_PERSPECTIVE
        tw = p.get("to_world")
        tw = ScalarTransform4f() if tw is None else tw
        m = tw.matrix[:3, :3].astype(np.float64)
        if np.any(np.abs(m @ m.T - np.eye(3)) > 1e-3):                 # transform.h:300-312, perspective.cpp:85-86
            raise RuntimeError("Scale factors in the camera-to-world transformation are not allowed!")
        s.to_world = _xf(tw)
        s.near_clip = float(p.get("near_clip", 1e-2))
        s.far_clip = float(p.get("far_clip", 1e4))
        p.get("focus_distance")
        self._srf(p, s, where)                                         # perspective.cpp:113-121
        if s.near_clip <= 0:
            raise RuntimeError("The 'near_clip' parameter must be greater than zero!")
        if s.far_clip <= s.near_clip:
            raise RuntimeError("The 'far_clip' parameter must be greater than 'near_clip'.")
        s.fov_x = parse_fov(p, s.film_width / float(s.film_height))
        s.principal_point_offset[:] = (float(p.get("principal_point_offset_x", 0.0)), float(p.get("principal_point_offset_y", 0.0)))

    def _distant(self, p, s, where):
        s.type = A.SENSOR_DISTANT
        if p.has("direction"):                                         # distant.cpp:243-259
            if p.has("to_world"):
                raise RuntimeError("Only one of the parameters 'direction' and 'to_world'can be specified at the same time!'")
            direction = normalize32(np.asarray(p.get("direction"), dtype=np.float32))
            if p.has("orientation"):
                up = normalize32(np.cross(direction, np.asarray(p.get("orientation"), dtype=np.float32)).astype(np.float32))
            else:
                _, up = coordinate_system(direction)
            s.to_world = _xf(ScalarTransform4f.look_at([0, 0, 0], direction, up))
        else:
            s.to_world = _xf(p.get("to_world"))
        s.distant_flip_directions = int(bool(p.get("flip_directions", False)))
        self._ray_target(p, "ray_target", s, where)
        self._ray_origin(p, "ray_origin", s, where)

    def _radiancemeter(self, p, s, where):
        # src/sensors/radiancemeter.cpp:60-98: one ray along +z of to_world (or of look_at(origin, origin + direction)); it is the
        # one-sub-sensor case of mradiancemeter (same ray arithmetic, :124-127 vs mradiancemeter.cpp:150-153)
        s.type = A.SENSOR_MRADIANCEMETER
        self._srf(p, s, where)                                         # radiancemeter.cpp:61-68
        if p.has("to_world"):
            p.get("direction"); p.get("origin")
            m = p.get("to_world").matrix
        else:
            if p.has("direction") != p.has("origin"):
                raise RuntimeError("If the sensor is specified through origin and direction both values must be set!")
            if p.has("direction"):
                origin = np.asarray(p.get("origin"), dtype=np.float32)
                direction = np.asarray(p.get("direction"), dtype=np.float32)
                up, _ = coordinate_system(direction)
                m = ScalarTransform4f.look_at(origin, (origin + direction).astype(np.float32), up).matrix
            else:
                m = ScalarTransform4f().matrix
        if (s.film_width, s.film_height) != (1, 1):
            raise RuntimeError("This sensor only supports films of size 1x1 Pixels!")
        self._multi_transforms(s, np.asarray(m, dtype=np.float32).reshape(1, 4, 4))

    def _distantflux(self, p, s, where):                               # src/sensors/distantflux.cpp:60-105,141-187
        s.type = A.SENSOR_DISTANTFLUX
        tw = p.get("to_world")
        s.to_world = _xf(ScalarTransform4f() if tw is None else tw)
        self._ray_target(p, "target", s, where)
        self._ray_origin(p, "origin", s, where)

    def _sub_sensors(self, p, s, with_origins):
        """src/sensors/mradiancemeter.cpp:72-132 / src/sensors/mdistant.cpp:60-98,147-203: N sub-sensors, one per film column"""
        def tokens(key):                                                   # string::tokenize(props.string(key), " ,")
            return [t for t in str(p.get(key)).replace(",", " ").split() if t]
        dirs = tokens("directions")
        if len(dirs) % 3 != 0:
            raise RuntimeError("Invalid specification! Number of parameters %d, is not a multiple of three." % len(dirs))
        count = len(dirs) // 3
        mats = np.zeros((count, 4, 4), dtype=np.float32)
        if with_origins:
            origs = tokens("origins")
            if len(origs) % 3 != 0:
                raise RuntimeError("Invalid specification! Number of parameters %d, is not a multiple of three." % len(origs))
            if len(origs) != len(dirs):
                raise RuntimeError("Invalid specification! Number of parameters for origins and directions (%d, %d) are not equal." % (len(origs), len(dirs)))
        for i in range(count):
            direction = np.array([np.float32(x) for x in dirs[3 * i:3 * i + 3]], dtype=np.float32)    # std::stof
            if with_origins:
                origin = np.array([np.float32(x) for x in origs[3 * i:3 * i + 3]], dtype=np.float32)
                up, _ = coordinate_system(direction)                                               # mradiancemeter.cpp:109: first vector
                mats[i] = ScalarTransform4f.look_at(origin, (origin + direction).astype(np.float32), up).matrix
            else:
                _, up = coordinate_system(direction)                                               # mdistant.cpp:166-167: second vector
                mats[i] = ScalarTransform4f.look_at([0, 0, 0], direction, up).matrix
        if (s.film_width, s.film_height) != (count, 1):
            raise RuntimeError("Film size must be [sensor_count, 1]. Expected [%d, 1], got [%d, %d]" % (count, s.film_width, s.film_height))
        self._multi_transforms(s, mats)

    def _mradiancemeter(self, p, s, where):
        s.type = A.SENSOR_MRADIANCEMETER
        if p.has("to_world"):
            raise RuntimeError("This sensor is specified through a set of origin and direction values and cannot use the to_world transform.")
        self._sub_sensors(p, s, True)

    def _mdistant(self, p, s, where):
        s.type = A.SENSOR_MDISTANT
        self._sub_sensors(p, s, False)
        self._ray_target(p, "target", s, where)                         # mdistant.cpp:71-88,188-198

    def _srf(self, p, s, where):
        """"srf" of perspective / radiancemeter: the spectral response function the wavelengths are sampled from.  Outside the spectral
        variants the plugins warn and ignore it (perspective.cpp:113-121, radiancemeter.cpp:62-68)."""
        if not p.has("srf"):
            return
        v = p.get("srf")
        if not self.spectral:
            return
        if isinstance(v, dict) and v.get("type") not in ("uniform", "discrete"):
            raise RuntimeError("srf: sample_spectrum is available for 'uniform' and 'discrete' spectra in this backend (%s)" % where)
        s.srf = 1 + self._spectrum(v, where + ".srf")

    # ------------------------------------------------------------ integrator
    def set_integrator(self, d, where):
        p = Props(d, where)
        self.aov_names = []
        if p.type not in INTEGRATOR_PLUGINS:
            raise RuntimeError("Unknown / unsupported integrator plugin \"%s\"" % p.type)
        INTEGRATOR_PLUGINS[p.type](self, d, p, where)

    @staticmethod
    def _nested_integrators(d):
        """The child objects of a wrapper (nbins, bins, moment), in props.objects() order"""
        return [(k, v) for k, v in sorted_items(d) if isinstance(v, dict) and k not in ("type", "id")]

    def _wrap(self, p, name, child, where):
        """The wrapper is the SamplingIntegrator that renders (nbins.cpp / bins.cpp / moment.cpp: Base(props)): ITS block_size,
        samples_per_pass and timeout drive the render loop (integrator.cpp:29-48); of the nested integrator only sample() is used.
        Builds the nested integrator and returns its record with the wrapper's three values."""
        p.get(name)
        outer = (int(p.get("block_size", 0)), int(p.get("samples_per_pass", -1)), float(p.get("timeout", -1.0)))
        p.finish()
        self.set_integrator(child, where + "." + name)
        it = self.integrator
        it.block_size, it.samples_per_pass, it.timeout = outer
        return it

    def _bin_integrator(self, d, p, where):
        # src/integrators/nbins.cpp:55-98, bins.cpp:23-85: wavelength-bin AOVs around one nested sampling integrator
        if not self.spectral:
            raise RuntimeError("This integrator can only be used with a spectral variant!")
        nested = self._nested_integrators(d)
        for k, v in nested:
            if v.get("type") not in tuple(SAMPLING_INTEGRATORS) + ("nbins", "bins"):
                raise RuntimeError("Child objects must be of type 'SamplingIntegrator'!")
        if len(nested) > 1:
            raise RuntimeError("More than one sub-integrator specified!")
        if not nested:
            raise RuntimeError("Must specify a sub-integrator!")
        if nested[0][1].get("type") in ("nbins", "bins"):
            raise RuntimeError("nested bin integrators are not supported by this backend")
        lo, hi, names = [], [], []
        if p.type == "nbins":
            spec = p.get("wavelengths")
            if spec is None:
                raise RuntimeError("Property \"wavelengths\" has not been specified!")
            tol = float(p.get("tolerance", 1e-5))
            for tok in str(spec).replace(",", " ").split():
                try:
                    lo.append(float(tok))
                except ValueError:
                    raise RuntimeError("Could not parse floating point value '%s'" % tok)
                hi.append(tol); names += [tok, tok + "_pop"]
            mode = 1
        else:
            spec = p.get("bins")
            if spec is None:
                raise RuntimeError("Property \"bins\" has not been specified!")
            for tok in str(spec).replace(",", " ").split():
                item = tok.split(":")
                if len(item) != 3 or not all(item):
                    continue                                            # bins.cpp:47-51: warn and skip
                try:
                    lo.append(float(item[1])); hi.append(float(item[2]))
                except ValueError as e:
                    raise RuntimeError("Could not parse floating point value '%s'" % str(e).split("'")[-2])
                names += [item[0], item[0] + "_weights"]
            mode = 2
        it = self._wrap(p, nested[0][0], nested[0][1], where)
        if len(lo) > 64:
            raise RuntimeError("this backend supports at most 64 spectral bins")
        it.bin_mode, it.bin_count = mode, len(lo)
        self._bins = (np.ascontiguousarray(lo, np.float32), np.ascontiguousarray(hi, np.float32))
        self.keep += list(self._bins)
        it.bin_lo = self._bins[0].ctypes.data_as(A.fp); it.bin_hi = self._bins[1].ctypes.data_as(A.fp)
        self.aov_names = names

    def _moment(self, d, p, where):
        # src/integrators/moment.cpp:27-58: six AOV channels around one nested sampling integrator -- its result as XYZ and the square
        if self.spectral:
            raise RuntimeError("the moment integrator is not supported in the spectral variant by this backend")
        nested = self._nested_integrators(d)
        if not nested:
            raise RuntimeError("moment: must specify a nested integrator")
        if len(nested) > 1:
            raise RuntimeError("moment: more than one nested integrator (%s) is not supported by this backend" % ", ".join(k for k, _ in nested))
        name, child = nested[0]
        if child.get("type") not in SAMPLING_INTEGRATORS:
            raise RuntimeError("moment: the nested integrator \"%s\" must be one of path, volpath, volpathmis, not \"%s\"" % (name, child.get("type")))
        self._wrap(p, name, child, where).moment = 1
        self.aov_names = [name + c for c in (".X", ".Y", ".Z")] + ["m2_" + name + c for c in (".X", ".Y", ".Z")]       # moment.cpp:43-52

    def _sampling_integrator(self, d, p, where):
        it = A.Integrator()
        it.type = SAMPLING_INTEGRATORS[p.type]
        it.use_spectral_mis = int(bool(p.get("use_spectral_mis", True))) if p.type == "volpathmis" else 1
        it.max_depth = int(p.get("max_depth", -1))
        it.rr_depth = int(p.get("rr_depth", 5))
        it.hide_emitters = int(bool(p.get("hide_emitters", False)))
        it.block_size = int(p.get("block_size", 0))
        it.samples_per_pass = int(p.get("samples_per_pass", -1))
        it.timeout = float(p.get("timeout", -1.0))
        if it.rr_depth <= 0:
            raise RuntimeError("\"rr_depth\" must be set to a value greater than zero!")
        if it.max_depth < 0 and it.max_depth != -1:
            raise RuntimeError("\"max_depth\" must be set to -1 (infinite) or a value >= 0")
        p.finish()
        self.integrator = it

    # ------------------------------------------------------------ scene
    def load(self, d):
        if not isinstance(d, dict) or d.get("type") != "scene":
            raise RuntimeError("load_dict(): the top-level dictionary must have type 'scene' in this backend")
        for k, v in sorted_items(d):          # scene.cpp:23: props.objects() order
            if k in ("type", "id"):
                continue
            if not isinstance(v, dict):
                raise RuntimeError("Unexpected property \"%s\" at the scene level" % k)
            t = v.get("type")
            if t == "ref":
                raise RuntimeError("Reference found at the scene level: %s" % k)
            name = v.get("id", k)                                       # scene.cpp:237-244: a child goes by its id; here a key is one
            if t in SHAPE_PLUGINS:
                self.children.append((name, ("shape", self.add_shape(v, k))))
            elif t == "shapegroup":
                self.children.append((name, ("shape", self.add_shapegroup(v, k))))
            elif t == "instance":
                self.children.append((name, ("shape", self.add_instance(v, k))))
            elif t in ("directional", "constant", "area", "point"):
                self.children.append((name, ("emitter", self.add_emitter(v, k))))
            elif t in SENSOR_PLUGINS:
                self.set_sensor(v, k)                                    # scene.cpp:41-60: any number; the first one visited is sensor 0
            elif t in INTEGRATOR_PLUGINS:
                if self.integrator is not None:
                    raise RuntimeError("Only one integrator can be specified per scene.")
                self.set_integrator(v, k)
            elif t in BSDF_PLUGINS:
                self.children.append((name, ("bsdf", self.add_bsdf(v, k))))
            elif t in ("homogeneous", "heterogeneous"):
                self.children.append((name, ("medium", self.add_medium(v, k))))
            elif t in ("isotropic", "hg", "rayleigh", "tabphase", "blendphase"):
                self.children.append((name, ("phase", self.add_phase(v, k))))
            elif t in ("gridvolume", "constvolume"):
                self.children.append((name, ("volume", self.add_volume(v, k))))
            elif t in TEXTURE_PLUGINS:                                   # declared at the scene level, referenced by id from BSDFs
                self.children.append((name, ("texture", self.add_texture(v, k))))
            else:
                raise RuntimeError("Unknown / unsupported plugin \"%s\" (key \"%s\")" % (t, k))
        if self.sensor is None:
            raise RuntimeError("No sensors found! (this backend does not instantiate a default camera)")
        if self.integrator is None:
            self.set_integrator({"type": "path"}, "integrator")          # scene.cpp:88-92
        if self.textures and self.integrator.moment:
            raise RuntimeError("Textures inside a moment integrator's scene are not supported by this backend")
        if self.blends and self.integrator.moment:
            raise RuntimeError("\"blendbsdf\" (%s) inside a moment integrator's scene is not supported by this backend" % ", ".join(self.blends))
        if (self.groups or self.instanced) and self.integrator.moment:
            raise RuntimeError("\"shapegroup\" / \"instance\" (%s) inside a moment integrator's scene is not supported by this backend" % ", ".join(self.groups + self.instanced))
        if (self.groups or self.instanced) and self.spectral:
            raise RuntimeError("\"shapegroup\" / \"instance\" (%s) is not supported in the gpu_spectral variant" % ", ".join(self.groups + self.instanced))
        if self.cones and self.integrator.moment:
            raise RuntimeError("\"cone\" (%s) inside a moment integrator's scene is not supported by this backend" % ", ".join(self.cones))
        if self.cones and self.spectral:
            raise RuntimeError("\"cone\" (%s) is not supported in the gpu_spectral variant" % ", ".join(self.cones))
        if self.twosided and self.integrator.moment:
            raise RuntimeError("\"twosided\" (%s) inside a moment integrator's scene is not supported by this backend" % ", ".join(self.twosided))
        if self.specular and self.integrator.moment:
            raise RuntimeError("\"dielectric\" / \"conductor\" (%s) inside a moment integrator's scene is not supported by this backend" % ", ".join(self.specular))
        return self.finish()

    def finish(self):
        desc = A.SceneDesc()
        desc.abi_version = A.MTS_ABI_VERSION

        def arr(cls, items):
            a = (cls * max(len(items), 1))(*items)
            self.keep.append(a)
            return a
        desc.volumes, desc.volume_count = arr(A.Volume, self.volumes), len(self.volumes)
        desc.phases, desc.phase_count = arr(A.Phase, self.phases), len(self.phases)
        desc.media, desc.medium_count = arr(A.Medium, self.media), len(self.media)
        desc.bsdfs, desc.bsdf_count = arr(A.Bsdf, self.bsdfs), len(self.bsdfs)
        desc.shapes, desc.shape_count = arr(A.Shape, self.shapes), len(self.shapes)
        desc.emitters, desc.emitter_count = arr(A.Emitter, self.emitters), len(self.emitters)
        desc.sensor = self.sensor
        desc.integrator = self.integrator
        desc.integrator.monochrome, desc.integrator.spectral = int(self.mono), int(self.spectral)
        desc.spectra, desc.spectrum_count = arr(A.Spectrum, self.spectra), len(self.spectra)
        if self.textures:                                                # a scene without textures keeps the zeroed tail
            desc.textures, desc.texture_count = arr(A.Texture, self.textures), len(self.textures)
            desc.bsdf_textures = arr(A.i32, [t for row in self.bsdf_textures for t in row])
        self.keep.append(desc)
        return desc


# plugin name -> the SceneBuilder method that builds it: what load() accepts and what set_sensor / set_integrator dispatch through
SENSOR_PLUGINS = {"perspective": SceneBuilder._perspective, "distant": SceneBuilder._distant, "radiancemeter": SceneBuilder._radiancemeter,
                  "distantflux": SceneBuilder._distantflux, "mradiancemeter": SceneBuilder._mradiancemeter, "mdistant": SceneBuilder._mdistant}
INTEGRATOR_PLUGINS = dict({name: SceneBuilder._sampling_integrator for name in SAMPLING_INTEGRATORS},
                          nbins=SceneBuilder._bin_integrator, bins=SceneBuilder._bin_integrator, moment=SceneBuilder._moment)


def build_scene_desc(d, mono=False, spectral=False):
    """Returns (SceneDesc, keepalive). The keepalive object owns every buffer the description points to.
    mono: build the scene with the semantics of the *_mono variants; spectral: with those of scalar_spectral."""
    b = SceneBuilder(mono, spectral)
    return b.load(d), b
