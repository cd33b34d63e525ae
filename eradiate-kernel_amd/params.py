"""traverse(scene) / ParameterMap: read and change the parameters of a loaded scene in place.

Mirrors /root/reference/src/python/python/util.py:14-190.  The reference walks the scene graph through every plugin's `traverse()`
and, on `update()`, calls `parameters_changed()` on the touched objects and their parents.  Here the graph was written down by the
SceneBuilder while it built the description (scene_dict.py: `nodes`, `children`); `update()` converts the assigned values with the
helpers `load_dict` uses, writes them into the description -- which then is the description a fresh `load_dict` of the edited
dictionary would produce -- and hands the dirty records to `mts_scene_update` in ONE call (include/mtsamd.h).

Keys are the reference's: a scene-level child goes by its id or dictionary key (scene.cpp:237-244), everything below by the names
the plugins give (`atmosphere.interior_medium.sigma_t.data`, `ground.bsdf.rho_0.value`, `sun.irradiance.value`); an object that is
referenced twice appears once, under the first name it was reached by (`put_object` skips known nodes), and clashing names get the
suffixes `_1`, `_2`, ...  Differences: a medium's phase function is listed (as `phase_function`, upstream Mitsuba's name; this
fork's Medium::traverse leaves it out); `gridvolume_spectral` data can be updated (gridvolume_spectral.cpp:396-398 leaves
parameters_changed unimplemented); a `d65` spectrum and a shape's default BSDF have no record of their own and are not listed; the
sensor, the film and the integrator are not listed, and geometry (`to_world`, mesh buffers) is listed read-only.

Arrays: the map keeps one live array per record (SceneBuilder.grids / tabs / spectrum_arrays); the array an update replaces is dropped.
A grid assigned as a device tensor leaves the description without a host copy (`data` = NULL: a stale array cannot be taken for the
scene's contents), reads back as that tensor, and goes down again on `set_dirty()`.  A device tensor for a colour grid of a *_mono
scene is refused: the grid's majorant is the colour maximum, which its luminance does not tell.
"""
import ctypes as C

import numpy as np

from . import _capi as A
from . import scene_dict as SD

_OBJ = {"spectrum": A.OBJ_SPECTRUM, "volume": A.OBJ_VOLUME, "phase": A.OBJ_PHASE, "medium": A.OBJ_MEDIUM, "bsdf": A.OBJ_BSDF, "emitter": A.OBJ_EMITTER, "texture": A.OBJ_TEXTURE}
_ARRAYS = {"spectrum": "spectra", "volume": "volumes", "phase": "phases", "medium": "media", "bsdf": "bsdfs", "emitter": "emitters", "shape": "shapes", "texture": "textures"}
_ABSENT = object()
_GEOMETRY = "geometry updates are not supported yet (shapes are uploaded once: no BVH refit)"


def _is_tensor(v):
    return type(v).__module__.split(".")[0] == "torch" and hasattr(v, "data_ptr")


class _Param:
    """One key: where its value lives in the description and how an assigned value gets there."""

    def __init__(self, kind, index, what, field, where="", emitter=False):
        self.kind, self.index, self.what, self.field, self.where, self.emitter = kind, index, what, field, where, emitter

    @property
    def readonly(self):
        if self.what == "geometry":
            return _GEOMETRY
        if self.what in ("size", "lambda", "resolution", "to_uv"):
            return "the parameter is read-only"
        return None


def _collect(keep):
    """The reference's SceneTraversal (util.py:149-188) over the builder's notes: {key: _Param}, in traversal order."""
    params, seen, prefixes, named = {}, set(), set(), {}

    def unique(name):
        base, ctr = name, 1
        while name in prefixes:
            name = "%s_%i" % (base, ctr)
            ctr += 1
        prefixes.add(name)
        return name

    def visit(node, name):
        if node in seen:
            return
        seen.add(node)
        name = unique(name)
        named[node] = name
        if node[0] == "colour":                                 # srgb.cpp:59-61 / srgb_d65.cpp:63-65
            params[name + ".value"] = _Param(node[1], node[2], "rgb", node[3], node[4], node[5])
            return
        if node[0] == "uniform":                                # uniform.cpp:108-112 in the rgb / mono variants: a blendbsdf's constant weight
            params[name + ".value"] = _Param(node[1], node[2], "weight", node[3], node[4])
            return
        if node[0] == "spectrum":
            plugin = keep.spectrum_plugins[node[1]]
            if plugin == "uniform":                             # uniform.cpp:108-112
                params[name + ".value"] = _Param("spectrum", node[1], "float", "value")
                params[name + ".lambda_min"] = _Param("spectrum", node[1], "lambda", "lambda_min")
                params[name + ".lambda_max"] = _Param("spectrum", node[1], "lambda", "lambda_max")
            elif plugin == "regular":                           # regular.cpp:59-62
                params[name + ".range"] = _Param("spectrum", node[1], "range", None)
                params[name + ".values"] = _Param("spectrum", node[1], "values", "values")
            elif plugin == "irregular":                         # irregular.cpp:67-70
                params[name + ".wavelengths"] = _Param("spectrum", node[1], "values", "wavelengths")
                params[name + ".values"] = _Param("spectrum", node[1], "values", "values")
            return
        for entry in keep.nodes.get(node, []):
            if entry[0] == "param":
                params[name + "." + entry[1]] = _Param(node[0], node[1], entry[2], entry[3])
            elif entry[0] == "alias":                           # twosided.cpp:183-186 with one child: brdf_1 is brdf_0, whose keys it repeats
                src = name + ".brdf_0"
                if named.get(entry[2]) == src:                  # (listed elsewhere before, a shared object: under neither name, as ever)
                    dst = unique(name + "." + entry[1])
                    for k in [k for k in params if k.startswith(src + ".")]:
                        params[dst + k[len(src):]] = params[k]
            else:
                visit(entry[2], name + "." + entry[1])

    for key, node in keep.children:
        visit(node, key)
    return params


class ParameterMap:
    """Dictionary-like view of a scene's parameters (util.py:14-138): read with `params[key]`, assign, then `update()`."""

    def __init__(self, desc, keep, scene=None):
        """Private constructor (use traverse()).  Without a `scene` the map works on the description alone: update() then only
        rewrites `desc` (what the CPU restatement and the tests of the key logic use)."""
        self._desc, self._keep, self._scene = desc, keep, scene
        self.properties = _collect(keep)
        self.update_list = {}                                   # key -> assigned value (None: marked by set_dirty alone)

    # ---- dictionary surface
    def __contains__(self, key):
        return key in self.properties

    def __len__(self):
        return len(self.properties)

    def keys(self):
        return self.properties.keys()

    def items(self):
        return ((k, self[k]) for k in self.keys())

    def __delitem__(self, key):
        del self.properties[key]

    def __repr__(self):
        return "ParameterMap[\n%s]" % "".join("    %s,\n" % k for k in self.keys())

    def keep(self, keys):
        """Only keep the elements whose keys are in `keys` (util.py:129-137)."""
        keys = set(keys)
        self.properties = {k: v for k, v in self.properties.items() if k in keys}

    def _record(self, p):
        return getattr(self._desc, _ARRAYS[p.kind])[p.index]

    def __getitem__(self, key):
        if key in self.update_list and self.update_list[key] is not None:
            return self.update_list[key]                        # assigned, not yet applied
        p = self.properties[key]
        rec = self._record(p)
        if p.what == "grid":
            return self._keep.grids[p.index]
        if p.what == "size":
            return (rec.nx, rec.ny, rec.nz)
        if p.what == "tab":
            return self._keep.tabs[p.index]
        if p.what == "texels":                                  # bitmap.cpp:562: the (height, width, channels) array
            return self._keep.bitmaps[p.index]
        if p.what == "resolution":
            return (rec.width, rec.height)
        if p.what == "to_uv":
            return np.array(list(rec.to_uv), np.float32).reshape(3, 3)
        if p.what == "rgb":
            return np.array(list(getattr(rec, p.field.split("+")[0])), np.float32)
        if p.what in ("weight", "eta"):                         # a float the record holds three times
            return getattr(rec, p.field)[0]
        if p.what == "range":
            return (rec.lambda_min, rec.lambda_max)
        if p.what == "values":
            return np.ctypeslib.as_array(getattr(rec, p.field), shape=(rec.count,)).copy()
        if p.what == "geometry":
            v = getattr(rec, p.field)
            if p.field == "to_world":
                return np.array(list(v.matrix), np.float32).reshape(4, 4)
            if isinstance(v, int):
                return v
            n = {"faces": 3 * rec.face_count, "vertex_texcoords": 2 * rec.vertex_count}.get(p.field, 3 * rec.vertex_count)
            return np.ctypeslib.as_array(v, shape=(n,)).copy()
        return getattr(rec, p.field)                            # float, lambda

    def __setitem__(self, key, value):
        """Marks and stores; nothing is converted or written before update()."""
        p = self.properties[key]
        if p.readonly:
            raise RuntimeError("ParameterMap: cannot assign to \"%s\": %s" % (key, p.readonly))
        self.update_list[key] = value

    def set_dirty(self, key):
        """Marks a parameter as changed without assigning (util.py:92-113): update() re-derives what depends on its current value."""
        p = self.properties[key]
        if p.readonly:
            raise RuntimeError("ParameterMap: cannot mark \"%s\": %s" % (key, p.readonly))
        self.update_list.setdefault(key, None)
        return p

    # ---- update
    def _convert(self, key, p, value):
        """The assigned value as the description holds it: through the helpers load_dict uses.  Returns (what to store, device pointer)."""
        rec = self._record(p)
        if p.what == "grid":
            if _is_tensor(value):
                if value.is_cuda:
                    if self._scene is None:
                        raise RuntimeError("\"%s\": a device tensor needs a scene in device memory" % key)
                    if self._keep.grid_mono_max.get(p.index):
                        # loaded from a colour grid under a *_mono variant: the description holds its luminance, with the COLOUR grid's
                        # maximum as the majorant (grid3d.cpp:157-160).  A device tensor can only carry the luminance, so the majorant
                        # could not follow: too small a majorant biases the render silently
                        raise RuntimeError("\"%s\": a device tensor cannot update a colour grid under %s: the grid's majorant is the maximum of the "
                                           "colour channels, which the luminance on the device does not tell; assign the (nz, ny, nx, 3) host array"
                                           % (key, "gpu_mono"))
                    want = rec.nz * rec.ny * rec.nx * rec.channels
                    dev = value.device.index if value.device.index is not None else 0
                    if dev != self._scene._device:
                        raise RuntimeError("\"%s\": the tensor lives on device %d, the scene on device %d" % (key, dev, self._scene._device))
                    if str(value.dtype) != "torch.float32":
                        raise RuntimeError("\"%s\": a device tensor must be float32, got %s" % (key, value.dtype))
                    if not value.is_contiguous():
                        raise RuntimeError("\"%s\": a device tensor must be contiguous" % key)
                    if value.numel() != want:
                        raise RuntimeError("\"%s\": the grid holds %d values (nz, ny, nx, channels = %d, %d, %d, %d), the tensor %d"
                                           % (key, want, rec.nz, rec.ny, rec.nx, rec.channels, value.numel()))
                    return value, int(value.data_ptr())
                value = value.detach().numpy()
            data, mono_max = self._keep._grid_data(value)
            if data.shape != (rec.nz, rec.ny, rec.nx, rec.channels):
                raise RuntimeError("\"%s\": 'size' / 'channels' cannot change: the grid is (nz, ny, nx, channels) = %s, got %s"
                                   % (key, (rec.nz, rec.ny, rec.nx, rec.channels), data.shape))
            return (data, mono_max), None
        if p.what == "texels":
            data = self._keep._bitmap_data(value)
            if data.shape != (rec.height, rec.width, rec.channels):
                raise RuntimeError("\"%s\": 'resolution' / 'channels' differ from what the scene was created with (the topology of a scene is frozen): "
                                   "the bitmap is (height, width, channels) = %s, got %s" % (key, (rec.height, rec.width, rec.channels), data.shape))
            return data, None
        if p.what == "tab":
            arr = SD._tab_values(value) if isinstance(value, str) else np.ascontiguousarray(np.asarray(value, np.float32).reshape(-1))
            if arr.size != rec.tab_count:
                raise RuntimeError("\"%s\": the table length ('tab_count') cannot change: %d entries, got %d" % (key, rec.tab_count, arr.size))
            return arr, None
        if p.what == "rgb":
            return self._keep._color(value, p.where, emitter=p.emitter), None
        if p.what == "weight":
            return (SD._weight(value, p.where),) * 3, None
        if p.what == "eta":                                     # dielectric.cpp:323: the relative index of refraction, a plain float
            return (float(value),) * 3, None
        if p.what == "range":
            lo, hi = (float(x) for x in value)
            return (lo, hi), None
        if p.what == "values":
            arr = np.ascontiguousarray(np.asarray(value, np.float32).reshape(-1))
            if arr.size != rec.count:
                raise RuntimeError("\"%s\": the number of entries ('count') cannot change: %d, got %d" % (key, rec.count, arr.size))
            return arr, None
        return float(value), None

    def update(self):
        """Applies every assignment since the last update: the description is rewritten in place and the device scene follows in one
        mts_scene_update.  A refused update raises and leaves description and scene as they were."""
        if self._scene is not None and not getattr(self._scene, "_handle", None):
            raise RuntimeError("ParameterMap.update(): the scene was destroyed")
        pending, self.update_list = self.update_list, {}
        if not pending:
            return
        keep, desc = self._keep, self._desc
        # a grid marked by set_dirty alone whose data lives in a device tensor (the description no longer points at host data)
        # goes down as that tensor again
        pending = {k: (keep.grids[self.properties[k].index] if v is None and self.properties[k].what == "grid"
                       and _is_tensor(keep.grids[self.properties[k].index]) else v) for k, v in pending.items()}
        new = {k: (self._convert(k, self.properties[k], v) if v is not None else None) for k, v in pending.items()}
        undo, dirty, alive = [], {}, []

        def put(rec, field, value):
            old = getattr(rec, field)
            if isinstance(old, C.Array):
                undo.append((rec, field, list(old)))
                getattr(rec, field)[:] = value
            else:
                if isinstance(old, C._Pointer):                 # a pointer read from a struct aliases the field: keep the address
                    old = C.cast(C.cast(old, C.c_void_p).value, type(old))
                undo.append((rec, field, old))
                setattr(rec, field, value)

        def remember(table, index):                             # the builder's side tables roll back with the description
            old = table[index]
            undo.append((table, index, old))

        for key, conv in new.items():
            p = self.properties[key]
            rec = self._record(p)
            dirty.setdefault((p.kind, p.index), None)
            if conv is None:
                continue
            value, device = conv
            if p.what == "grid":
                remember(keep.grids, p.index)
                if device is not None:
                    dirty[(p.kind, p.index)] = device
                    alive.append(value)
                    keep.grids[p.index] = value                  # (what params[key] reads; the scene has its own copy)
                    put(rec, "data", A.fp())                     # the description holds no host copy of this grid any more: NULL, so
                                                                 # nothing can take a stale array for the scene's data ("missing data")
                else:
                    data, mono_max = value
                    keep.grids[p.index] = data                   # one live array per record: the one it replaces goes with the undo list
                    put(rec, "data", data.ctypes.data_as(A.fp))
                    if mono_max is not None and keep.grid_mono_max.get(p.index):
                        put(rec, "max_value", mono_max)
            elif p.what == "texels":
                remember(keep.bitmaps, p.index)
                keep.bitmaps[p.index] = value
                put(rec, "data", value.ctypes.data_as(A.fp))
            elif p.what == "tab":
                remember(keep.tabs, p.index)
                keep.tabs[p.index] = value
                put(rec, "tab_values", value.ctypes.data_as(A.fp))
            elif p.what == "rgb":
                for field in p.field.split("+"):
                    put(rec, field, value)
            elif p.what == "range":
                put(rec, "lambda_min", value[0])
                put(rec, "lambda_max", value[1])
            elif p.what == "values":
                if (p.index, p.field) in keep.spectrum_arrays:
                    remember(keep.spectrum_arrays, (p.index, p.field))
                else:
                    undo.append((keep.spectrum_arrays, (p.index, p.field), _ABSENT))
                keep.spectrum_arrays[(p.index, p.field)] = value
                put(rec, p.field, value.ctypes.data_as(A.fp))
            else:
                put(rec, p.field, value)
        try:
            if self._scene is not None:
                recs = (A.Dirty * len(dirty))()
                for r, ((kind, index), device) in zip(recs, dirty.items()):
                    r.object, r.index, r.device_data = _OBJ[kind], index, device
                stream = None
                if alive:                                       # ordered after the tensors' producer
                    import torch
                    stream = torch.cuda.current_stream(self._scene._device).cuda_stream
                A.check(A.lib().mts_scene_update(self._scene._handle, C.byref(desc), recs, len(recs), C.c_void_p(stream)))
            else:
                self._check_host()
        except Exception:
            for target, field, old in reversed(undo):
                if isinstance(target, dict):
                    if old is _ABSENT:
                        target.pop(field, None)
                    else:
                        target[field] = old
                elif isinstance(old, list):
                    getattr(target, field)[:] = old
                else:
                    setattr(target, field, old)
            raise
        del alive                                               # the tensors were kept alive until the call returned

    def _check_host(self):
        """A map without a device scene still refuses what mts_scene_create would: the library validates the rewritten description
        (host only; mts_debug_scene_traits builds and drops the host scene)."""
        traits = C.c_int32()
        A.check(A.lib().mts_debug_scene_traits(C.byref(self._desc), C.byref(traits)))


def traverse(scene):
    """mitsuba.python.util.traverse(scene) (util.py:140-190)."""
    return ParameterMap(scene._desc, scene._keep, scene)
