"""ctypes binding of the C++ host layer (libuvrt_host.so: Mesh / BVH / RayTracer mirrors of
the reference's classes).  Method and field names are the reference's (raytracer.h:13-59)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libuvrt_host.so")
_LIB = None

NODE_DT = np.dtype([("minx", "<f4"), ("miny", "<f4"), ("minz", "<f4"), ("leftFirst", "<i4"),
                    ("maxx", "<f4"), ("maxy", "<f4"), ("maxz", "<f4"), ("triCount", "<i4")])

# RouteLaunch (host/raytracer.h): one launch of an iteration of a route; kind is capi.LAUNCH_STOP / capi.LAUNCH_SWEEP
ROUTE_LAUNCH_DT = np.dtype([("from", "<f4", 3), ("to", "<f4", 3), ("duration", "<f4"), ("kind", "<i4"), ("column", "<i4"),
                            ("reserved", "<i4")])

VIEW_DOSAGE, VIEW_MAXPOWER, VIEW_TEXTURE = 0, 1, 2

_vp = C.c_void_p
SYMBOLS = [
    ("uvrt_host_mesh_load", _vp, [C.c_char_p]),
    ("uvrt_host_mesh_from_tris", _vp, [_vp, C.c_int]),
    ("uvrt_host_mesh_free", None, [_vp]),
    ("uvrt_host_mesh_tri_count", C.c_int, [_vp]),
    ("uvrt_host_mesh_floor_height", C.c_float, [_vp]),
    ("uvrt_host_mesh_tris", _vp, [_vp]),
    ("uvrt_host_mesh_nodes", _vp, [_vp]),
    ("uvrt_host_mesh_nodes_used", C.c_uint, [_vp]),
    ("uvrt_host_mesh_tri_idx", _vp, [_vp]),
    ("uvrt_host_mesh_rebuild_bvh", None, [_vp]),
    ("uvrt_host_rt_new", _vp, []),
    ("uvrt_host_rt_free", None, [_vp]),
    ("uvrt_host_rt_set_route_dir", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_set_default_route", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_set_device", None, [_vp, C.c_int]),
    ("uvrt_host_rt_set_auto_save", None, [_vp, C.c_int]),
    ("uvrt_host_rt_init", None, [_vp, _vp]),
    ("uvrt_host_rt_load_route", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_save_route", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_update_photons_per_light", None, [_vp]),
    ("uvrt_host_rt_reset_dosage_map", None, [_vp]),
    ("uvrt_host_rt_clear_buffers", None, [_vp, C.c_int]),
    ("uvrt_host_rt_compute_dosage_map", None, [_vp]),
    ("uvrt_host_rt_compute_single", None, [_vp, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    ("uvrt_host_rt_compute_segment", None, [_vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    ("uvrt_host_rt_compute_segments", None, [_vp]),
    ("uvrt_host_rt_shade", None, [_vp]),
    ("uvrt_host_rt_add_lamp", None, [_vp]),
    ("uvrt_host_rt_calibrate", None, [_vp, C.c_float, C.c_float, C.c_float]),
    ("uvrt_host_rt_sync", None, [_vp]),
    ("uvrt_host_rt_read_dosage", None, [_vp, _vp, C.c_int, C.c_int]),
    ("uvrt_host_rt_ctx", _vp, [_vp]),
    ("uvrt_host_rt_set_shard", None, [_vp, C.c_int, C.c_int]),
    ("uvrt_host_rt_compute_batched", None, [_vp, C.c_int]),
    ("uvrt_host_rt_compute_batched_group", None, [C.POINTER(_vp), C.c_int, C.c_int]),
    ("uvrt_host_rt_set_ray_range", None, [_vp, C.c_int, C.c_int]),
    ("uvrt_host_rt_set_reduce_over_comm", None, [_vp, C.c_int]),
    ("uvrt_host_rt_lamp_count", C.c_int, [_vp]),
    ("uvrt_host_rt_get_lamp", None, [_vp, C.c_int, C.POINTER(C.c_float)]),
    ("uvrt_host_rt_set_lamps", None, [_vp, C.POINTER(C.c_float), C.c_int]),
    ("uvrt_host_plan_options_init", None, [_vp]),
    ("uvrt_host_plan_options_layout", C.c_int, [C.POINTER(C.c_int), C.c_int]),
    ("uvrt_host_rt_plan", None, [_vp, _vp, _vp, C.POINTER(C.c_uint)]),
    ("uvrt_host_rt_set_gather_refine", None, [_vp, C.c_double, C.c_int]),
    ("uvrt_host_rt_set_reflect_map", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_get_reflect_map", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_set_reflectance_map", None, [_vp, _vp, C.c_int]),
    ("uvrt_host_rt_reflectance_map", C.c_int, [_vp, _vp, C.c_int]),
    ("uvrt_host_rt_has_reflect_map", C.c_int, [_vp]),
    ("uvrt_host_rt_prepare_reflect_map", C.c_int, [_vp, C.c_float, C.c_char_p, C.c_int]),
    ("uvrt_host_reflect_rules", C.c_int, [C.c_char_p, _vp, C.c_int, C.c_float, _vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_set_mirror_map", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_get_mirror_map", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_set_mirrors", None, [_vp, _vp, C.c_int, _vp, C.c_int]),
    ("uvrt_host_rt_has_mirrors", C.c_int, [_vp]),
    ("uvrt_host_rt_prepare_mirror_map", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("uvrt_host_mirror_rules", C.c_int, [C.c_char_p, _vp, C.c_int, _vp, C.POINTER(C.c_int), _vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_set_sensor_map", None, [_vp, C.c_char_p]),
    ("uvrt_host_rt_get_sensor_map", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_set_sensors", None, [_vp, _vp, C.c_int]),
    ("uvrt_host_rt_has_sensors", C.c_int, [_vp]),
    ("uvrt_host_rt_prepare_sensor_map", C.c_int, [_vp, C.c_char_p, C.c_int]),
    ("uvrt_host_rt_active_sensors", C.c_int, [_vp, _vp, C.c_int]),
    ("uvrt_host_rt_read_sensors", C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    ("uvrt_host_rt_calibrate_at_sensor", None, [_vp, C.c_float, C.c_int, C.c_int]),
    ("uvrt_host_sensor_rules", C.c_int, [C.c_char_p, _vp, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    ("uvrt_host_rt_plan_group", None, [C.POINTER(_vp), C.c_int, _vp, _vp, C.POINTER(C.c_uint)]),
    ("uvrt_host_rt_plan_bounds", None, [_vp, _vp]),
    ("uvrt_host_rt_plan_segments", C.c_int, [_vp, C.POINTER(C.c_float), C.c_int]),
    ("uvrt_host_rt_end_plan", None, [_vp]),
    ("uvrt_host_rt_set_candidate_grid", None, [_vp, C.c_int, C.c_int, C.c_float]),
    ("uvrt_host_grid_positions", None, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float,
                                        C.POINTER(C.c_float)]),
    ("uvrt_host_route_launches", C.c_int, [_vp, C.c_int, C.c_float, C.c_float, _vp, C.c_int]),
    ("uvrt_host_rt_get", C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    ("uvrt_host_rt_set", C.c_int, [_vp, C.c_char_p, C.c_double]),
]

_FIELDS = {"lightLength", "lightHeight", "maxPhotonCount", "photonCount", "maxIterations",
           "currIterations", "lightIntensity", "minDosage", "minPower", "photonsPerLight", "compTime",
           "progress", "finishedComputation", "thresholdView", "startedComputation", "calibratedPower",
           "photonMapSize", "viewMode", "driveSpeed", "gatherSamples", "gatherSampling", "gatherRelError",
           "gatherMaxExtra", "reflectance", "reflectSamples", "reflectBounces", "gatherBatch", "reflectSided",
           "sensorSamples", "sensorLaunches"}
_INT_FIELDS = {"maxPhotonCount", "photonCount", "maxIterations", "currIterations", "photonsPerLight",
               "photonMapSize", "viewMode", "gatherSamples", "gatherSampling", "gatherMaxExtra",
               "reflectSamples", "reflectBounces", "gatherBatch", "reflectSided", "sensorSamples", "sensorLaunches"}
_BOOL_FIELDS = {"finishedComputation", "thresholdView", "startedComputation"}



class PlanOptions(C.Structure):
    """uvrt_host_plan_options (host/host_capi.cpp), the plain mirror of RayTracer::PlanOptions that uvrt_host_rt_plan and
    uvrt_host_rt_plan_group take.  A new one holds the defaults of RayTracer::PlanOptions{} (uvrt_host_plan_options_init);
    keyword arguments set fields."""
    _fields_ = [("min_dose", C.c_float), ("min_photons", C.c_int), ("margin", C.c_double), ("rel_gap", C.c_double),
                ("max_iterations", C.c_int), ("mask", _vp), ("gather_samples", C.c_int), ("gather_sampling", C.c_int),
                ("gather_confidence", C.c_double), ("gather_rel_error", C.c_double), ("gather_max_extra", C.c_int),
                ("reflectance", C.c_float), ("reflect_samples", C.c_int), ("reflect_bounces", C.c_int),
                ("reflect_sided", C.c_int), ("reflect_mapped", C.c_int), ("mirror_mapped", C.c_int), ("gather_batch", C.c_int)]

    def __init__(self, **fields):
        super().__init__()
        lib().uvrt_host_plan_options_init(C.byref(self))
        for name, value in fields.items():
            setattr(self, name, value)


def lib():
    global _LIB
    if _LIB is None:
        capi.lib()   # the device library first: fails loudly when the HIP extension is missing
        if not os.path.exists(LIB_PATH):
            raise capi.UvrtError("host library missing: %s (run __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def parse_reflect_rules(path, tris, base):
    """RayTracer::ParseReflectRules: the rules file `path` over the 64-byte Tri records `tris` (centroids filled, as a Mesh or
    a BVH build leaves them) into rho float32[2][T], every entry starting at `base`.  Host only: no GPU is touched.  A line
    that cannot be read raises ValueError("FILE:LINE: reason")."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    out = np.empty((2, t.shape[0]), dtype=np.float32)
    err = C.create_string_buffer(1024)
    if lib().uvrt_host_reflect_rules(os.fsencode(path), t.ctypes.data_as(_vp), t.shape[0], float(np.float32(base)),
                                     out.ctypes.data_as(_vp), err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return out


def parse_mirror_rules(path, tris):
    """RayTracer::ParseMirrorRules: the rules file `path` over the 64-byte Tri records `tris` (centroids filled) into (panels
    capi.MIRROR_DT[count], panel_of_tri uint8[T]: 0 or k + 1).  Host only: no GPU is touched.  A line that cannot be read raises
    ValueError("FILE:LINE: reason")."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    panels = np.zeros(capi.MIRROR_MAX, dtype=capi.MIRROR_DT)
    members = np.zeros(t.shape[0], dtype=np.uint8)
    count = C.c_int(0)
    err = C.create_string_buffer(1024)
    if lib().uvrt_host_mirror_rules(os.fsencode(path), t.ctypes.data_as(_vp), t.shape[0], panels.ctypes.data_as(_vp),
                                    C.byref(count), members.ctypes.data_as(_vp), err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    return panels[:count.value].copy(), members


def parse_sensor_rules(path):
    """RayTracer::ParseSensorRules: the rules file `path` into capi.SENSOR_DT[count], in file order (a grid's cell centres x
    fastest, then y, then z).  Host only: no GPU is touched.  A line that cannot be read raises ValueError("FILE:LINE: reason")."""
    count = C.c_int(0)
    err = C.create_string_buffer(1024)
    if lib().uvrt_host_sensor_rules(os.fsencode(path), None, 0, C.byref(count), err, len(err)) != 0:
        raise ValueError(err.value.decode(errors="replace"))
    out = np.zeros(max(count.value, 1), dtype=capi.SENSOR_DT)
    lib().uvrt_host_sensor_rules(os.fsencode(path), out.ctypes.data_as(_vp), count.value, C.byref(count), err, len(err))
    return out[:count.value].copy()


class Mesh:
    """Tmpl8::Mesh: GLB -> Tri[] -> floorHeight -> BVH (mesh.cpp:5-136, bvh.cpp)."""

    def __init__(self, glb_path=None, tris=None):
        L = lib()
        if glb_path is not None:
            self._h = L.uvrt_host_mesh_load(os.fsencode(glb_path))
            if not self._h:
                raise capi.UvrtError("cannot load %s" % glb_path)
        else:
            t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
            self._h = L.uvrt_host_mesh_from_tris(t.ctypes.data_as(_vp), t.shape[0])
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.uvrt_host_mesh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def triangleCount(self):
        return int(self._L.uvrt_host_mesh_tri_count(self._h))

    @property
    def floorHeight(self):
        return float(self._L.uvrt_host_mesh_floor_height(self._h))

    @property
    def nodesUsed(self):
        return int(self._L.uvrt_host_mesh_nodes_used(self._h))

    def _view(self, ptr, nbytes):
        return (C.c_char * nbytes).from_address(ptr)

    def tris(self):
        T = self.triangleCount
        return np.frombuffer(self._view(self._L.uvrt_host_mesh_tris(self._h), T * 64),
                             dtype=np.float32).reshape(T, 16).copy()

    def nodes(self):
        n = self.nodesUsed
        return np.frombuffer(self._view(self._L.uvrt_host_mesh_nodes(self._h), n * 32), dtype=NODE_DT).copy()

    def triIdx(self):
        T = self.triangleCount
        return np.frombuffer(self._view(self._L.uvrt_host_mesh_tri_idx(self._h), T * 4), dtype=np.uint32).copy()

    def rebuild_bvh(self):
        self._L.uvrt_host_mesh_rebuild_bvh(self._h)


class RayTracer:
    """Tmpl8::RayTracer over the HIP C ABI.  `glb` / `route_xml` are conveniences of the
    binding: the route file is loaded from its own directory under its own name."""

    def __init__(self, glb=None, route_xml=None, device=0, mesh=None, init=True):
        L = lib()
        self._L = L
        if not init:          # route / parameter handling only: no device context is created
            self.mesh = None
            self._h = L.uvrt_host_rt_new()
            L.uvrt_host_rt_set_auto_save(self._h, 0)
            self.ctx = None
            return
        self.mesh = mesh if mesh is not None else Mesh(glb)
        self._h = L.uvrt_host_rt_new()
        L.uvrt_host_rt_set_device(self._h, int(device))
        L.uvrt_host_rt_set_auto_save(self._h, 0)
        if route_xml is not None:
            d, name = os.path.split(os.path.abspath(route_xml))
            L.uvrt_host_rt_set_route_dir(self._h, os.fsencode(d + os.sep))
            L.uvrt_host_rt_set_default_route(self._h, os.fsencode(os.path.splitext(name)[0]))
        else:
            L.uvrt_host_rt_set_route_dir(self._h, b"/nonexistent/")
        L.uvrt_host_rt_init(self._h, self.mesh._h)
        self.ctx = _BorrowedCtx(L.uvrt_host_rt_ctx(self._h), self.mesh.triangleCount)

    def close(self):
        if getattr(self, "_h", None):
            self._L.uvrt_host_rt_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getattr__(self, name):
        if name in _FIELDS:
            v = C.c_double()
            self._L.uvrt_host_rt_get(self._h, name.encode(), C.byref(v))
            if name in _BOOL_FIELDS:
                return bool(v.value)
            return int(v.value) if name in _INT_FIELDS else float(v.value)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _FIELDS:
            if name == "reflectBounces" and not (0 <= int(value) <= 16 and int(value) == value):
                raise ValueError("reflectBounces must be an integer in [0, 16]")
            if name == "reflectSided" and not (int(value) in (0, 1) and int(value) == value):
                raise ValueError("reflectSided must be 0 or 1")
            if name == "gatherBatch":
                _check_gather_batch(value)
            self._L.uvrt_host_rt_set(self._h, name.encode(), float(value))
            if name == "photonCount":
                self._L.uvrt_host_rt_update_photons_per_light(self._h)
        else:
            object.__setattr__(self, name, value)

    # ---- RayTracer::reflectMap: a reflectance per face for the face-resolved bounces ----
    @property
    def reflectMap(self):
        """the rules file of the reflectance map ("" for none); a relative name is resolved against the route directory.  Used
        only with reflectSided = 1; every face starts at `reflectance`."""
        buf = C.create_string_buffer(4096)
        self._L.uvrt_host_rt_get_reflect_map(self._h, buf, len(buf))
        return os.fsdecode(buf.value)

    @reflectMap.setter
    def reflectMap(self, path):
        path = path or ""
        if any(ch in path for ch in "<>&"):
            raise ValueError("reflectMap: a file name with <, > or & cannot stand in a route file")
        self._L.uvrt_host_rt_set_reflect_map(self._h, os.fsencode(path))

    def SetReflectanceMap(self, planes):
        """the planes themselves, float32[2][T] (face 0's, then face 1's), for a caller that brings them; None forgets them"""
        if planes is None:
            self._L.uvrt_host_rt_set_reflectance_map(self._h, None, 0)
            return
        v = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1)
        if not (np.all(np.isfinite(v)) and np.all(v >= 0.0) and np.all(v <= 1.0)):
            raise ValueError("every reflectance must be finite and in [0, 1]")
        if self.mesh is not None and v.size != 2 * self.mesh.triangleCount:
            raise ValueError("the reflectance map must hold 2 x triangleCount values")
        self._L.uvrt_host_rt_set_reflectance_map(self._h, v.ctypes.data_as(_vp), v.size)

    def reflectance_map(self):
        """the planes a mapped launch would upload now: the file's when reflectMap names one (None until it has been read), else
        SetReflectanceMap's; None without either"""
        n = self._L.uvrt_host_rt_reflectance_map(self._h, None, 0)
        if n == 0:
            return None
        out = np.empty(n, dtype=np.float32)
        self._L.uvrt_host_rt_reflectance_map(self._h, out.ctypes.data_as(_vp), n)
        return out.reshape(2, -1)

    def _has_reflect_map(self):
        return bool(self._L.uvrt_host_rt_has_reflect_map(self._h))

    def _check_reflect_map(self, base=None, sided=None):
        """what the host layer would end the process for: a map without reflectSided, a rules file with a line it cannot read (the
        file is read here, once per name and base, into the cache the launches use), a map of the wrong size"""
        if not self._has_reflect_map():
            return
        if not (self.reflectSided if sided is None else sided):
            raise ValueError("reflectMap needs reflectSided = 1: only the face-resolved bounces know which face a reflectance belongs to")
        if self.mesh is None:
            raise ValueError("a reflectance map needs a mesh (this RayTracer was made with init=False)")
        err = C.create_string_buffer(1024)
        if self._L.uvrt_host_rt_prepare_reflect_map(self._h, float(np.float32(self.reflectance if base is None else base)), err,
                                                    len(err)) != 0:
            raise ValueError(err.value.decode(errors="replace"))
        if self._L.uvrt_host_rt_reflectance_map(self._h, None, 0) != 2 * self.mesh.triangleCount:
            raise ValueError("the reflectance map must hold 2 x triangleCount values")

    # ---- RayTracer::mirrorMap: specular panels and the mirror gather behind every gather launch ----
    @property
    def mirrorMap(self):
        """the rules file of the specular panels ("" for none); a relative name is resolved against the route directory.  Used
        only with gatherSamples > 0."""
        buf = C.create_string_buffer(4096)
        self._L.uvrt_host_rt_get_mirror_map(self._h, buf, len(buf))
        return os.fsdecode(buf.value)

    @mirrorMap.setter
    def mirrorMap(self, path):
        path = path or ""
        if any(ch in path for ch in "<>&"):
            raise ValueError("mirrorMap: a file name with <, > or & cannot stand in a route file")
        self._L.uvrt_host_rt_set_mirror_map(self._h, os.fsencode(path))

    def SetMirrors(self, panels, panel_of_tri=None):
        """the panels themselves (capi.mirror records, 1 to 8) and panel_of_tri uint8[T] (0 or k + 1), for a caller that brings
        them; SetMirrors(None) forgets them"""
        if panels is None:
            self._L.uvrt_host_rt_set_mirrors(self._h, None, 0, None, 0)
            return
        rec = np.ascontiguousarray(np.array(panels, dtype=capi.MIRROR_DT).reshape(-1))
        members = np.ascontiguousarray(panel_of_tri, dtype=np.uint8).reshape(-1)
        if not 1 <= rec.size <= capi.MIRROR_MAX:
            raise ValueError("SetMirrors takes 1 to %d panels" % capi.MIRROR_MAX)
        ok = np.isfinite(rec["point"]).all() and np.isfinite(rec["normal"]).all() and np.isfinite(rec["reflectance"]).all()
        if not ok or (rec["reflectance"] < 0).any() or (rec["reflectance"] > 1).any() or (rec["reserved"] != 0).any():
            raise ValueError("every panel needs finite values, a reflectance in [0, 1] and reserved = 0")
        if (np.abs(rec["normal"]).max(axis=1) == 0).any():
            raise ValueError("a panel's normal is zero")
        if members.size and members.max() > rec.size:
            raise ValueError("panel_of_tri names a panel that is not there")
        if self.mesh is not None and members.size != self.mesh.triangleCount:
            raise ValueError("panel_of_tri must hold triangleCount entries")
        self._L.uvrt_host_rt_set_mirrors(self._h, rec.ctypes.data_as(_vp), rec.size, members.ctypes.data_as(_vp), members.size)

    def _has_mirrors(self):
        return bool(self._L.uvrt_host_rt_has_mirrors(self._h))

    def _check_mirrors(self, samples=None):
        """what the host layer would end the process for: panels without gatherSamples, a rules file with a line it cannot read
        (the file is read here, once per name, into the cache the launches use)"""
        if not self._has_mirrors():
            return
        if not (self.gatherSamples if samples is None else samples):
            raise ValueError("mirrorMap needs gatherSamples > 0: the mirror gather adds to the direct gather's plane")
        if self.mesh is None:
            raise ValueError("specular panels need a mesh (this RayTracer was made with init=False)")
        err = C.create_string_buffer(1024)
        if self._L.uvrt_host_rt_prepare_mirror_map(self._h, err, len(err)) != 0:
            raise ValueError(err.value.decode(errors="replace"))

    # ---- RayTracer::sensorMap: virtual dosimeters gathered beside every launch ----
    @property
    def sensorMap(self):
        """the rules file of the sensors ("" for none); a relative name is resolved against the route directory"""
        buf = C.create_string_buffer(4096)
        self._L.uvrt_host_rt_get_sensor_map(self._h, buf, len(buf))
        return os.fsdecode(buf.value)

    @sensorMap.setter
    def sensorMap(self, path):
        path = path or ""
        if any(ch in path for ch in "<>&"):
            raise ValueError("sensorMap: a file name with <, > or & cannot stand in a route file")
        self._L.uvrt_host_rt_set_sensor_map(self._h, os.fsencode(path))

    def set_sensors(self, sensors):
        """RayTracer::SetSensors: the sensors themselves (capi.sensor records or a capi.SENSOR_DT array), for a caller that
        brings them; None forgets them"""
        if sensors is None:
            self._L.uvrt_host_rt_set_sensors(self._h, None, 0)
            return
        rec = np.ascontiguousarray(np.array(sensors, dtype=capi.SENSOR_DT).reshape(-1))
        if not 1 <= rec.size <= capi.SENSOR_MAX:
            raise ValueError("set_sensors takes 1 to 2^24 sensors")
        if not (np.isfinite(rec["pos"]).all() and np.isfinite(rec["normal"]).all()):
            raise ValueError("every sensor needs a finite position and normal")
        if (~np.isin(rec["kind"], (capi.SENSOR_PLANAR, capi.SENSOR_SPHERICAL))).any() or (rec["reserved"] != 0).any():
            raise ValueError("every sensor needs kind 0 (planar) or 1 (spherical) and reserved = 0")
        if ((rec["kind"] == capi.SENSOR_PLANAR) & (np.abs(rec["normal"]).max(axis=1) == 0)).any():
            raise ValueError("a planar sensor's normal is zero")
        self._L.uvrt_host_rt_set_sensors(self._h, rec.ctypes.data_as(_vp), rec.size)

    SetSensors = set_sensors

    def _has_sensors(self):
        return bool(self._L.uvrt_host_rt_has_sensors(self._h))

    def _check_sensors(self, batched=False):
        """what the host layer would end the process for: sensors beside mirror panels or in a batched computation, a rules file
        with a line it cannot read (the file is read here, once per name, into the cache the launches use)"""
        if not self._has_sensors():
            return
        if batched:
            raise ValueError("sensors are not supported by ComputeIterationsBatched: they are gathered launch by launch")
        if self._has_mirrors():
            raise ValueError("sensors are not supported with mirror panels: a sensor would not see the panels' light")
        err = C.create_string_buffer(1024)
        if self._L.uvrt_host_rt_prepare_sensor_map(self._h, err, len(err)) != 0:
            raise ValueError(err.value.decode(errors="replace"))

    def sensors(self):
        """the sensors a launch would gather now, capi.SENSOR_DT (the file's once it has been read, else set_sensors')"""
        self._check_sensors()
        n = self._L.uvrt_host_rt_active_sensors(self._h, None, 0)
        out = np.zeros(max(n, 1), dtype=capi.SENSOR_DT)
        self._L.uvrt_host_rt_active_sensors(self._h, out.ctypes.data_as(_vp), n)
        return out[:n].copy()

    def read_sensors(self):
        """RayTracer::ReadSensors: (dose float32[K] in mJ/cm^2, peak float32[K] in microW/cm^2, one standard error of dose
        float64[K]) under the divisors and scaled powers Shade uses for the dosage and the maxpower view"""
        if not self._has_sensors():
            raise ValueError("read_sensors: no sensors (sensorMap or set_sensors)")
        self._check_sensors()
        n = self._L.uvrt_host_rt_active_sensors(self._h, None, 0)
        dose, peak, err = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float64)
        self._L.uvrt_host_rt_read_sensors(self._h, dose.ctypes.data_as(_vp), peak.ctypes.data_as(_vp), err.ctypes.data_as(_vp), n)
        return dose, peak, err

    ReadSensors = read_sensors

    def calibrate_power_at_sensor(self, measure_power, sensor, light_index=0):
        """RayTracer::CalibratePowerAtSensor: lightIntensity from a reading of `measure_power` at sensor `sensor` with the lamp
        at position `light_index`, in the room as it stands; returns the calibrated power"""
        if not self._has_sensors():
            raise ValueError("calibrate_power_at_sensor: no sensors (sensorMap or set_sensors)")
        self._check_sensors()
        self._check_reflect_map()
        if not 0 <= int(sensor) < self._L.uvrt_host_rt_active_sensors(self._h, None, 0):
            raise ValueError("calibrate_power_at_sensor: no such sensor")
        if not 0 <= int(light_index) < self._L.uvrt_host_rt_lamp_count(self._h):
            raise ValueError("calibrate_power_at_sensor: no such lamp position")
        self._L.uvrt_host_rt_calibrate_at_sensor(self._h, float(measure_power), int(sensor), int(light_index))
        return self.calibratedPower

    CalibratePowerAtSensor = calibrate_power_at_sensor

    # reference method names
    def UpdatePhotonsPerLight(self): self._L.uvrt_host_rt_update_photons_per_light(self._h)
    def ComputeDosageMap(self):
        self._check_sensors()
        self._check_reflect_map()
        self._check_mirrors()
        self._L.uvrt_host_rt_compute_dosage_map(self._h)
    def ComputeSingleLightDosageMap(self, lamp, photonsPerLight, triangleCount):
        self._check_sensors()
        self._check_reflect_map()
        self._check_mirrors()
        self._L.uvrt_host_rt_compute_single(self._h, lamp[0], lamp[1], lamp[2], int(photonsPerLight),
                                            int(triangleCount))
    def ComputeSegmentDosageMap(self, a, b, photonsPerLight, triangleCount):
        """the dose of the drive from position a to position b ((x, z) pairs) at driveSpeed"""
        self._check_sensors()
        self._check_reflect_map()
        self._check_mirrors()
        self._L.uvrt_host_rt_compute_segment(self._h, a[0], a[1], b[0], b[1], int(photonsPerLight), int(triangleCount))
    def ComputeSegments(self):
        """the segments of one iteration, in order (nothing at driveSpeed 0)"""
        self._check_sensors()
        self._check_reflect_map()
        self._check_mirrors()
        self._L.uvrt_host_rt_compute_segments(self._h)
    def Shade(self): self._L.uvrt_host_rt_shade(self._h)
    def ResetDosageMap(self):
        self._check_sensors()
        self._L.uvrt_host_rt_reset_dosage_map(self._h)
    def ClearBuffers(self, resetColor): self._L.uvrt_host_rt_clear_buffers(self._h, int(bool(resetColor)))
    def AddLamp(self): self._L.uvrt_host_rt_add_lamp(self._h)
    def CalibratePower(self, measurePower, measureHeight, measureDist):
        self._L.uvrt_host_rt_calibrate(self._h, measurePower, measureHeight, measureDist)
    def SaveRoute(self, name): self._L.uvrt_host_rt_save_route(self._h, os.fsencode(name))
    def LoadRoute(self, name): self._L.uvrt_host_rt_load_route(self._h, os.fsencode(name))
    def set_route_dir(self, d): self._L.uvrt_host_rt_set_route_dir(self._h, os.fsencode(d))

    # headless additions
    def Sync(self): self._L.uvrt_host_rt_sync(self._h)
    def set_shard(self, rank, world): self._L.uvrt_host_rt_set_shard(self._h, int(rank), int(world))
    def ComputeIterationsBatched(self, iterations):
        self._check_sensors(batched=True)
        self._L.uvrt_host_rt_compute_batched(self._h, int(iterations))
    def SetRayRange(self, rank, world): self._L.uvrt_host_rt_set_ray_range(self._h, int(rank), int(world))
    def set_reduce_over_comm(self, on): self._L.uvrt_host_rt_set_reduce_over_comm(self._h, int(bool(on)))

    @property
    def gather_batch(self):
        """RayTracer::gatherBatch = B: with gatherSamples > 0 the launches of ComputeDosageMap / ComputeSegments are traced in
        groups of up to B (one uvrt_gather_direct_batch each).  0 (default) and 1: launch by launch.  B changes
        no bit of any result."""
        return self.gatherBatch

    @gather_batch.setter
    def gather_batch(self, value):
        self.gatherBatch = value

    def set_gather_refine(self, rel_error, max_extra=64):
        """gatherRelError and gatherMaxExtra in one call: every gather launch is refined (0: off)"""
        self._L.uvrt_host_rt_set_gather_refine(self._h, float(rel_error), int(max_extra))

    def PlanDurations(self, min_dose=None, min_photons=16, margin=1e-6, rel_gap=1e-3, max_iterations=200, mask=None,
                      gather_samples=0, gather_sampling=0, gather_confidence=0.0):
        """RayTracer::PlanDurations: one batched computation over the current positions from the current SEED with the
        exposure captured, then the least durations that bring every required triangle to min_dose (default: the
        route's minDosage).  They are written into the positions; returns (durations float32[P], report dict with
        the starting "seed").  With driveSpeed > 0 (2 to 128 positions) the segments between consecutive positions are
        fixed columns of the plan at the time the drive takes: the dict then also carries the fields of the bounds
        report (capi.PlanBoundsReport) and "segment_durations" (float32[P - 1]).  gather_samples = S > 0 plans from the
        direct gather instead (PlanOptions::gatherSamples): the launches of a gatherSamples = S run, launch by launch, into
        an exposure matrix of f64 expected counts (ctx.plan_read_exposure_expected), so triangles no photon reaches are
        planned for too; the plan is as good as the estimator.  gather_sampling (PlanOptions::gatherSampling)
        is those launches' sampling mode: 0 independent, 1 stratified; it needs gather_samples > 0.
        gather_confidence = z > 0 (PlanOptions::gatherConfidence) plans for the estimate's lower confidence bound, expected -
        z standard errors element by element; it needs gather_samples >= 2 and is meant for 16 and more.
        0 is the plan without it, bit for bit.  (PlanDurationsBatched, PlanDurationsRefined and PlanDurationsReflect also take
        mirror_mapped = 1 (PlanOptions::mirrorMapped) among their plan arguments: the mirror gather over the ray tracer's specular
        panels (mirrorMap or SetMirrors) follows every gather launch of the plan; it needs gather_samples > 0 and
        panels and refuses gather_confidence.)  (PlanDurationsRefined is this call with the adaptive gather, PlanDurationsBatched
        with the plan's gather launches traced in groups.)"""
        return self._plan_durations(min_dose, min_photons, margin, rel_gap, max_iterations, mask, gather_samples, gather_sampling,
                                    gather_confidence, 0.0, 64)

    def PlanDurationsBatched(self, gather_batch, **plan):
        """PlanDurations(**plan) with PlanOptions::gatherBatch = B in [0, 64]: the plan's gather launches are traced in groups of
        up to B, one shadow-ray pass each.  B > 0 needs gather_samples > 0; it changes no bit of the durations, the
        report or the captured columns.  0 and 1 are PlanDurations.  (PlanDurationsRefined and PlanDurationsReflect take
        gather_batch = B among their plan arguments.)"""
        args = _plan_args("PlanDurationsBatched", plan, mirror_mapped=0)
        return self._plan_durations(gather_rel_error=0.0, gather_max_extra=64, gather_batch=gather_batch, **args)

    def PlanDurationsRefined(self, gather_rel_error, gather_max_extra=64, **plan):
        """PlanDurations(**plan) with PlanOptions::gatherRelError = gather_rel_error and gatherMaxExtra = gather_max_extra:
        every gather launch of the plan is refined before its capture.  tau > 0 needs gather_samples >= 2 and
        works with and without gather_confidence; 0 is PlanDurations, bit for bit."""
        args = _plan_args("PlanDurationsRefined", plan, gather_batch=0, mirror_mapped=0)
        return self._plan_durations(gather_rel_error=gather_rel_error, gather_max_extra=gather_max_extra, **args)

    def PlanDurationsReflect(self, reflectance, reflect_samples=16, gather_rel_error=0.0, gather_max_extra=64, reflect_bounces=0,
                             reflect_sided=0, reflect_mapped=0, **plan):
        """PlanDurations(**plan) with PlanOptions::reflectance = rho and reflectSamples: every gather launch of the plan gets one
        diffuse bounce before its capture.  rho > 0 needs gather_samples > 0 and refuses gather_confidence: the
        variance plane knows nothing of the indirect part.  0 is PlanDurations / PlanDurationsRefined, bit for bit.
        reflect_bounces = K in [1, 16] (PlanOptions::reflectBounces): K bounces over hit links recorded once per scene instead of
        the bounce traced per launch; 0 is the traced bounce, bit for bit.
        reflect_sided = 1 (PlanOptions::reflectSided): those K bounces face-resolved; it needs rho > 0 and K >= 1 and
        refuses gather_batch >= 2; 0 is the two-sided bounces, bit for bit.
        reflect_mapped = 1 (PlanOptions::reflectMapped): those bounces take the ray tracer's reflectance map (reflectMap or
        SetReflectanceMap) with rho as every face's start; it needs reflect_sided = 1 and a map; 0 is the one rho,
        bit for bit."""
        args = _plan_args("PlanDurationsReflect", plan, gather_batch=0, mirror_mapped=0)
        rho, s2 = float(np.float32(reflectance)), int(reflect_samples)
        if int(reflect_bounces) != reflect_bounces or not (0 <= int(reflect_bounces) <= 16):
            raise ValueError("reflect_bounces must be an integer in [0, 16]")
        if not (0.0 <= rho <= 1.0):
            raise ValueError("reflectance must be in [0, 1]")
        if reflect_sided not in (0, 1) or int(reflect_sided) != reflect_sided:
            raise ValueError("reflect_sided must be 0 or 1")
        if reflect_sided and not rho > 0.0:
            raise ValueError("reflect_sided needs reflectance > 0: without a bounce there are no faces to resolve")
        if reflect_sided and int(reflect_bounces) < 1:
            raise ValueError("reflect_sided needs reflect_bounces >= 1: the traced single bounce has no face-resolved form")
        if reflect_sided and _check_gather_batch(args["gather_batch"]):
            raise ValueError("reflect_sided is not supported with gather_batch >= 2: a gather batch keeps no face planes")
        if reflect_mapped not in (0, 1) or int(reflect_mapped) != reflect_mapped:
            raise ValueError("reflect_mapped must be 0 or 1")
        if reflect_mapped and not reflect_sided:
            raise ValueError("reflect_mapped needs reflect_sided = 1: only the face-resolved bounces know which face a reflectance belongs to")
        if reflect_mapped and not self._has_reflect_map():
            raise ValueError("reflect_mapped needs a reflectance map (reflectMap or SetReflectanceMap)")
        if reflect_mapped:
            self._check_reflect_map(base=rho, sided=1)
        if rho > 0.0 and not args["gather_samples"]:
            raise ValueError("reflectance needs gather_samples > 0")
        if rho > 0.0 and float(args["gather_confidence"]) != 0.0:
            raise ValueError("reflectance is not supported with gather_confidence")
        if rho > 0.0 and (s2 < 2 or s2 > 4096 or s2 & 1):
            raise ValueError("reflect_samples must be even and in [2, 4096]")
        return self._plan_durations(gather_rel_error=gather_rel_error, gather_max_extra=gather_max_extra, reflectance=rho,
                                    reflect_samples=s2, reflect_bounces=int(reflect_bounces), reflect_sided=int(reflect_sided),
                                    reflect_mapped=int(reflect_mapped), **args)

    def _plan_durations(self, min_dose, min_photons, margin, rel_gap, max_iterations, mask, gather_samples, gather_sampling,
                        gather_confidence, gather_rel_error, gather_max_extra, reflectance=0.0, reflect_samples=16,
                        reflect_bounces=0, gather_batch=0, reflect_sided=0, reflect_mapped=0, mirror_mapped=0):
        if mirror_mapped not in (0, 1) or int(mirror_mapped) != mirror_mapped:
            raise ValueError("mirror_mapped must be 0 or 1")
        if mirror_mapped and not gather_samples:
            raise ValueError("mirror_mapped needs gather_samples > 0")
        if mirror_mapped and float(gather_confidence) != 0.0:
            raise ValueError("mirror_mapped is not supported with gather_confidence: the variance plane knows nothing of the specular part")
        if mirror_mapped and not self._has_mirrors():
            raise ValueError("mirror_mapped needs specular panels (mirrorMap or SetMirrors)")
        if mirror_mapped:
            self._check_mirrors(samples=gather_samples)
        if gather_sampling and not gather_samples:
            raise ValueError("gather_sampling needs gather_samples > 0")
        B = _check_gather_batch(gather_batch)
        if B and not gather_samples:
            raise ValueError("gather_batch needs gather_samples > 0")
        z = float(gather_confidence)
        if not (z >= 0.0) or z == float("inf"):
            raise ValueError("gather_confidence must be finite and >= 0")
        if z > 0.0 and int(gather_samples) < 2:
            raise ValueError("gather_confidence needs gather_samples >= 2")
        tau, extra = float(gather_rel_error), int(gather_max_extra)
        if not (tau >= 0.0) or tau == float("inf"):
            raise ValueError("gather_rel_error must be finite and >= 0")
        if tau > 0.0 and int(gather_samples) < 2:
            raise ValueError("gather_rel_error needs gather_samples >= 2")
        if tau > 0.0 and (extra < 2 or extra > 4096 or extra & (extra - 1)):
            raise ValueError("gather_max_extra must be a power of two in [2, 4096]")
        keep = _mask_arg(mask, self.mesh.triangleCount)
        opt = PlanOptions(min_dose=-1.0 if min_dose is None else float(min_dose), min_photons=int(min_photons), margin=float(margin),
                          rel_gap=float(rel_gap), max_iterations=int(max_iterations), mask=_addr(keep),
                          gather_samples=int(gather_samples), gather_sampling=int(gather_sampling), gather_confidence=z,
                          gather_rel_error=tau, gather_max_extra=extra, reflectance=float(reflectance),
                          reflect_samples=int(reflect_samples), reflect_bounces=int(reflect_bounces),
                          reflect_sided=int(reflect_sided), reflect_mapped=int(reflect_mapped), mirror_mapped=int(mirror_mapped),
                          gather_batch=B)
        rep, seed = capi.PlanReport(), C.c_uint()
        self._L.uvrt_host_rt_plan(self._h, C.byref(opt), C.byref(rep), C.byref(seed))
        return _plan_result(self, rep, seed)

    def EndPlan(self):
        """release the exposure matrix PlanDurations leaves on the device (model dose / required set read-backs)"""
        self._L.uvrt_host_rt_end_plan(self._h)

    def SetCandidateGrid(self, nx, nz, inset=0.5):
        """replace the positions by an nx x nz grid over the mesh's x/z bounds, inset by `inset` metres"""
        self._L.uvrt_host_rt_set_candidate_grid(self._h, int(nx), int(nz), float(inset))

    def lamps(self):
        out = []
        buf = (C.c_float * 3)()
        for i in range(self._L.uvrt_host_rt_lamp_count(self._h)):
            self._L.uvrt_host_rt_get_lamp(self._h, i, buf)
            out.append((float(buf[0]), float(buf[1]), float(buf[2])))
        return out

    def set_lamps(self, lamps):
        flat = (C.c_float * (3 * len(lamps)))(*[float(np.float32(v)) for l in lamps for v in l])
        self._L.uvrt_host_rt_set_lamps(self._h, flat, len(lamps))

    def read_dosage(self, first=0, count=None):
        T = self.mesh.triangleCount
        count = T - first if count is None else count
        out = np.empty(count, dtype=np.float32)
        self._L.uvrt_host_rt_read_dosage(self._h, out.ctypes.data_as(_vp), first, count)
        return out


def compute_iterations_batched_group(rts, iterations):
    """RayTracer::ComputeIterationsBatched over instances that share every launch by ray range (one process)."""
    arr = (C.c_void_p * len(rts))(*[rt._h for rt in rts])
    lib().uvrt_host_rt_compute_batched_group(arr, len(rts), int(iterations))


def _check_gather_batch(value):
    if int(value) != value or not (0 <= int(value) <= 64):
        raise ValueError("gather_batch must be an integer in [0, 64]")
    return int(value)


def _plan_args(who, plan, **own):
    """the **plan of the wrapper `who` over PlanDurations' arguments and the wrapper's `own`; a name that is neither is a TypeError"""
    args = dict(min_dose=None, min_photons=16, margin=1e-6, rel_gap=1e-3, max_iterations=200, mask=None, gather_samples=0,
                gather_sampling=0, gather_confidence=0.0, **own)
    unknown = set(plan) - set(args)
    if unknown:
        raise TypeError("%s: unknown arguments %s" % (who, sorted(unknown)))
    args.update(plan)
    return args


def _mask_arg(mask, T):
    if mask is None:
        return None
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    if m.size != T:
        raise ValueError("mask must have one entry per triangle")
    return m


def _addr(a):
    return None if a is None else a.ctypes.data


def _plan_result(rt, rep, seed):
    d = rep.as_dict()
    d["seed"] = int(seed.value)
    brep = capi.PlanBoundsReport()
    rt._L.uvrt_host_rt_plan_bounds(rt._h, C.byref(brep))
    if brep.fixed_columns > 0:        # a driving plan: the segments were fixed columns
        d.update(brep.as_dict())
        seg = (C.c_float * brep.fixed_columns)()
        n = rt._L.uvrt_host_rt_plan_segments(rt._h, seg, brep.fixed_columns)
        d["segment_durations"] = np.frombuffer(seg, dtype=np.float32)[:n].copy()
    return np.array([l[2] for l in rt.lamps()], dtype=np.float32), d


def plan_durations_group(rts, min_dose=None, min_photons=16, margin=1e-6, rel_gap=1e-3, max_iterations=200, mask=None):
    """RayTracer::PlanDurations over instances that share every launch by ray range (one process): every context
    captures after the group reduce and solves on its own; the durations must agree."""
    arr = (C.c_void_p * len(rts))(*[rt._h for rt in rts])
    keep = _mask_arg(mask, rts[0].mesh.triangleCount)
    opt = PlanOptions(min_dose=-1.0 if min_dose is None else float(min_dose), min_photons=int(min_photons), margin=float(margin),
                      rel_gap=float(rel_gap), max_iterations=int(max_iterations), mask=_addr(keep))
    rep, seed = capi.PlanReport(), C.c_uint()
    lib().uvrt_host_rt_plan_group(arr, len(rts), C.byref(opt), C.byref(rep), C.byref(seed))
    return _plan_result(rts[0], rep, seed)


def grid_positions(bounds, nx, nz, inset=0.5):
    """RayTracer::GridPositions: (x, z) of an nx x nz grid over bounds = (xmin, xmax, zmin, zmax) inset by `inset`,
    x fastest; float32[nx * nz, 2]"""
    out = (C.c_float * (2 * nx * nz))()
    xmin, xmax, zmin, zmax = (float(v) for v in bounds)
    lib().uvrt_host_grid_positions(xmin, xmax, zmin, zmax, int(nx), int(nz), float(inset), out)
    return np.frombuffer(out, dtype=np.float32).reshape(nx * nz, 2).copy()


def route_launches(lamps, y, drive_speed):
    """RayTracer::RouteLaunches: the launches of one iteration over lamps = (x, z, duration) triples with the lamp's foot
    at height y: the stops, then (drive_speed > 0, two positions or more) the segments; ROUTE_LAUNCH_DT[P]"""
    xzd = np.ascontiguousarray(lamps, dtype=np.float32).reshape(-1, 3)
    L = lib()
    n = L.uvrt_host_route_launches(xzd.ctypes.data, len(xzd), float(y), float(drive_speed), None, 0)
    out = np.zeros(n, dtype=ROUTE_LAUNCH_DT)
    L.uvrt_host_route_launches(xzd.ctypes.data, len(xzd), float(y), float(drive_speed), out.ctypes.data, n)
    return out


class _BorrowedCtx(capi.Ctx):
    """The uvrt_ctx owned by a C++ RayTracer, exposed with the capi.Ctx methods (read-backs,
    knobs, device pointers).  Never destroyed from Python."""

    def __init__(self, handle, T):
        self._L = capi.lib()
        self._h = C.c_void_p(handle)
        self.T = T

    def close(self):
        self._h = None
