"""Python binding of libprt_hip.so (ctypes over the C ABI in include/prt.h).

This is test / benchmark plumbing: numpy (or torch device pointers) in, numpy out.  All compute
happens in the HIP kernels; there is no Python or CPU fallback — if the library or a GPU is missing
the calls raise PrtError.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEV_LIB_PATH = os.path.join(_HERE, "libprt_hip_dev.so")
# PRT_LIB=<path>: another build of the library (A/B tools); PRT_DEV_LIB=1: the dev-hooks build (sweep tools that set PRT_TUNE_*)
_LIB_PATH = os.environ.get("PRT_LIB") or (_DEV_LIB_PATH if os.environ.get("PRT_DEV_LIB") == "1" else os.path.join(_HERE, "libprt_hip.so"))
_libs = {}


class PrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libprt_hip error {code}: {msg}")
        self.code = code


def lib_path():
    return _LIB_PATH


def load():
    """dlopen the in-tree libprt_hip.so (build it first with pooraytracer_amd.build.build())."""
    if _LIB_PATH in _libs:
        return _libs[_LIB_PATH]
    if not os.path.exists(_LIB_PATH):
        raise PrtError(-100, f"{_LIB_PATH} not built; run `python -m pooraytracer_amd.build` (needs hipcc)")
    # PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1 (same SONAMEs as /opt/rocm).
    # Two HIP runtimes cannot coexist in one process, and torch fails to initialise on the system
    # one, so when torch is importable it is imported first and this library binds to its runtime.
    if not os.environ.get("PRT_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(_LIB_PATH)
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    L.prt_abi_version.restype = C.c_int
    L.prt_last_error.restype = C.c_char_p
    L.prt_device_count.argtypes = [C.POINTER(C.c_int)]
    L.prt_scene_create.argtypes = [vp, C.POINTER(vp)]
    L.prt_scene_destroy.argtypes = [vp]
    L.prt_scene_destroy.restype = None
    L.prt_scene_upload.argtypes = [vp, i32]
    L.prt_scene_bvh_info.argtypes = [vp, vp]
    L.prt_scene_update_vertices.argtypes = [vp, vp, vp]
    L.prt_scene_refit.argtypes = [vp, vp, vp]
    L.prt_scene_refit_device.argtypes = [vp, vp, vp, vp]
    L.prt_scene_refit_info.argtypes = [vp, vp]
    L.prt_scene_rebuild.argtypes = [vp, vp, vp]
    L.prt_scene_rebuild_device.argtypes = [vp, vp, vp, vp]
    L.prt_scene_set_dynamic_lights.argtypes = [vp, i32]
    L.prt_scene_get_dynamic_lights.argtypes = [vp, C.POINTER(C.c_int)]
    L.prt_scene_light_update_info.argtypes = [vp, vp]
    L.prt_scene_set_distance_queries.argtypes = [vp, i32]
    L.prt_scene_get_distance_queries.argtypes = [vp, C.POINTER(C.c_int)]
    L.prt_closest_point.argtypes = [vp, vp, sz, vp, i32]
    L.prt_closest_point_device.argtypes = [vp, vp, sz, vp, i32, vp]
    L.prt_scene_topology_info.argtypes = [vp, vp]
    L.prt_scene_set_signed_queries.argtypes = [vp, i32]
    L.prt_scene_get_signed_queries.argtypes = [vp, C.POINTER(C.c_int)]
    L.prt_scene_pseudonormals.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.prt_signed_distance.argtypes = [vp, vp, sz, vp, i32]
    L.prt_signed_distance_device.argtypes = [vp, vp, sz, vp, i32, vp]
    L.prt_scene_set_winding_queries.argtypes = [vp, i32]
    L.prt_scene_get_winding_queries.argtypes = [vp, C.POINTER(C.c_int)]
    L.prt_scene_winding_moments.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.prt_winding_number.argtypes = [vp, vp, sz, C.c_double, vp, i32]
    L.prt_winding_number_device.argtypes = [vp, vp, sz, C.c_double, vp, i32, vp]
    L.prt_scene_light_table_words.argtypes = [vp, vp, u64, C.POINTER(u64)]
    L.prt_scene_light_count.argtypes = [vp, C.POINTER(u64)]
    L.prt_scene_light_order.argtypes = [vp, vp, u64]
    L.prt_trace_closest.argtypes = [vp, vp, sz, vp, i32]
    L.prt_trace_closest_device.argtypes = [vp, vp, sz, vp, i32, vp]
    L.prt_trace_closest_device_prec.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_closest_sorted_device.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_occluded.argtypes = [vp, vp, sz, vp, i32]
    L.prt_trace_occluded_device.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_occluded_sorted_device.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_surface.argtypes = [vp, vp, sz, vp, i32]
    L.prt_trace_surface_device.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_surface_sorted_device.argtypes = [vp, vp, sz, vp, i32, i32, vp]
    L.prt_trace_multi.argtypes = [vp, vp, vp, sz, C.c_int32, vp, i32]
    L.prt_trace_multi_device.argtypes = [vp, vp, vp, sz, C.c_int32, vp, i32, i32, vp]
    L.prt_trace_multi_sorted_device.argtypes = [vp, vp, vp, sz, C.c_int32, vp, i32, i32, vp]
    L.prt_sample_lights.argtypes = [vp, vp, sz, u64, vp]
    L.prt_render.argtypes = [vp, vp, vp, vp, vp]
    L.prt_render_device.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    L.prt_ray_color.argtypes = [vp, vp, vp, sz, vp, C.c_int32, vp, vp]
    L.prt_ray_color_device.argtypes = [vp, vp, vp, sz, vp, C.c_int32, vp, vp, vp]
    L.prt_get_counters.argtypes = [vp, vp]
    L.prt_tonemap_srgb8.argtypes = [vp, vp, i32, i32, vp, vp]
    L.prt_material_eval.argtypes = [vp, i32, sz, vp, vp, vp, u64, vp]
    L.prt_material_scatter.argtypes = [vp, i32, sz, vp, vp, vp, vp, u64, vp, vp, vp]
    L.prt_texture_value.argtypes = [vp, i32, sz, vp, vp]
    L.prt_render_samples.argtypes = [vp, vp, vp, vp, sz, i32, i32, vp, vp]
    L.prt_render_multi.argtypes = [vp, i32, vp, vp, vp]
    L.prt_accum_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.prt_accum_destroy.argtypes = [vp]
    L.prt_accum_destroy.restype = None
    L.prt_accum_render.argtypes = [vp, C.c_int32, vp]
    L.prt_accum_samples.argtypes = [vp, C.POINTER(u64)]
    L.prt_accum_reset.argtypes = [vp]
    L.prt_accum_resolve.argtypes = [vp, vp, vp, vp, vp]
    L.prt_accum_read.argtypes = [vp, vp, vp]
    L.prt_accum_export.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.prt_accum_import.argtypes = [vp, vp, u64, u64]
    L.prt_accum_create_adaptive.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
    L.prt_accum_render_adaptive.argtypes = [vp, C.c_int32, C.POINTER(u64), vp]
    L.prt_accum_pixel_samples.argtypes = [vp, vp]
    L.prt_accum_export_adaptive.argtypes = [vp, vp, vp, vp, C.POINTER(u64), C.POINTER(u64)]
    L.prt_accum_import_adaptive.argtypes = [vp, vp, vp, vp, u64, u64]
    L.prt_denoise_defaults.argtypes = [vp]
    L.prt_denoise_defaults.restype = None
    L.prt_render_features.argtypes = [vp, vp, vp, C.c_int32, vp, vp, vp, vp]
    L.prt_render_features_device.argtypes = [vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
    L.prt_denoise.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
    L.prt_denoise_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp]
    L.prt_accum_resolve_denoised.argtypes = [vp, vp, vp, vp, vp]
    L.prt_accum_read_denoised.argtypes = [vp, vp, vp]
    L.prt_denoise_guided_defaults.argtypes = [vp]
    L.prt_denoise_guided_defaults.restype = None
    L.prt_denoise_guided.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.prt_denoise_guided_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.prt_accum_variance.argtypes = [vp, vp, vp]
    L.prt_accum_read_variance.argtypes = [vp, vp]
    L.prt_accum_resolve_denoised_guided.argtypes = [vp, vp, vp, vp, vp]
    L.prt_accum_read_denoised_guided.argtypes = [vp, vp, vp]
    if L.prt_abi_version() != _abi.PRT_ABI_VERSION and os.environ.get("PRT_ABI_ANY") != "1":  # (PRT_ABI_ANY: A/B tools timing an older build)
        raise PrtError(-101, "ABI version mismatch between _abi.py and libprt_hip.so")
    try:
        L.prt_shutdown.restype = None
        L.prt_dev_hooks.restype = C.c_int
    except AttributeError:
        if os.environ.get("PRT_ABI_ANY") != "1":
            raise
    _libs[_LIB_PATH] = L
    return L


def _point_queries(name, points, max_dist):
    """The PrtPointQuery batch of closest_point / signed_distance; shape and dtype errors are raised here."""
    if not isinstance(points, np.ndarray):
        raise TypeError(f"{name}: points must be a numpy array, not {type(points).__name__}")
    if points.dtype != np.float64:
        raise TypeError(f"{name}: points must be float64, not {points.dtype}")
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: points must have shape (n, 3), not {points.shape}")
    n = points.shape[0]
    md = np.asarray(max_dist)
    if md.dtype.kind not in "fiu":
        raise TypeError(f"{name}: max_dist must be real, not {md.dtype}")
    if md.shape not in ((), (n,)):
        raise ValueError(f"{name}: max_dist must be a scalar or have shape ({n},), not {md.shape}")
    q = np.zeros(n, dtype=_abi.POINT_QUERY_DTYPE)
    q["p"] = points
    q["max_dist"] = md
    return q


class dev_hooks:
    """`with api.dev_hooks():` — inside, scenes are created by libprt_hip_dev.so, the build of the same sources that reads the
    PRT_TUNE_* / PRT_TEST_* environment hooks (the shipped libprt_hip.so reads none).  A Scene keeps the library that made it."""

    def __enter__(self):
        global _LIB_PATH
        self._saved = _LIB_PATH
        _LIB_PATH = _DEV_LIB_PATH
        L = load()
        assert L.prt_dev_hooks() == 1
        return L

    def __exit__(self, *exc):
        global _LIB_PATH
        _LIB_PATH = self._saved
        return False


def last_render_form(L=None):
    """prt_last_render_form of `L` (default: the current library): which form of the render kernel the library's last K3
    launch used — _abi.RENDER_FORM_PLAIN or RENDER_FORM_GENERIC; RENDER_FORM_UNKNOWN from the shipped library, which keeps no
    record, and before the first launch."""
    return int((L or load()).prt_last_render_form())


def last_render_subform(L=None):
    """prt_last_render_subform of `L` (default: the current library): _abi.RENDER_SUBFORM_DIFFUSE when the last K3 launch was the
    DIFFUSE form of the PLAIN kernel (an all-Lambertian scene), RENDER_SUBFORM_NONE for every other launch; RENDER_SUBFORM_UNKNOWN
    from the shipped library and before the first launch."""
    return int((L or load()).prt_last_render_subform())


def shutdown():
    """prt_shutdown of every library loaded so far (cached RCCL communicators)."""
    for L in _libs.values():
        L.prt_shutdown()


def _check(rc, L=None):
    if rc != 0:
        raise PrtError(rc, (L or load()).prt_last_error().decode("utf-8", "replace"))


def _f64(a, k):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, k)


def denoise_params(L=None, guided=False, **params):
    """A PrtDenoiseParams: prt_denoise_defaults (guided: prt_denoise_guided_defaults), then the given fields (iterations,
    demodulate, sigma_color, sigma_normal, sigma_depth, sigma_albedo, feature_spp)."""
    p = _abi.PrtDenoiseParams()
    L = L or load()
    (L.prt_denoise_guided_defaults if guided else L.prt_denoise_defaults)(C.byref(p))
    names = {f for f, _ in _abi.PrtDenoiseParams._fields_} - {"reserved"}
    for k, v in params.items():
        if k not in names:
            raise TypeError(f"denoise: unknown parameter {k!r}")
        setattr(p, k, int(v) if k in ("iterations", "demodulate", "feature_spp") else float(v))
    return p


def denoise_defaults():
    """prt_denoise_defaults as a dict."""
    p = denoise_params()
    return {f: getattr(p, f) for f, _ in _abi.PrtDenoiseParams._fields_ if f != "reserved"}


def denoise_guided_defaults():
    """prt_denoise_guided_defaults as a dict."""
    p = denoise_params(guided=True)
    return {f: getattr(p, f) for f, _ in _abi.PrtDenoiseParams._fields_ if f != "reserved"}


def device_count():
    n = C.c_int(0)
    rc = load().prt_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class Scene:
    """A scene handle: host-side preparation at construction, `upload(device)` before any compute."""

    def __init__(self, scene_data, device_bvh=False):
        self.data = scene_data
        L = self._L = load()
        desc, keep = _abi.marshal_scene(scene_data)
        if device_bvh:
            desc.flags = _abi.PRT_SCENE_DEVICE_BVH  # tree built on the GPU in upload()
        h = C.c_void_p()
        _check(L.prt_scene_create(C.byref(desc), C.byref(h)), L)
        del keep  # the library copies everything it needs during create
        self._h = h
        self.device = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.prt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, device=0):
        _check(self._L.prt_scene_upload(self._h, device), self._L)
        self.device = device
        return self

    def update_vertices(self, vertices, normals=None):
        """New positions for the same triangles; an uploaded scene rebuilds its BVH on the GPU."""
        v = np.ascontiguousarray(vertices, dtype=np.float64)
        assert v.shape == self.data.vertices.shape
        n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float64)
        _check(self._L.prt_scene_update_vertices(self._h, v.ctypes.data, None if n is None else n.ctypes.data), self._L)
        return self

    def _refit_array(self, a, what, who="refit"):
        """A caller's positions (or normals) as the C call wants them; shape and dtype errors are raised here, before any call."""
        if not isinstance(a, np.ndarray):
            raise TypeError(f"{who}: {what} must be a numpy array, not {type(a).__name__}")
        if a.dtype != np.float64:
            raise TypeError(f"{who}: {what} must be float64, not {a.dtype}")
        if a.shape != self.data.vertices.shape:
            raise ValueError(f"{who}: {what} must have shape {self.data.vertices.shape}, not {a.shape}")
        return np.ascontiguousarray(a)

    def _positions_call(self, fn, who, vertices, normals):
        v = self._refit_array(vertices, "vertices", who)
        n = None if normals is None else self._refit_array(normals, "normals", who)
        _check(fn(self._h, v.ctypes.data, None if n is None else n.ctypes.data), self._L)
        return self

    def _positions_call_device(self, fn, who, d_vertices_ptr, d_normals_ptr, stream):
        for name, p in (("d_vertices_ptr", d_vertices_ptr), ("d_normals_ptr", d_normals_ptr), ("stream", stream)):
            if isinstance(p, bool) or not (p is None or isinstance(p, (int, np.integer))):
                raise TypeError(f"{who}: {name} must be an integer address or None, not {type(p).__name__}")
        if not d_vertices_ptr and self.data.vertices.shape[0]:
            raise ValueError(f"{who}: d_vertices_ptr is null")
        _check(fn(self._h, int(d_vertices_ptr or 0) or None, int(d_normals_ptr or 0) or None, int(stream or 0) or None), self._L)
        return self

    def refit(self, vertices, normals=None):
        """New positions for the same triangles of an uploaded scene, in place: the records and the BVH's boxes follow on the
        GPU, the tree keeps its topology and nothing is reloaded (prt_scene_refit).  Emitters must stay where they are unless
        `dynamic_lights` is on."""
        return self._positions_call(self._L.prt_scene_refit, "refit", vertices, normals)

    def refit_device(self, d_vertices_ptr, d_normals_ptr=None, stream=None):
        """The same from device memory: raw pointers to [n_tris][3][3] float64 arrays on the scene's device (e.g.
        tensor.data_ptr() of a contiguous float64 tensor), asynchronous on `stream` after one small read-back.  The host
        copy of the geometry goes stale: upload() is refused until update_vertices() or refit() has replaced every position."""
        return self._positions_call_device(self._L.prt_scene_refit_device, "refit_device", d_vertices_ptr, d_normals_ptr, stream)

    def rebuild(self, vertices, normals=None):
        """New positions as for refit(), and a NEW tree of them from the device builder (prt_scene_rebuild): what a refitted
        tree has lost (refit_info()["sah_ratio"]) comes back, while textures, materials and light tables stay resident.
        Synchronous.  Emitters must stay where they are unless `dynamic_lights` is on."""
        return self._positions_call(self._L.prt_scene_rebuild, "rebuild", vertices, normals)

    def rebuild_device(self, d_vertices_ptr, d_normals_ptr=None, stream=None):
        """The same from device memory (the arguments of refit_device): the kernels run on `stream`, the call returns when the
        new tree is resident.  The host copy of the geometry goes stale as after refit_device."""
        return self._positions_call_device(self._L.prt_scene_rebuild_device, "rebuild_device", d_vertices_ptr, d_normals_ptr, stream)

    def refit_info(self):
        """PrtRefitInfo as a dict: refits since the upload, the last one's hipEvent times, the grid, sah_ratio (synchronous)."""
        b = _abi.PrtRefitInfo()
        _check(self._L.prt_scene_refit_info(self._h, C.byref(b)), self._L)
        out = {f: getattr(b, f) for f, _ in _abi.PrtRefitInfo._fields_}
        out["grid_origin"], out["grid_step"] = tuple(b.grid_origin), tuple(b.grid_step)
        return out

    def bvh_info(self):
        b = _abi.PrtBvhInfo()
        _check(self._L.prt_scene_bvh_info(self._h, C.byref(b)), self._L)
        return {f: getattr(b, f) for f, _ in _abi.PrtBvhInfo._fields_}

    def light_order(self):
        n = C.c_uint64(0)
        _check(self._L.prt_scene_light_count(self._h, C.byref(n)), self._L)
        out = np.zeros(n.value, dtype=np.int32)
        _check(self._L.prt_scene_light_order(self._h, out.ctypes.data, n.value), self._L)
        return out

    @property
    def dynamic_lights(self):
        """Whether refit* / rebuild* accept a moved emitter (prt_scene_set_dynamic_lights): off by default; on, the light
        tree, its records and its O(1) tables follow the new positions on the device."""
        on = C.c_int(0)
        _check(self._L.prt_scene_get_dynamic_lights(self._h, C.byref(on)), self._L)
        return bool(on.value)

    @dynamic_lights.setter
    def dynamic_lights(self, on):
        _check(self._L.prt_scene_set_dynamic_lights(self._h, int(bool(on))), self._L)

    def light_update_info(self):
        """PrtLightUpdateInfo as a dict: light updates since the upload, the last one's times and outcome (synchronous)."""
        b = _abi.PrtLightUpdateInfo()
        _check(self._L.prt_scene_light_update_info(self._h, C.byref(b)), self._L)
        return {f: getattr(b, f) for f, _ in _abi.PrtLightUpdateInfo._fields_}

    def light_table_words(self):
        """The resident O(1) light-table words as a uint32 array, read back from the device (empty: no tables)."""
        n = C.c_uint64(0)
        _check(self._L.prt_scene_light_table_words(self._h, None, 0, C.byref(n)), self._L)
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check(self._L.prt_scene_light_table_words(self._h, out.ctypes.data, n.value, C.byref(n)), self._L)
        return out

    def trace_closest(self, rays, count_work=False):
        rays = np.ascontiguousarray(rays, dtype=_abi.RAY_DTYPE)
        hits = np.zeros(rays.shape[0], dtype=_abi.HIT_DTYPE)
        _check(self._L.prt_trace_closest(self._h, rays.ctypes.data, rays.shape[0], hits.ctypes.data, int(count_work)), self._L)
        return hits

    def trace_closest_device(self, d_rays_ptr, n, d_hits_ptr, count_work=False, stream=None, precision=0, sort=False):
        """K1 on device buffers; precision = _abi.PRECISION_F64 (default) or PRECISION_F32 (fp32 fast mode).  sort=True: K4
        first — the batch is traced in a locality order (same hits, for scenes that do not fit the caches)."""
        fn = self._L.prt_trace_closest_sorted_device if sort else self._L.prt_trace_closest_device_prec
        _check(fn(self._h, d_rays_ptr, n, d_hits_ptr, int(count_work), int(precision), stream))

    def trace_occluded(self, rays, count_work=False):
        """Any-hit query: uint8 [n], 1 where some triangle lies in the ray's [tmin, tmax] (== trace_closest's prim >= 0)."""
        rays = np.ascontiguousarray(rays, dtype=_abi.RAY_DTYPE)
        occ = np.zeros(rays.shape[0], dtype=np.uint8)
        _check(self._L.prt_trace_occluded(self._h, rays.ctypes.data, rays.shape[0], occ.ctypes.data, int(count_work)), self._L)
        return occ

    def trace_occluded_device(self, d_rays_ptr, n, d_out_ptr, count_work=False, stream=None, precision=0, sort=False):
        """The any-hit kernel on device buffers: one byte per ray into d_out_ptr; precision and sort as trace_closest_device."""
        fn = self._L.prt_trace_occluded_sorted_device if sort else self._L.prt_trace_occluded_device
        _check(fn(self._h, d_rays_ptr, n, d_out_ptr, int(count_work), int(precision), stream))

    def trace_surface(self, rays, count_work=False):
        """Surface query: a SURFACE_DTYPE array [n] — trace_closest's hit record followed by position, face-forwarded normal,
        tangent, uv, the material's albedo and emission and its index and type (all zero / -1 on a miss)."""
        rays = np.ascontiguousarray(rays, dtype=_abi.RAY_DTYPE)
        out = np.zeros(rays.shape[0], dtype=_abi.SURFACE_DTYPE)
        _check(self._L.prt_trace_surface(self._h, rays.ctypes.data, rays.shape[0], out.ctypes.data, int(count_work)), self._L)
        return out

    def trace_surface_device(self, d_rays_ptr, n, d_out_ptr, count_work=False, stream=None, precision=0, sort=False):
        """The surface kernel on device buffers: one 192-byte PrtSurface per ray into d_out_ptr (32-byte aligned); precision
        and sort as trace_closest_device."""
        fn = self._L.prt_trace_surface_sorted_device if sort else self._L.prt_trace_surface_device
        _check(fn(self._h, d_rays_ptr, n, d_out_ptr, int(count_work), int(precision), stream), self._L)

    def trace_multi(self, rays, k, after=None, count_work=False):
        """Multi-hit query (prt_trace_multi): the first k hits along each ray in ascending (t, prim), as an (n, k) array of
        HIT_DTYPE; slots past a ray's last hit hold the miss record (t = inf, prim = -1).  `after`: None, or an (n,)
        HIT_CURSOR_DTYPE array - only hits after (t, prim) of a ray's cursor are reported; feeding back the last hit of a
        page (its t and prim) gives the next page.  Shape and dtype errors are raised here, before any call."""
        if not isinstance(rays, np.ndarray):
            raise TypeError(f"trace_multi: rays must be a numpy array, not {type(rays).__name__}")
        if rays.dtype != _abi.RAY_DTYPE:
            raise TypeError(f"trace_multi: rays must have RAY_DTYPE, not {rays.dtype}")
        if rays.ndim != 1:
            raise ValueError(f"trace_multi: rays must have shape (n,), not {rays.shape}")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"trace_multi: k must be an integer, not {type(k).__name__}")
        if not 1 <= k <= _abi.MULTI_HIT_MAX:
            raise ValueError(f"trace_multi: k must be 1..{_abi.MULTI_HIT_MAX}, not {k}")
        n = rays.shape[0]
        if after is not None:
            if not isinstance(after, np.ndarray):
                raise TypeError(f"trace_multi: after must be a numpy array, not {type(after).__name__}")
            if after.dtype != _abi.HIT_CURSOR_DTYPE:
                raise TypeError(f"trace_multi: after must have HIT_CURSOR_DTYPE, not {after.dtype}")
            if after.shape != (n,):
                raise ValueError(f"trace_multi: after must have shape ({n},), not {after.shape}")
            after = np.ascontiguousarray(after)
        rays = np.ascontiguousarray(rays)
        hits = np.zeros((n, int(k)), dtype=_abi.HIT_DTYPE)
        _check(self._L.prt_trace_multi(self._h, rays.ctypes.data, None if after is None else after.ctypes.data, n, int(k),
                                       hits.ctypes.data, int(count_work)), self._L)
        return hits

    def trace_multi_device(self, d_rays_ptr, n, k, d_hits_ptr, d_after_ptr=None, count_work=False, precision=0, sort=False,
                           stream=None):
        """The multi-hit kernel on device buffers (raw pointers: n PrtRay, n * k PrtHit 32-byte aligned, n PrtHitCursor or
        None); precision and sort as trace_closest_device.  Cursors are not checked on the host."""
        fn = self._L.prt_trace_multi_sorted_device if sort else self._L.prt_trace_multi_device
        _check(fn(self._h, d_rays_ptr, d_after_ptr, int(n), int(k), d_hits_ptr, int(count_work), int(precision), stream), self._L)

    @property
    def distance_queries(self):
        """Whether the scene answers closest_point* (prt_scene_set_distance_queries): off by default; on, an uploaded scene
        keeps the fp64 corners of every triangle on the device (96 bytes each) and upload / refit* / rebuild* keep them in
        step.  Switching on after refit_device / rebuild_device moved the geometry past the host copy is refused."""
        on = C.c_int(0)
        _check(self._L.prt_scene_get_distance_queries(self._h, C.byref(on)), self._L)
        return bool(on.value)

    @distance_queries.setter
    def distance_queries(self, on):
        _check(self._L.prt_scene_set_distance_queries(self._h, int(bool(on))), self._L)

    def closest_point(self, points, max_dist=np.inf, count_work=False):
        """Closest-point query (prt_closest_point): points (n, 3) float64, max_dist a scalar or (n,) search radius.  Returns a
        CLOSEST_POINT_DTYPE array [n]: dist, the nearest point of the mesh, its barycentrics, prim, feature (0 face, 1-3
        edge, 4-6 vertex) and side; dist = inf and prim = -1 where no triangle lies within max_dist.  Shape and dtype errors
        are raised here, before any call."""
        q = _point_queries("closest_point", points, max_dist)
        n = q.shape[0]
        out = np.zeros(n, dtype=_abi.CLOSEST_POINT_DTYPE)
        _check(self._L.prt_closest_point(self._h, q.ctypes.data, n, out.ctypes.data, int(count_work)), self._L)
        return out

    def closest_point_device(self, d_q_ptr, n, d_out_ptr, count_work=False, stream=None):
        """prt_closest_point_device: asynchronous, on device buffers (raw pointers: n PrtPointQuery of 32 bytes, n
        PrtClosestPoint of 64 bytes, 32-byte aligned).  The queries are not checked on the host."""
        _check(self._L.prt_closest_point_device(self._h, d_q_ptr, int(n), d_out_ptr, int(count_work), stream), self._L)

    @property
    def signed_queries(self):
        """Whether the scene answers signed_distance* (prt_scene_set_signed_queries): off by default; switching on also
        switches distance_queries on, and an uploaded scene then keeps the welded topology's ids and the angle-weighted
        pseudonormals of every vertex and edge on the device; refit* / rebuild* refresh the pseudonormals."""
        on = C.c_int(0)
        _check(self._L.prt_scene_get_signed_queries(self._h, C.byref(on)), self._L)
        return bool(on.value)

    @signed_queries.setter
    def signed_queries(self, on):
        _check(self._L.prt_scene_set_signed_queries(self._h, int(bool(on))), self._L)

    def topology_info(self):
        """prt_scene_topology_info as a dict: what welding the whole scene's corners found (works without a device)."""
        info = _abi.PrtTopologyInfo()
        _check(self._L.prt_scene_topology_info(self._h, C.byref(info)), self._L)
        return {f: int(getattr(info, f)) for f, _ in _abi.PrtTopologyInfo._fields_ if f != "reserved"}

    def pseudonormals(self):
        """prt_scene_pseudonormals: float64 [n_tris, 6, 3] - per triangle the (unnormalised) pseudonormals of its edges
        v0v1, v1v2, v2v0 and vertices v0, v1, v2 as the device holds them; zeros for a slot without an id."""
        n = C.c_uint64(0)
        out = np.zeros((int(np.asarray(self.data.vertices).shape[0]), 6, 3), dtype=np.float64)
        _check(self._L.prt_scene_pseudonormals(self._h, out.ctypes.data, out.shape[0], C.byref(n)), self._L)
        assert n.value == out.shape[0]
        return out

    def signed_distance(self, points, max_dist=np.inf, count_work=False):
        """Signed distance query (prt_signed_distance): arguments as closest_point.  Returns a SIGNED_DISTANCE_DTYPE array
        [n]: closest_point's record with sdist = sign * dist in place of dist and sign in place of reserved; sign is that of
        dot(N, p - point) with N the angle-weighted pseudonormal of the nearest feature (-1: inside a closed mesh)."""
        q = _point_queries("signed_distance", points, max_dist)
        out = np.zeros(q.shape[0], dtype=_abi.SIGNED_DISTANCE_DTYPE)
        _check(self._L.prt_signed_distance(self._h, q.ctypes.data, q.shape[0], out.ctypes.data, int(count_work)), self._L)
        return out

    def signed_distance_device(self, d_q_ptr, n, d_out_ptr, count_work=False, stream=None):
        """prt_signed_distance_device: asynchronous, on device buffers (n PrtPointQuery, n PrtSignedDistance of 64 bytes,
        32-byte aligned).  The queries are not checked on the host."""
        _check(self._L.prt_signed_distance_device(self._h, d_q_ptr, int(n), d_out_ptr, int(count_work), stream), self._L)

    @property
    def winding_queries(self):
        """Whether the scene answers winding_number* (prt_scene_set_winding_queries): off by default; switching on also
        switches distance_queries on, and an uploaded scene then keeps four 64-byte moment records per tree node on the
        device; refit* refresh them, rebuild* make the new tree's."""
        on = C.c_int(0)
        _check(self._L.prt_scene_get_winding_queries(self._h, C.byref(on)), self._L)
        return bool(on.value)

    @winding_queries.setter
    def winding_queries(self, on):
        _check(self._L.prt_scene_set_winding_queries(self._h, int(bool(on))), self._L)

    def winding_moments(self):
        """prt_scene_winding_moments: float64 [n_nodes, 4, 8] - per child slot of every node of the resident tree the record
        N[3], c[3], r, A as the device holds it; zeros for an unused slot."""
        n = C.c_uint64(0)
        _check(self._L.prt_scene_winding_moments(self._h, None, 0, C.byref(n)), self._L)
        out = np.zeros((int(n.value), 4, 8), dtype=np.float64)
        _check(self._L.prt_scene_winding_moments(self._h, out.ctypes.data, out.shape[0], C.byref(n)), self._L)
        assert n.value == out.shape[0]
        return out

    def winding_number(self, points, beta=2.0, count_work=False):
        """Generalized winding number of each point (prt_winding_number): points float64 (n, 3).  Returns float64 [n]: ~1
        inside a closed mesh whose faces are counter-clockwise seen from outside, ~0 outside, in between across holes.
        beta > 1 trades error for work; beta = inf is the exact sum over every triangle.  The value depends on the tree."""
        q = _point_queries("winding_number", points, 0.0)
        out = np.zeros(q.shape[0], dtype=np.float64)
        _check(self._L.prt_winding_number(self._h, q.ctypes.data, q.shape[0], float(beta), out.ctypes.data, int(count_work)), self._L)
        return out

    def winding_number_device(self, d_q_ptr, n, d_out_ptr, beta=2.0, count_work=False, stream=None):
        """prt_winding_number_device: asynchronous, on device buffers (n PrtPointQuery, n doubles).  The queries are not
        checked on the host."""
        _check(self._L.prt_winding_number_device(self._h, d_q_ptr, int(n), float(beta), d_out_ptr, int(count_work), stream), self._L)

    def inside(self, points, beta=2.0):
        """winding_number(points, beta) > 0.5."""
        return self.winding_number(points, beta) > 0.5

    def sample_lights(self, origins, seed=1):
        origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(origins.shape[0], dtype=_abi.LIGHT_SAMPLE_DTYPE)
        _check(self._L.prt_sample_lights(self._h, origins.ctypes.data, origins.shape[0], seed, out.ctypes.data), self._L)
        return out

    # ---- test hooks for the material arithmetic (include/prt.h)
    def material_eval(self, material, wi, wo, uv=None, seed=1):
        wi, wo = _f64(wi, 3), _f64(wo, 3)
        uv = None if uv is None else _f64(uv, 2)
        out = np.zeros_like(wi)
        _check(self._L.prt_material_eval(self._h, material, wi.shape[0], wi.ctypes.data, wo.ctypes.data,
                                        None if uv is None else uv.ctypes.data, seed, out.ctypes.data), self._L)
        return out

    def material_scatter(self, material, rd, normal=(0, 0, 1), tangent=(1, 0, 0), uv=None, seed=1):
        rd = _f64(rd, 3)
        uv = None if uv is None else _f64(uv, 2)
        nrm, tan = _f64(normal, 3), _f64(tangent, 3)
        wi, att, ok = np.zeros_like(rd), np.zeros_like(rd), np.zeros(rd.shape[0], dtype=np.int32)
        _check(self._L.prt_material_scatter(self._h, material, rd.shape[0], rd.ctypes.data, nrm.ctypes.data, tan.ctypes.data,
                                           None if uv is None else uv.ctypes.data, seed, wi.ctypes.data, att.ctypes.data,
                                           ok.ctypes.data), self._L)
        return wi, att, ok.astype(bool)

    def texture_value(self, texture, uv):
        uv = _f64(uv, 2)
        out = np.zeros((uv.shape[0], 3))
        _check(self._L.prt_texture_value(self._h, texture, uv.shape[0], uv.ctypes.data, out.ctypes.data), self._L)
        return out

    def render(self, camera=None, f32=False, **kw):
        """Render one frame to host memory.  Returns (H,W,3) float64 (and float32 if f32=True)."""
        cam = camera or self.data.camera
        c, p = _abi.make_camera(cam), _abi.make_params(**kw)
        out64 = np.zeros((cam.height, cam.width, 3), dtype=np.float64)
        out32 = np.zeros((cam.height, cam.width, 3), dtype=np.float32) if f32 else None
        _check(self._L.prt_render(self._h, C.byref(c), C.byref(p), out64.ctypes.data,
                                 out32.ctypes.data if f32 else None), self._L)
        return (out64, out32) if f32 else out64

    def render_samples(self, pixels_xy, camera=None, sample_begin=0, sample_count=None, trace=False, **kw):
        """RayColor of single camera samples through K3 (test hook, include/prt.h): (n_pixels, count, 3) float64 and, with
        trace=True, the paths' signatures (n_pixels, count, TRACE_WORDS) int32.  kw as for render(); spp = the default count."""
        cam = camera or self.data.camera
        c, p = _abi.make_camera(cam), _abi.make_params(**kw)
        count = p.spp if sample_count is None else int(sample_count)
        px = np.ascontiguousarray(pixels_xy, dtype=np.int32).reshape(-1, 2)
        out = np.zeros((px.shape[0], count, 3), dtype=np.float64)
        tr = np.zeros((px.shape[0], count, _abi.TRACE_WORDS), dtype=np.int32) if trace else None
        _check(self._L.prt_render_samples(self._h, C.byref(c), C.byref(p), px.ctypes.data, px.shape[0], int(sample_begin), count,
                                         out.ctypes.data, tr.ctypes.data if trace else None), self._L)
        return (out, tr) if trace else out

    def render_device(self, d_f64_ptr, d_f32_ptr, camera=None, count_work=False, stream=None, **kw):
        """Asynchronous render into device buffers (raw device pointers, e.g. torch tensor.data_ptr())."""
        cam = camera or self.data.camera
        c, p = _abi.make_camera(cam), _abi.make_params(**kw)
        _check(self._L.prt_render_device(self._h, C.byref(c), C.byref(p), d_f64_ptr, d_f32_ptr, int(count_work), stream), self._L)

    @staticmethod
    def _ray_color_params(kw):
        """PrtRenderParams of a ray batch: kw as for render(), plus `reserved` (the struct's reserved word, which must be 0)."""
        reserved = kw.pop("reserved", 0)
        p = _abi.make_params(**kw)
        p.reserved = int(reserved)
        return p

    def ray_color(self, rays, keys=None, sample_begin=0, f32=False, **kw):
        """RayColor of caller-supplied rays (prt_ray_color): rays a RAY_DTYPE array (o and d are read, d not normalised), keys
        an optional uint32 array — ray i's random streams are keyed (seed, keys[i] or i, s).  Returns (n, 3) float64, the mean
        over samples [sample_begin, sample_begin + spp) (and float32 if f32=True).  kw as for render(); tiles and ranks are
        ignored, pixel_jitter must be off."""
        rays = np.ascontiguousarray(rays, dtype=_abi.RAY_DTYPE).reshape(-1)
        n = rays.shape[0]
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
            if keys.shape[0] != n:
                raise ValueError(f"ray_color: {keys.shape[0]} keys for {n} rays")
        p = self._ray_color_params(kw)
        out64 = np.zeros((n, 3), dtype=np.float64)
        out32 = np.zeros((n, 3), dtype=np.float32) if f32 else None
        _check(self._L.prt_ray_color(self._h, rays.ctypes.data, None if keys is None else keys.ctypes.data, n, C.byref(p),
                                     int(sample_begin), out64.ctypes.data, out32.ctypes.data if f32 else None), self._L)
        return (out64, out32) if f32 else out64

    def ray_color_device(self, d_rays_ptr, n, d_f64_ptr, d_f32_ptr, d_keys_ptr=None, sample_begin=0, stream=None, **kw):
        """prt_ray_color_device: asynchronous, on device buffers (raw pointers: n PrtRay, optionally n uint32 keys, n triples of
        float64 and / or float32).  The rays are not checked: a non-finite or zero direction gives an unspecified result."""
        p = self._ray_color_params(kw)
        _check(self._L.prt_ray_color_device(self._h, d_rays_ptr, d_keys_ptr, int(n), C.byref(p), int(sample_begin), d_f64_ptr,
                                            d_f32_ptr, stream), self._L)

    def features(self, camera=None, feature_spp=1, **kw):
        """First-hit feature buffers (prt_render_features, include/prt.h): dict of albedo (H, W, 3) float32, normal (H, W, 3)
        float32, depth (H, W) float32 (+inf on a miss) and prim (H, W) int32 (-1 on a miss).  kw as for render()."""
        cam = camera or self.data.camera
        c, p = _abi.make_camera(cam), _abi.make_params(**kw)
        h, w = cam.height, cam.width
        out = {"albedo": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32),
               "depth": np.zeros((h, w), np.float32), "prim": np.zeros((h, w), np.int32)}
        _check(self._L.prt_render_features(self._h, C.byref(c), C.byref(p), int(feature_spp), out["albedo"].ctypes.data,
                                          out["normal"].ctypes.data, out["depth"].ctypes.data, out["prim"].ctypes.data), self._L)
        return out

    def features_device(self, d_albedo, d_normal, d_depth, d_prim, camera=None, feature_spp=1, stream=None, **kw):
        """prt_render_features_device: asynchronous, into device buffers (raw pointers; any may be None)."""
        cam = camera or self.data.camera
        c, p = _abi.make_camera(cam), _abi.make_params(**kw)
        _check(self._L.prt_render_features_device(self._h, C.byref(c), C.byref(p), int(feature_spp), d_albedo, d_normal, d_depth,
                                                 d_prim, stream), self._L)

    def denoise(self, rgb, features, **params):
        """The a-trous filter (prt_denoise) on host arrays: rgb (H, W, 3), features a dict with albedo (H, W, 3), normal
        (H, W, 3) and depth (H, W) (what features() returns).  params: fields of PrtDenoiseParams, else the defaults.
        Returns (H, W, 3) float32."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"denoise: rgb must have shape (H, W, 3), got {rgb.shape}")
        h, w = rgb.shape[:2]
        a = np.ascontiguousarray(features["albedo"], dtype=np.float32)
        n = np.ascontiguousarray(features["normal"], dtype=np.float32)
        z = np.ascontiguousarray(features["depth"], dtype=np.float32)
        if a.shape != rgb.shape or n.shape != rgb.shape or z.shape != rgb.shape[:2]:
            raise ValueError(f"denoise: feature shapes {a.shape} {n.shape} {z.shape} do not match rgb {rgb.shape}")
        p = denoise_params(self._L, **params)
        out = np.empty_like(rgb)
        _check(self._L.prt_denoise(self._h, w, h, rgb.ctypes.data, a.ctypes.data, n.ctypes.data, z.ctypes.data, C.byref(p),
                                  out.ctypes.data), self._L)
        return out

    def denoise_device(self, width, height, d_rgb, d_albedo, d_normal, d_depth, d_out, stream=None, **params):
        """prt_denoise_device: asynchronous, on device buffers (raw pointers)."""
        p = denoise_params(self._L, **params)
        _check(self._L.prt_denoise_device(self._h, int(width), int(height), d_rgb, d_albedo, d_normal, d_depth, C.byref(p), d_out,
                                         stream), self._L)

    def denoise_guided(self, rgb, variance, features, return_variance=False, **params):
        """The variance-guided a-trous filter (prt_denoise_guided) on host arrays: rgb and features as for denoise(), variance
        (H, W) the variance of each pixel's mean luminance (AdaptiveAccumulator.variance()).  params: fields of
        PrtDenoiseParams, else the guided defaults.  Returns (H, W, 3) float32, and with return_variance=True also the
        filtered variance (H, W) float32."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"denoise_guided: rgb must have shape (H, W, 3), got {rgb.shape}")
        h, w = rgb.shape[:2]
        v = np.ascontiguousarray(variance, dtype=np.float32)
        a = np.ascontiguousarray(features["albedo"], dtype=np.float32)
        n = np.ascontiguousarray(features["normal"], dtype=np.float32)
        z = np.ascontiguousarray(features["depth"], dtype=np.float32)
        if a.shape != rgb.shape or n.shape != rgb.shape or z.shape != rgb.shape[:2] or v.shape != rgb.shape[:2]:
            raise ValueError(f"denoise_guided: shapes {v.shape} {a.shape} {n.shape} {z.shape} do not match rgb {rgb.shape}")
        p = denoise_params(self._L, guided=True, **params)
        out = np.empty_like(rgb)
        vout = np.empty_like(v) if return_variance else None
        _check(self._L.prt_denoise_guided(self._h, w, h, rgb.ctypes.data, v.ctypes.data, a.ctypes.data, n.ctypes.data, z.ctypes.data,
                                         C.byref(p), out.ctypes.data, vout.ctypes.data if return_variance else None), self._L)
        return (out, vout) if return_variance else out

    def denoise_guided_device(self, width, height, d_rgb, d_variance, d_albedo, d_normal, d_depth, d_out, d_out_variance=None,
                              stream=None, **params):
        """prt_denoise_guided_device: asynchronous, on device buffers (raw pointers; d_out_variance may be None)."""
        p = denoise_params(self._L, guided=True, **params)
        _check(self._L.prt_denoise_guided_device(self._h, int(width), int(height), d_rgb, d_variance, d_albedo, d_normal, d_depth,
                                                C.byref(p), d_out, d_out_variance, stream), self._L)

    def tonemap_srgb8(self, d_f32_ptr, width, height, d_u8_ptr, stream=None):
        _check(self._L.prt_tonemap_srgb8(self._h, d_f32_ptr, width, height, d_u8_ptr, stream), self._L)

    def counters(self):
        c = _abi.PrtCounters()
        _check(self._L.prt_get_counters(self._h, C.byref(c)), self._L)
        return {f: getattr(c, f) for f, _ in _abi.PrtCounters._fields_}


class Accumulator:
    """Progressive, resumable rendering (prt_accum_*, include/prt.h): running fp64 sums of every sample rendered so far.
    After n samples, image() is Scene.render(spp=n) of the same camera and keywords (within ~1e-13: summation order).
    Keywords as for Scene.render, minus spp (the pass size is add()'s argument); they are frozen here.  Destroy (close, or
    leave the `with` block) before the scene is closed."""

    def __init__(self, scene, camera=None, **kw):
        if "spp" in kw:
            raise TypeError("Accumulator: spp is not a parameter (the pass size is add()'s argument)")
        self.scene = scene
        self._L = scene._L
        self.camera = camera or scene.data.camera
        self._shape = (self.camera.height, self.camera.width, 3)
        c, p = _abi.make_camera(self.camera), _abi.make_params(**kw)
        h = C.c_void_p()
        _check(self._L.prt_accum_create(scene._h, C.byref(c), C.byref(p), C.byref(h)), self._L)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.prt_accum_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, n, stream=None):
        """Asynchronous: render the next n samples of every owned pixel and add them to the sums."""
        if int(n) != n or n < 1:
            raise ValueError(f"Accumulator.add: n must be an integer >= 1, got {n!r}")
        _check(self._L.prt_accum_render(self._h, int(n), stream), self._L)
        return self

    @property
    def samples(self):
        n = C.c_uint64(0)
        _check(self._L.prt_accum_samples(self._h, C.byref(n)), self._L)
        return n.value

    def image(self, f32=False):
        """The frame of the samples so far: (H, W, 3) float64, or float32 with f32=True."""
        out = np.zeros(self._shape, dtype=np.float32 if f32 else np.float64)
        _check(self._L.prt_accum_read(self._h, None if f32 else out.ctypes.data, out.ctypes.data if f32 else None), self._L)
        return out

    def resolve(self, d_f64_ptr=None, d_f32_ptr=None, d_u8_ptr=None, stream=None):
        """Asynchronous resolve into device buffers (raw device pointers, e.g. torch tensor.data_ptr())."""
        _check(self._L.prt_accum_resolve(self._h, d_f64_ptr, d_f32_ptr, d_u8_ptr, stream), self._L)

    def srgb8(self):
        """The frame of the samples so far as 8-bit sRGB, (H, W, 3) uint8 (the bytes Scene.tonemap_srgb8 makes of image(f32=True))."""
        import torch
        dev = torch.device("cuda", self.scene.device or 0)
        d = torch.empty(self._shape, dtype=torch.uint8, device=dev)
        self.resolve(d_u8_ptr=d.data_ptr())
        torch.cuda.synchronize(dev)
        return d.cpu().numpy()

    def reset(self):
        _check(self._L.prt_accum_reset(self._h), self._L)
        return self

    def denoised(self, **params):
        """The frame of the samples so far, denoised (prt_accum_read_denoised): (H, W, 3) float32.  params: fields of
        PrtDenoiseParams, else the defaults.  The features are traced once with this accumulator's camera and keywords."""
        p = denoise_params(self._L, **params)
        out = np.zeros(self._shape, dtype=np.float32)
        _check(self._L.prt_accum_read_denoised(self._h, C.byref(p), out.ctypes.data), self._L)
        return out

    def resolve_denoised(self, d_f32_ptr=None, d_u8_ptr=None, stream=None, **params):
        """Asynchronous prt_accum_resolve_denoised into device buffers (raw pointers)."""
        p = denoise_params(self._L, **params)
        _check(self._L.prt_accum_resolve_denoised(self._h, C.byref(p), d_f32_ptr, d_u8_ptr, stream), self._L)

    def denoised_guided(self, **params):
        """The frame of the samples so far through the variance-guided filter (prt_accum_read_denoised_guided): (H, W, 3)
        float32.  params: fields of PrtDenoiseParams, else the guided defaults.  Adaptive accumulators only (a plain one keeps
        no moments: PrtError), after at least two batches."""
        p = denoise_params(self._L, guided=True, **params)
        out = np.zeros(self._shape, dtype=np.float32)
        _check(self._L.prt_accum_read_denoised_guided(self._h, C.byref(p), out.ctypes.data), self._L)
        return out

    def resolve_denoised_guided(self, d_f32_ptr=None, d_u8_ptr=None, stream=None, **params):
        """Asynchronous prt_accum_resolve_denoised_guided into device buffers (raw pointers)."""
        p = denoise_params(self._L, guided=True, **params)
        _check(self._L.prt_accum_resolve_denoised_guided(self._h, C.byref(p), d_f32_ptr, d_u8_ptr, stream), self._L)

    def variance(self, d_f32_ptr=None, stream=None):
        """The variance of each pixel's mean luminance from the batch-means moments (prt_accum_read_variance): (H, W) float32,
        0 where the pixel has no samples.  With d_f32_ptr: asynchronous prt_accum_variance into that device buffer instead.
        Adaptive accumulators only, after at least two batches."""
        if d_f32_ptr is not None:
            _check(self._L.prt_accum_variance(self._h, d_f32_ptr, stream), self._L)
            return None
        out = np.zeros(self._shape[:2], dtype=np.float32)
        _check(self._L.prt_accum_read_variance(self._h, out.ctypes.data), self._L)
        return out

    def state(self):
        """Checkpoint: (sums (H, W, 3) float64, samples, fingerprint)."""
        sums = np.zeros(self._shape, dtype=np.float64)
        n, fp = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.prt_accum_export(self._h, sums.ctypes.data, C.byref(n), C.byref(fp)), self._L)
        return sums, n.value, fp.value

    def restore(self, sums, samples, fingerprint):
        """Resume from state() of an accumulator with the same camera, keywords and scene counts (another process or scene)."""
        sums = np.asarray(sums)
        if sums.shape != self._shape:
            raise ValueError(f"Accumulator.restore: sums must have shape {self._shape}, got {sums.shape}")
        if int(samples) != samples or samples < 0:
            raise ValueError(f"Accumulator.restore: samples must be an integer >= 0, got {samples!r}")
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        _check(self._L.prt_accum_import(self._h, sums.ctypes.data, int(samples), int(fingerprint)), self._L)
        return self


class AdaptiveAccumulator(Accumulator):
    """Adaptive sampling (prt_accum_create_adaptive, include/prt.h): each pixel gets samples, in rounds, until its own
    batch-means noise estimate se <= max(rel_tol * |mean|, abs_tol), never fewer than min_spp and never more than max_spp.
    A pixel that stopped after n_p samples holds Scene.render(spp=n_p)'s value there.  batch = samples per batch (0: the
    library's default, _abi.ADAPTIVE_DEFAULT_BATCH); min_spp, max_spp and every round size are multiples of it.  Other
    keywords as for Accumulator.  add(), state() and restore() are refused: use step(), export() and load()."""

    def __init__(self, scene, camera=None, *, rel_tol, abs_tol, min_spp, max_spp, batch=0, **kw):
        if "spp" in kw:
            raise TypeError("AdaptiveAccumulator: spp is not a parameter (max_spp bounds every pixel)")
        self.scene = scene
        self._L = scene._L
        self.camera = camera or scene.data.camera
        self._shape = (self.camera.height, self.camera.width, 3)
        c, p = _abi.make_camera(self.camera), _abi.make_params(**kw)
        a = _abi.PrtAdaptiveParams(int(min_spp), int(max_spp), int(batch), 0, float(rel_tol), float(abs_tol))
        self.batch = int(batch) or _abi.ADAPTIVE_DEFAULT_BATCH
        self.min_spp, self.max_spp, self.rel_tol, self.abs_tol = int(min_spp), int(max_spp), float(rel_tol), float(abs_tol)
        h = C.c_void_p()
        _check(self._L.prt_accum_create_adaptive(scene._h, C.byref(c), C.byref(p), C.byref(a), C.byref(h)), self._L)
        self._h = h

    def step(self, n, stream=None):
        """One round of n samples (a multiple of batch) for every active pixel; returns the number of pixels rendered
        (0: every pixel has stopped).  Reads one word back from the device; the rendering itself is asynchronous."""
        if int(n) != n or n < 1:
            raise ValueError(f"AdaptiveAccumulator.step: n must be an integer >= 1, got {n!r}")
        k = C.c_uint64(0)
        _check(self._L.prt_accum_render_adaptive(self._h, int(n), C.byref(k), stream), self._L)
        return k.value

    def run(self, n_per_round, on_round=None):
        """Rounds of n_per_round samples until no pixel is active; returns the number of rounds that rendered.
        on_round(n_active, n_per_round) is called after every round that rendered."""
        rounds = 0
        while True:
            k = self.step(n_per_round)
            if k == 0:
                return rounds
            rounds += 1
            if on_round is not None:
                on_round(k, n_per_round)

    def pixel_samples(self):
        """Samples per pixel, (H, W) uint32."""
        out = np.zeros(self._shape[:2], dtype=np.uint32)
        _check(self._L.prt_accum_pixel_samples(self._h, out.ctypes.data), self._L)
        return out

    def export(self):
        """Checkpoint: dict of sums (H, W, 3) float64, moments (H, W) float64, counts (H, W) uint32, samples, fingerprint."""
        sums = np.zeros(self._shape, dtype=np.float64)
        mom = np.zeros(self._shape[:2], dtype=np.float64)
        cnt = np.zeros(self._shape[:2], dtype=np.uint32)
        n, fp = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.prt_accum_export_adaptive(self._h, sums.ctypes.data, mom.ctypes.data, cnt.ctypes.data, C.byref(n),
                                                 C.byref(fp)), self._L)
        return {"sums": sums, "moments": mom, "counts": cnt, "samples": n.value, "fingerprint": fp.value}

    def load(self, state):
        """Resume from export() of an adaptive accumulator with the same camera, keywords, adaptive parameters and scene counts."""
        sums = np.asarray(state["sums"])
        mom, cnt = np.asarray(state["moments"]), np.asarray(state["counts"])
        if sums.shape != self._shape or mom.shape != self._shape[:2] or cnt.shape != self._shape[:2]:
            raise ValueError(f"AdaptiveAccumulator.load: shapes {sums.shape} {mom.shape} {cnt.shape}, want {self._shape} and {self._shape[:2]}")
        if cnt.dtype != np.uint32 and (cnt.min(initial=0) < 0 or cnt.max(initial=0) > 0xFFFFFFFF):
            raise ValueError("AdaptiveAccumulator.load: counts out of uint32 range")
        samples = state["samples"]
        if int(samples) != samples or samples < 0:
            raise ValueError(f"AdaptiveAccumulator.load: samples must be an integer >= 0, got {samples!r}")
        sums = np.ascontiguousarray(sums, dtype=np.float64)
        mom = np.ascontiguousarray(mom, dtype=np.float64)
        cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
        _check(self._L.prt_accum_import_adaptive(self._h, sums.ctypes.data, mom.ctypes.data, cnt.ctypes.data, int(samples),
                                                 int(state["fingerprint"])), self._L)
        return self


def render_multi(scene_list, camera=None, **kw):
    """prt_render_multi: one frame over several uploaded replicas of a scene (different GPUs: tiles + one RCCL reduce of the
    fp32 framebuffer; one GPU: tile shares summed on it).  Returns (H, W, 3) float32."""
    cam = camera or scene_list[0].data.camera
    c, p = _abi.make_camera(cam), _abi.make_params(**kw)
    hs = (C.c_void_p * len(scene_list))(*[s._h for s in scene_list])
    out = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
    L = scene_list[0]._L
    _check(L.prt_render_multi(hs, len(scene_list), C.byref(c), C.byref(p), out.ctypes.data), L)
    return out
