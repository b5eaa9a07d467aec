"""ctypes binding of the C-ABI in include/wtgpu.h (libwtgpu.so).  No compute happens in Python."""
import ctypes as C
import json
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))

# The renderer pipelines batches over several HIP streams.  The ROCm runtime stages by-value kernel arguments in a 1 MiB ring per
# stream: a batch enqueues ~1000 launches of ~1 KB, a full ring blocks the enqueueing thread until the GPU catches up, and the internal
# streams serialise behind it (measured: enqueue 209 ms -> 16 ms per pass).  The variable is read when the HIP runtime initialises, i.e.
# it only takes effect if this package is imported BEFORE torch (bench.py sets it itself).
os.environ.setdefault("HSA_KERNARG_POOL_SIZE", str(16 << 20))


def lib_path():
    # WTGPU_LIB: an alternative build of the library (A/B experiments with compile-time knobs)
    return os.environ.get("WTGPU_LIB") or os.path.join(_HERE, "libwtgpu.so")


class WtgpuError(RuntimeError):
    pass


class SceneParams(C.Structure):
    _fields_ = [("res", C.c_uint32), ("max_depth", C.c_int32), ("fsd", C.c_int32), ("mis", C.c_int32), ("rr", C.c_int32),
                ("force_ray_tracing", C.c_int32), ("mesh_detail", C.c_int32), ("lut_n_theta", C.c_uint32), ("lut_m", C.c_uint32),
                ("polarimetric", C.c_int32)]


class TestHooks(C.Structure):      # wave_tracer_amd/csrc/wtgpu_test_hooks.h (not part of the public C-ABI)
    _fields_ = [("only_s", C.c_uint32), ("only_t", C.c_uint32), ("crop_of", C.c_uint32)]


class SensorMaskSpec(C.Structure):   # wtgpu_sensor_mask_spec
    _fields_ = [("present", C.c_int32), ("samples", C.c_uint32), ("regex", C.c_char_p), ("shape_flags", C.POINTER(C.c_uint8)),
                ("n_shapes", C.c_uint32)]


class FirstHitSpec(C.Structure):     # wtgpu_first_hit_spec
    _fields_ = [("samples", C.c_uint32), ("maps", C.c_uint32), ("ids", C.c_uint32), ("pad", C.c_uint32), ("seed", C.c_uint64)]


class FirstHitMaterialSpec(C.Structure):   # wtgpu_first_hit_material_spec
    _fields_ = [("samples", C.c_uint32), ("maps", C.c_uint32), ("ids", C.c_uint32), ("n_k", C.c_uint32), ("k", C.c_float * 4), ("seed", C.c_uint64)]


class LosSpec(C.Structure):          # wtgpu_los_spec
    _fields_ = [("samples", C.c_uint32), ("maps", C.c_uint32), ("elem", C.c_uint32), ("ids", C.c_uint32), ("flags", C.c_uint32), ("n_emitters", C.c_uint32),
                ("emitters", C.c_uint32 * 32), ("t_min", C.c_float), ("pad", C.c_uint32), ("seed", C.c_uint64)]


class TonemapSpec(C.Structure):      # wtgpu_tonemap_spec
    _fields_ = [("present", C.c_int32), ("op", C.c_int32), ("mode", C.c_int32), ("gamma", C.c_float), ("db_min", C.c_float), ("db_max", C.c_float),
                ("colourmap", C.c_char_p), ("function", C.c_char_p)]


class Tonemap(C.Structure):          # wtgpu_tonemap
    _fields_ = [("op", C.c_int32), ("mode", C.c_int32), ("gamma", C.c_float), ("db_min", C.c_float), ("db_max", C.c_float),
                ("table", C.POINTER(C.c_float)), ("table_n", C.c_uint32)]


class FilmSource(C.Structure):       # wtgpu_film_source: the accumulators with spe, or a developed f32 film
    _fields_ = [("value", C.c_void_p), ("weight", C.c_void_p), ("light", C.c_void_p), ("spe", C.c_uint64), ("developed", C.c_void_p)]


class FilmStatsSpec(C.Structure):    # wtgpu_film_stats_spec
    _fields_ = [("stokes_component", C.c_uint32), ("scale", C.c_uint32), ("bins", C.c_uint32), ("flags", C.c_uint32), ("lo", C.c_float), ("hi", C.c_float)]


class FilmStats(C.Structure):        # wtgpu_film_stats
    _fields_ = [("n", C.c_uint64), ("n_nan", C.c_uint64), ("n_negative", C.c_uint64), ("n_zero", C.c_uint64), ("n_below", C.c_uint64), ("n_above", C.c_uint64),
                ("min", C.c_float), ("max", C.c_float), ("min_positive", C.c_float), ("pad", C.c_float), ("sum", C.c_double)]


class FilmZonalSpec(C.Structure):    # wtgpu_film_zonal_spec
    _fields_ = [("stokes_component", C.c_uint32), ("scale", C.c_uint32), ("bins", C.c_uint32), ("flags", C.c_uint32), ("n_zones", C.c_uint32), ("lo", C.c_float),
                ("hi", C.c_float)]


# wtgpu_film_zonal as a numpy record (72 bytes, no padding)
FILM_ZONAL_FIELDS = [("n", "<u8"), ("n_nan", "<u8"), ("n_inf", "<u8"), ("n_negative", "<u8"), ("n_zero", "<u8"), ("n_below", "<u8"), ("n_above", "<u8"),
                     ("min", "<f4"), ("max", "<f4"), ("sum", "<f8")]
FILM_ZONAL_MAX_ZONES = 65536
FILM_ZONAL_NO_ZONE = 0xFFFFFFFF


class FilmSegmentsSpec(C.Structure):  # wtgpu_film_segments_spec
    _fields_ = [("flags", C.c_uint32), ("min_area", C.c_uint32), ("max_records", C.c_uint32), ("pad", C.c_uint32)]


class FilmSegmentsInfo(C.Structure):  # wtgpu_film_segments_info
    _fields_ = [("n_segments", C.c_uint64), ("n_dropped", C.c_uint64), ("n_members", C.c_uint64), ("n_dropped_pixels", C.c_uint64)]


# wtgpu_film_segment as a numpy record (48 bytes, no padding)
FILM_SEGMENT_FIELDS = [("klass", "<u4"), ("area", "<u4"), ("first", "<u4"), ("x0", "<u4"), ("y0", "<u4"), ("x1", "<u4"), ("y1", "<u4"), ("pad", "<u4"),
                       ("sum_x", "<u8"), ("sum_y", "<u8")]
FILM_SEGMENTS_DIAGONAL = 1


class FilmDistanceSpec(C.Structure):  # wtgpu_film_distance_spec
    _fields_ = [("flags", C.c_uint32), ("pad", C.c_uint32 * 3)]


class FilmDistanceInfo(C.Structure):  # wtgpu_film_distance_info
    _fields_ = [("n_sites", C.c_uint64), ("argmax", C.c_uint64), ("max_dist2", C.c_uint32), ("pad", C.c_uint32)]


FILM_DISTANCE_INVERT = 1
FILM_DISTANCE_NONE = 0xFFFFFFFF   # dist2 and nearest where the plane holds no site
FILM_DISTANCE_MAX_SIDE = 32768    # wider or higher sensors are refused


class FilmCompareSpec(C.Structure):  # wtgpu_film_compare_spec
    _fields_ = [("stokes_component", C.c_uint32), ("flags", C.c_uint32), ("eps", C.c_double)]


FILM_COMPARE_FIELDS = [("n", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_nonfinite_mismatch", C.c_uint64), ("n_differ", C.c_uint64), ("argmax", C.c_uint64),
                       ("max_abs", C.c_double), ("sum_abs", C.c_double), ("sum_sq", C.c_double), ("sum_a_sq", C.c_double), ("sum_b_sq", C.c_double),
                       ("sum_rel", C.c_double)]


class FilmCompare(C.Structure):      # wtgpu_film_compare
    _fields_ = FILM_COMPARE_FIELDS


class FilmPolarSpec(C.Structure):    # wtgpu_film_polar_spec
    _fields_ = [("flags", C.c_uint32), ("maps", C.c_uint32), ("picture_plane", C.c_uint32), ("format", C.c_uint32), ("c2", C.c_double), ("s2", C.c_double),
                ("sat_gain", C.c_float), ("pad", C.c_float), ("tonemap", Tonemap)]


FILM_POLAR_FIELDS = [("n", C.c_uint64), ("n_nonfinite", C.c_uint64), ("n_dark", C.c_uint64), ("n_over", C.c_uint64), ("argmax", C.c_uint64),
                     ("max_dop", C.c_double), ("sum_i", C.c_double), ("sum_q", C.c_double), ("sum_u", C.c_double), ("sum_v", C.c_double),
                     ("sum_lin", C.c_double), ("sum_pol", C.c_double)]


class FilmPolar(C.Structure):        # wtgpu_film_polar
    _fields_ = FILM_POLAR_FIELDS


class FilmDenoiseSpec(C.Structure):  # wtgpu_film_denoise_spec
    _fields_ = [("window_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float),
                ("eps", C.c_float), ("pad2", C.c_float)]


class FilmDenoiseGuides(C.Structure):  # wtgpu_film_denoise_guides
    _fields_ = [("n_guides", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float * 8)]


FILM_DENOISE_SAME_ID = 1
FILM_DENOISE_MAX_GUIDES = 8
# bit i of wtgpu_first_hit_spec.maps / .ids, the floats (words) of each and their order in memory
FIRST_HIT_MAPS = [("coverage", 1), ("depth", 1), ("position", 3), ("normal_geo", 3), ("normal_shading", 3), ("uv", 2), ("facing", 1)]
FIRST_HIT_IDS = [("shape", 1), ("triangle", 1)]
FIRST_HIT_MAX_SAMPLES = 4096
# bit i of wtgpu_first_hit_material_spec.maps (n_k floats each, in this order in memory) / .ids
FIRST_HIT_MATERIAL_MAPS = ["albedo", "specular", "opacity", "roughness", "emission"]
FIRST_HIT_MATERIAL_IDS = ["material", "type"]
FIRST_HIT_MATERIAL_MAX_K = 4
# the same of wtgpu_los_spec.maps (per element and emitter), .elem and .ids (per element)
LOS_MAPS = [("visible", 1), ("distance", 1), ("direction", 3), ("cos", 1)]
LOS_ELEM = [("point", 3), ("nearest_distance", 1)]
LOS_IDS = [("n_visible", 1), ("nearest", 1)]
LOS_FRONT_ONLY = 1
LOS_MAX_SAMPLES, LOS_MAX_EMITTERS = 4096, 32
FILM_POLAR_MAPS = ["dolp", "dop", "docp", "aolp", "chi", "analyser"]      # bit i of wtgpu_film_polar_spec.maps, and the order of the maps in memory
FILM_STATS_SCALES = ["linear", "dB"]
FILM_STATS_ABS, FILM_STATS_LUMINANCE = 1, 2
FILM_STATS_MAX_BINS = 4096
TONEMAP_OPS = ["linear", "gamma", "sRGB", "dB", "function"]       # tonemap_e
TONEMAP_MODES = ["select", "normal", "colourmap"]                 # tonemap_mode_e
TONEMAP_FORMATS = {"f32": 0, "u8": 1, "u16": 2}


class SceneInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("n_tris", C.c_uint32), ("n_edges", C.c_uint32),
                ("n_nodes", C.c_uint32), ("n_leaves", C.c_uint32), ("n_shapes", C.c_uint32), ("n_emitters", C.c_uint32),
                ("n_materials", C.c_uint32), ("max_depth", C.c_int32), ("sensor_type", C.c_uint32), ("fsd_lut_power", C.c_double * 2),
                ("bytes_per_sample_state", C.c_uint64), ("stokes", C.c_uint32), ("integrator", C.c_uint32)]


COUNTER_FIELDS = ["samples", "segments", "ray_queries", "cone_queries", "vertices", "connections", "shadow_rays", "cone_tri_overflow",
                  "edge_overflow", "fsd_edge_overflow", "fsd_pool_overflow", "fsd_interactions", "null_interactions",
                  "surface_interactions", "light_splats", "walk_iteration_cap_hits", "traversal_stack_dropped"]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in COUNTER_FIELDS]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n in COUNTER_FIELDS}


# every symbol include/wtgpu.h declares
SYMBOLS = ["wtgpu_scene_create_named", "wtgpu_scene_create_from_desc", "wtgpu_scene_get_info", "wtgpu_scene_host_desc",
           "wtgpu_scene_upload", "wtgpu_render", "wtgpu_trace_rays", "wtgpu_traverse_cones", "wtgpu_get_counters",
           "wtgpu_reset_counters", "wtgpu_last_render_timings", "wtgpu_develop", "wtgpu_scene_destroy", "wtgpu_last_error",
           "wtgpu_scene_stats_json", "wtgpu_calibrate_copy", "wtgpu_render_async", "wtgpu_join", "wtgpu_query_regions", "wtgpu_render_progressive",
           "wtgpu_cancel", "wtgpu_pause", "wtgpu_resume", "wtgpu_capture_intermediate", "wtgpu_comm_unique_id", "wtgpu_comm_create", "wtgpu_film_reduce", "wtgpu_comm_destroy", "wtgpu_scene_create_from_xml",
           "wtgpu_scene_shape_id", "wtgpu_scene_sensor_mask_spec", "wtgpu_sensor_mask", "wtgpu_sensor_mask_host",
           "wtgpu_first_hit", "wtgpu_first_hit_host", "wtgpu_line_of_sight", "wtgpu_line_of_sight_host",
           "wtgpu_first_hit_material", "wtgpu_first_hit_material_host", "wtgpu_scene_channel_wavenumbers",
           "wtgpu_scene_tonemap_spec", "wtgpu_develop_device", "wtgpu_tonemap_device", "wtgpu_tonemap_host",
           "wtgpu_film_stats_edges", "wtgpu_film_stats_device", "wtgpu_film_stats_host",
           "wtgpu_film_compare_device", "wtgpu_film_compare_host", "wtgpu_film_polar_device", "wtgpu_film_polar_host",
           "wtgpu_tonemap_source_device", "wtgpu_tonemap_source_host", "wtgpu_film_stats_source_device", "wtgpu_film_stats_source_host",
           "wtgpu_film_compare_source_device", "wtgpu_film_compare_source_host", "wtgpu_film_polar_source_device", "wtgpu_film_polar_source_host",
           "wtgpu_film_zonal_device", "wtgpu_film_zonal_host", "wtgpu_film_segments_device", "wtgpu_film_segments_host",
           "wtgpu_film_distance_device", "wtgpu_film_distance_host",
           "wtgpu_film_denoise_device", "wtgpu_film_denoise_host",
           "wtgpu_film_denoise_guided_device", "wtgpu_film_denoise_guided_host"]
PROGRESS_CB = C.CFUNCTYPE(C.c_int, C.c_uint64, C.c_uint64, C.c_void_p)
CAPTURE_CB = C.CFUNCTYPE(None, C.c_uint64, C.c_void_p)

_lib = None


def connect_class_order():
    """Test hook (wtgpu_test_hooks.h): the length-class keys (tk * key_dim + sk) in the order k_connect_class takes the classes, as the host computes
    it, and key_dim."""
    import numpy as np
    lib = load_library()
    lib.wtgpu_test_connect_class_order.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    n, dim = C.c_uint32(0), C.c_uint32(0)
    _check(lib.wtgpu_test_connect_class_order(None, 0, C.byref(n), C.byref(dim)))
    keys = np.zeros(n.value, np.uint32)
    _check(lib.wtgpu_test_connect_class_order(keys.ctypes.data, keys.size, C.byref(n), C.byref(dim)))
    return keys, int(dim.value)


def dn_exp2_neg(t):
    """Test hook (wtgpu_test_hooks.h): wt/film_denoise.h's dn_exp2_neg, 2^-t for t >= 0, element by element on the host; t, result: numpy f32."""
    import numpy as np
    t = np.ascontiguousarray(t, dtype=np.float32)
    out = np.zeros(t.shape, dtype=np.float32)
    _check(load_library().wtgpu_test_dn_exp2_neg(t.ctypes.data, t.size, out.ctypes.data))
    return out


def fz_sum(x=(), words=None):
    """Test hook (wtgpu_test_hooks.h): the zonal statistics' exact sum by itself (wt/film_zonal.h) on the host — fz_add of the finite ones of the f32
    x onto `words` (nine uint64, two's complement; None: zeros), then fz_round -> (the f64, the words as they then are)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    w = np.zeros(9, np.uint64) if words is None else np.array(words, dtype=np.uint64).reshape(9).copy()
    out = C.c_double(0.0)
    _check(load_library().wtgpu_test_fz_sum(w.ctypes.data, x.ctypes.data if x.size else None, x.size, C.byref(out)))
    return out.value, w


def film_zonal_form(scene):
    """Test hook (wtgpu_test_hooks.h): the form of k_film_zonal the scene's last film_zonal_device call launched — "lds", "global", or None before
    the first call.  Both forms give the same bits, so only this tells which one ran."""
    lds = C.c_uint32(0)
    _check(load_library().wtgpu_test_film_zonal_form(scene.handle, C.byref(lds)))
    return {0: "global", 1: "lds"}.get(lds.value)


def film_segments_form(scene):
    """Test hook (wtgpu_test_hooks.h): (form, overflow) of the scene's last film_segments_device call — form "tiled" or "global" (the form of its first two
    phases, WTGPU_FILM_SEGMENTS_TILED; both give the same bits, so only this tells which one ran),
    overflow the union-find's overflow word (0: no loop hit its step bound); (None, None) before the first call."""
    form, over = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().wtgpu_test_film_segments_form(scene.handle, C.byref(form), C.byref(over)))
    return (None, None) if form.value == 0xFFFFFFFF else ({0: "global", 1: "tiled"}[form.value], int(over.value))


def film_distance_form(scene):
    """Test hook (wtgpu_test_hooks.h): the form of k_dist_rows that the scene's last film_distance_device call launched — "groups" (the outward search
    ends at |dx| = 64 and goes on group by group, WTGPU_FILM_DISTANCE_GROUPS=1) or "plain" (the outward search alone); both give the same bits, so
    only this tells which one ran; None before the first call."""
    groups = C.c_uint32(0)
    _check(load_library().wtgpu_test_film_distance_form(scene.handle, C.byref(groups)))
    return {0: "plain", 1: "groups"}.get(groups.value)


def film_segments_find(parent, x, bound):
    """Test hook (wtgpu_test_hooks.h): the segments' union-find walk by itself on the host (csrc/kernels_segments.hip: seg_find) — up the uint32
    `parent` array from x with at most `bound` loads -> (where it ended, whether the bound was hit or a parent lies above its child)."""
    import numpy as np
    parent = np.ascontiguousarray(parent, dtype=np.uint32).reshape(-1)
    root, over = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().wtgpu_test_film_segments_find(parent.ctypes.data, parent.size, int(x), int(bound), C.byref(root), C.byref(over)))
    return int(root.value), bool(over.value)


def load_library():
    """Loads libwtgpu.so; raises loudly if the HIP extension has not been built (there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise WtgpuError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"(hipcc --offload-arch=gfx950); wave_tracer_amd has no CPU fallback")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes in one process leave the second one without
    # devices.  Importing torch first makes the dynamic loader bind libwtgpu.so to the runtime torch already loaded, so
    # that torch tensors / streams and our kernels share one HIP context.
    # The kernel-argument ring must be set before the HIP runtime initialises (its first API call).
    os.environ.setdefault("HSA_KERNARG_POOL_SIZE", str(16 << 20))
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    lib.wtgpu_scene_create_named.argtypes = [C.c_char_p, C.POINTER(SceneParams), C.POINTER(vp)]
    lib.wtgpu_scene_create_named_hooks.argtypes = [C.c_char_p, C.POINTER(SceneParams), C.POINTER(TestHooks), C.POINTER(vp)]
    lib.wtgpu_scene_create_from_desc.argtypes = [vp, C.POINTER(vp)]
    lib.wtgpu_scene_create_from_xml.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), u32, C.POINTER(SceneParams), C.POINTER(vp)]
    lib.wtgpu_scene_compare.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    lib.wtgpu_scene_compare_part.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.c_size_t]
    lib.wtgpu_trace_ab_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.wtgpu_render_progressive.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64, u32, PROGRESS_CB, vp, C.POINTER(u64)]
    lib.wtgpu_cancel.argtypes = [vp]
    lib.wtgpu_pause.argtypes = [vp]
    lib.wtgpu_resume.argtypes = [vp]
    lib.wtgpu_capture_intermediate.argtypes = [vp, CAPTURE_CB, vp]
    lib.wtgpu_comm_unique_id.argtypes = [vp]
    lib.wtgpu_comm_create.argtypes = [i32, i32, i32, vp, C.POINTER(vp)]
    lib.wtgpu_film_reduce.argtypes = [vp, vp, vp, vp, vp, u64, u64, i32]
    lib.wtgpu_comm_destroy.argtypes = [vp]
    lib.wtgpu_comm_destroy.restype = None
    lib.wtgpu_scene_get_info.argtypes = [vp, C.POINTER(SceneInfo)]
    lib.wtgpu_scene_host_desc.argtypes = [vp]
    lib.wtgpu_scene_host_desc.restype = vp
    lib.wtgpu_scene_upload.argtypes = [vp, i32, u64]
    lib.wtgpu_render.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64]
    lib.wtgpu_render_async.argtypes = [vp, vp, vp, vp, vp, u64, u64, u64]
    lib.wtgpu_join.argtypes = [vp, vp]
    lib.wtgpu_trace_rays.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
    lib.wtgpu_traverse_cones.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp]
    lib.wtgpu_query_regions.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]
    lib.wtgpu_test_fsd_apertures.argtypes = [vp, vp, vp, vp, vp, vp, u32, u32, u32, u32, vp, vp]
    lib.wtgpu_test_utd_sums.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]
    lib.wtgpu_test_profile_counters.argtypes = [vp, vp, u32]
    lib.wtgpu_test_bsdf_queries.argtypes = [vp, vp, vp, u32, i32, vp]
    lib.wtgpu_test_source_queries.argtypes = [vp, vp, vp, u32, vp]
    lib.wtgpu_test_flux_queries.argtypes = [vp, vp, vp, u32, vp]
    lib.wtgpu_scene_shape_id.argtypes = [vp, u32, C.POINTER(C.c_char_p)]
    lib.wtgpu_scene_sensor_mask_spec.argtypes = [vp, C.POINTER(SensorMaskSpec)]
    lib.wtgpu_sensor_mask.argtypes = [vp, vp, vp, u32, u64, vp]
    lib.wtgpu_sensor_mask_host.argtypes = [vp, vp, u32, u64, u32, vp]
    lib.wtgpu_first_hit.argtypes = [vp, vp, C.POINTER(FirstHitSpec), vp, vp]
    lib.wtgpu_first_hit_host.argtypes = [vp, C.POINTER(FirstHitSpec), u32, vp, vp]
    lib.wtgpu_first_hit_material.argtypes = [vp, vp, C.POINTER(FirstHitMaterialSpec), vp, vp]
    lib.wtgpu_first_hit_material_host.argtypes = [vp, C.POINTER(FirstHitMaterialSpec), u32, vp, vp]
    lib.wtgpu_scene_channel_wavenumbers.argtypes = [vp, vp]
    lib.wtgpu_line_of_sight.argtypes = [vp, vp, C.POINTER(LosSpec), vp, vp, vp, vp, vp, vp]
    lib.wtgpu_line_of_sight_host.argtypes = [vp, C.POINTER(LosSpec), vp, vp, vp, u32, vp, vp, vp]
    lib.wtgpu_scene_tonemap_spec.argtypes = [vp, C.POINTER(TonemapSpec)]
    lib.wtgpu_develop_device.argtypes = [vp, vp, vp, vp, vp, u64, vp]
    lib.wtgpu_tonemap_device.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(Tonemap), u32, vp, u32, vp]
    lib.wtgpu_tonemap_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(Tonemap), u32, vp, u32, u32, vp]
    lib.wtgpu_film_stats_edges.argtypes = [C.POINTER(FilmStatsSpec), vp]
    lib.wtgpu_film_stats_device.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(FilmStatsSpec), vp, vp, vp]
    lib.wtgpu_film_stats_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(FilmStatsSpec), vp, u32, vp, vp]
    lib.wtgpu_film_compare_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmCompareSpec), vp, vp, vp]
    lib.wtgpu_film_compare_host.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmCompareSpec), vp, u32, vp, vp]
    lib.wtgpu_film_polar_device.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(FilmPolarSpec), vp, vp, vp, vp]
    lib.wtgpu_film_polar_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(FilmPolarSpec), vp, u32, vp, vp, vp]
    src = C.POINTER(FilmSource)
    lib.wtgpu_tonemap_source_device.argtypes = [vp, vp, src, C.POINTER(Tonemap), u32, vp, u32, vp]
    lib.wtgpu_tonemap_source_host.argtypes = [vp, src, C.POINTER(Tonemap), u32, vp, u32, u32, vp]
    lib.wtgpu_film_stats_source_device.argtypes = [vp, vp, src, C.POINTER(FilmStatsSpec), vp, vp, vp]
    lib.wtgpu_film_stats_source_host.argtypes = [vp, src, C.POINTER(FilmStatsSpec), vp, u32, vp, vp]
    lib.wtgpu_film_zonal_device.argtypes = [vp, vp, src, C.POINTER(FilmZonalSpec), vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.wtgpu_film_zonal_host.argtypes = [vp, src, C.POINTER(FilmZonalSpec), vp, vp, u32, vp, vp, C.POINTER(u64), vp]
    lib.wtgpu_film_segments_device.argtypes = [vp, vp, C.POINTER(FilmSegmentsSpec), vp, vp, vp, C.POINTER(FilmSegmentsInfo), vp]
    lib.wtgpu_film_segments_host.argtypes = [vp, C.POINTER(FilmSegmentsSpec), vp, vp, u32, vp, C.POINTER(FilmSegmentsInfo), vp]
    lib.wtgpu_film_distance_device.argtypes = [vp, vp, C.POINTER(FilmDistanceSpec), vp, vp, vp, vp, C.POINTER(FilmDistanceInfo)]
    lib.wtgpu_film_distance_host.argtypes = [vp, C.POINTER(FilmDistanceSpec), vp, vp, u32, vp, vp, C.POINTER(FilmDistanceInfo)]
    lib.wtgpu_test_film_distance_form.argtypes = [vp, C.POINTER(u32)]
    lib.wtgpu_test_film_segments_form.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    lib.wtgpu_test_film_segments_find.argtypes = [vp, u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
    lib.wtgpu_test_fz_sum.argtypes = [vp, vp, u64, C.POINTER(C.c_double)]
    lib.wtgpu_test_film_zonal_form.argtypes = [vp, C.POINTER(u32)]
    lib.wtgpu_film_compare_source_device.argtypes = [vp, vp, src, src, C.POINTER(FilmCompareSpec), vp, vp, vp]
    lib.wtgpu_film_compare_source_host.argtypes = [vp, src, src, C.POINTER(FilmCompareSpec), vp, u32, vp, vp]
    lib.wtgpu_film_polar_source_device.argtypes = [vp, vp, src, C.POINTER(FilmPolarSpec), vp, vp, vp, vp]
    lib.wtgpu_film_polar_source_host.argtypes = [vp, src, C.POINTER(FilmPolarSpec), vp, u32, vp, vp, vp]
    lib.wtgpu_film_denoise_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmDenoiseSpec), vp, vp, vp]
    lib.wtgpu_film_denoise_host.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmDenoiseSpec), vp, u32, vp, vp]
    lib.wtgpu_film_denoise_guided_device.argtypes = [vp, vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmDenoiseSpec), C.POINTER(FilmDenoiseGuides), vp, vp, vp, vp, vp]
    lib.wtgpu_film_denoise_guided_host.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(FilmDenoiseSpec), C.POINTER(FilmDenoiseGuides), vp, vp, vp, u32, vp, vp]
    lib.wtgpu_test_dn_exp2_neg.argtypes = [vp, u64, vp]
    lib.wtgpu_calibrate_copy.argtypes = [u64, i32]
    lib.wtgpu_get_counters.argtypes = [vp, C.POINTER(Counters)]
    lib.wtgpu_reset_counters.argtypes = [vp]
    lib.wtgpu_last_render_timings.argtypes = [vp, C.POINTER(C.c_float * 12)]
    lib.wtgpu_develop.argtypes = [vp, vp, vp, vp, u64, vp]
    lib.wtgpu_scene_destroy.argtypes = [vp]
    lib.wtgpu_scene_destroy.restype = None
    lib.wtgpu_last_error.restype = C.c_char_p
    lib.wtgpu_scene_stats_json.argtypes = [vp]
    lib.wtgpu_scene_stats_json.restype = C.c_char_p
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise WtgpuError(f"wtgpu error {rc}: {load_library().wtgpu_last_error().decode(errors='replace')}")


def _bit_groups(names, table, what, who, n_k=None):
    """One group of a map spec -> (bits, layout, total): `names` in any order, bit i and the memory order from table[i] = (name, n) or name.
    layout: [(name, offset, width)], width 0 = one value without an axis of its own.  n_k: every entry is n_k values (the material maps)."""
    names = [names] if isinstance(names, str) else list(names)
    table = [(e, 1) if isinstance(e, str) else e for e in table]
    known = [n for n, _ in table]
    for n in names:
        if n not in known:
            raise ValueError(f"{who}: unknown {what} {n!r} (one of {known})")
    bits, layout, off = 0, [], 0
    for i, (n, k) in enumerate(table):
        if n in names:
            k = k if n_k is None else k * n_k
            bits |= 1 << i
            layout.append((n, off, 0 if k == 1 and n_k is None else k))
            off += k
    return bits, layout, off


def _views(layouts, arrays):
    """{name: view} of one array [..., K] per group (None where K = 0) by the group's layout (_bit_groups)."""
    return {n: a[..., off:off + k] if k else a[..., off] for layout, a in zip(layouts, arrays) for n, off, k in layout}


def _map_outputs(shapes, dev=None):
    """One array per group of shape `shape` (None where its last extent is 0), the last group the ids: torch tensors on `dev` (ids int32), or
    zeroed numpy arrays (ids uint32).  -> the arrays and their addresses."""
    ids = len(shapes) - 1
    if dev is not None:
        import torch
        arrays = [torch.empty(s, dtype=torch.int32 if g == ids else torch.float32, device=dev) if s[-1] else None for g, s in enumerate(shapes)]
        return arrays, [None if a is None else a.data_ptr() for a in arrays]
    import numpy as np
    arrays = [np.zeros(s, np.uint32 if g == ids else np.float32) if s[-1] else None for g, s in enumerate(shapes)]
    return arrays, [None if a is None else a.ctypes.data for a in arrays]


class Scene:
    """Handle of a flattened scene (host-baked; optionally uploaded to one GPU)."""

    def __init__(self, name, res=256, max_depth=-1, fsd=-1, mis=-1, rr=-1, force_ray_tracing=0, mesh_detail=1, lut=(0, 0), only_s=None, only_t=None, crop_of=0,
                 polarimetric=0):
        lib = load_library()
        p = SceneParams(res, max_depth, fsd, mis, rr, force_ray_tracing, mesh_detail, lut[0], lut[1], polarimetric)
        h = C.c_void_p()
        if only_s is None and only_t is None and not crop_of:
            _check(lib.wtgpu_scene_create_named(name.encode(), C.byref(p), C.byref(h)))
        else:       # test hooks (single-strategy renders, crops of a larger film)
            hooks = TestHooks(0 if only_s is None else only_s + 1, 0 if only_t is None else only_t + 1, crop_of)
            _check(lib.wtgpu_scene_create_named_hooks(name.encode(), C.byref(p), C.byref(hooks), C.byref(h)))
        self._h = h
        self.name = name
        info = SceneInfo()
        _check(lib.wtgpu_scene_get_info(h, C.byref(info)))
        self.info = info
        # `channels` = film planes per pixel: spectral channels x Stokes components (1, or 4 for polarimetric sensors)
        self.spectral_channels, self.stokes = info.channels, info.stokes
        self.width, self.height, self.channels = info.width, info.height, info.channels * info.stokes
        self.device = None

    @classmethod
    def from_desc(cls, desc_ptr, keepalive=None, name="<desc>"):
        """Wraps an already flattened scene (pointer to a host `wt::scene_t`, wtgpu_scene_create_from_desc): the entry point a port of
        the reference's own loader would use.  `keepalive`: the object owning the host arrays (they must outlive the handle)."""
        lib = load_library()
        self = cls.__new__(cls)
        h = C.c_void_p()
        _check(lib.wtgpu_scene_create_from_desc(C.c_void_p(desc_ptr), C.byref(h)))
        self._h = h
        self._keepalive = keepalive
        self.name = name
        info = SceneInfo()
        _check(lib.wtgpu_scene_get_info(h, C.byref(info)))
        self.info = info
        self.spectral_channels, self.stokes = info.channels, info.stokes
        self.width, self.height, self.channels = info.width, info.height, info.channels * info.stokes
        self.device = None
        return self

    @classmethod
    def from_xml(cls, path, defines=None, res=0, max_depth=-1, fsd=-1, mis=-1, rr=-1, force_ray_tracing=0, lut=(0, 0), polarimetric=0, mesh_detail=1):
        """Loads a scene file of the reference's XML format with the minimal reader (wtgpu_scene_create_from_xml).  `defines`: dict of
        the reference's -D command-line defines.  mesh_detail: tessellation of the procedural stand-ins that replace Git-LFS pointer
        files (0: low-poly, for the CPU checker)."""
        lib = load_library()
        self = cls.__new__(cls)
        p = SceneParams(res, max_depth, fsd, mis, rr, force_ray_tracing, mesh_detail, lut[0], lut[1], polarimetric)
        d = [f"{k}={v}".encode() for k, v in (defines or {}).items()]
        arr = (C.c_char_p * max(1, len(d)))(*d)
        h = C.c_void_p()
        _check(lib.wtgpu_scene_create_from_xml(str(path).encode(), arr, len(d), C.byref(p), C.byref(h)))
        self._h = h
        self.name = os.path.basename(str(path))
        info = SceneInfo()
        _check(lib.wtgpu_scene_get_info(h, C.byref(info)))
        self.info = info
        self.spectral_channels, self.stokes = info.channels, info.stokes
        self.width, self.height, self.channels = info.width, info.height, info.channels * info.stokes
        self.device = None
        return self

    def first_difference(self, other, part=None):
        """Test hook (wtgpu_scene_compare[_part]): '' when the two flattened scenes are identical byte for byte, else the first differing
        array.  part: "sensor" | "opts" | "emitters" compares only that record."""
        buf = C.create_string_buffer(256)
        if part:
            rc = load_library().wtgpu_scene_compare_part(self._h, other._h, part.encode(), buf, 256)
        else:
            rc = load_library().wtgpu_scene_compare(self._h, other._h, buf, 256)
        if rc not in (0, 1):
            _check(rc)
        return buf.value.decode()

    @property
    def handle(self):
        return self._h

    def host_desc(self):
        return load_library().wtgpu_scene_host_desc(self._h)

    def stats(self):
        return json.loads(load_library().wtgpu_scene_stats_json(self._h).decode())

    def emitter_summary(self):
        """The scene's emitters in selection order: [{type, cutoff_deg, shape, select_pmf}]."""
        return self.stats()["emitter_list"]

    def upload(self, device=0, max_batch_samples=0):
        _check(load_library().wtgpu_scene_upload(self._h, int(device), int(max_batch_samples)))
        self.device = int(device)
        return self

    def render_into(self, value, weight, light, sample_begin, sample_end, seed, stream=None):
        """value/weight/light: CUDA(HIP) float64 torch tensors [H,W,C], [H,W], [H,W,C] (accumulated into)."""
        sp = C.c_void_p(stream) if stream else None
        _check(load_library().wtgpu_render(self._h, sp, value.data_ptr(), weight.data_ptr(), light.data_ptr(), int(sample_begin),
                                           int(sample_end), int(seed)))

    def render_async_into(self, value, weight, light, sample_begin, sample_end, seed, stream=None):
        """Like render_into, but `stream` does not wait for the work: consecutive calls pipeline on the GPU.  Call join(stream)
        before anything reads or overwrites the films."""
        sp = C.c_void_p(stream) if stream else None
        _check(load_library().wtgpu_render_async(self._h, sp, value.data_ptr(), weight.data_ptr(), light.data_ptr(), int(sample_begin),
                                                 int(sample_end), int(seed)))

    def render_progressive(self, value, weight, light, sample_begin, sample_end, seed, chunk_spp=1, progress=None, stream=None):
        """Blocking render with the reference's control surface: progress(samples_done, samples_total) -> truthy to stop; cancel() from
        any thread.  Returns (cancelled, samples_per_element_done)."""
        sp = C.c_void_p(stream) if stream else None
        cb = PROGRESS_CB((lambda d, t, u: 1 if progress(d, t) else 0) if progress else (lambda d, t, u: 0))
        done = C.c_uint64(0)
        lib = load_library()
        rc = lib.wtgpu_render_progressive(self._h, sp, value.data_ptr(), weight.data_ptr(), light.data_ptr(), int(sample_begin), int(sample_end),
                                          int(seed), int(chunk_spp), cb, None, C.byref(done))
        if rc == 6:      # WTGPU_CANCELLED
            return True, int(done.value)
        _check(rc)
        return False, int(done.value)

    def cancel(self):
        _check(load_library().wtgpu_cancel(self._h))

    def pause(self):
        """The running render_progressive stops launching at its next chunk boundary until resume() (scene_renderer_t's pause interrupt)."""
        _check(load_library().wtgpu_pause(self._h))

    def resume(self):
        _check(load_library().wtgpu_resume(self._h))

    def capture_intermediate(self, fn):
        """`capture intermediate`: fn(samples_per_element_done) is called once by the render thread at its next chunk boundary, with the films
        consistent (exactly the completed chunks).  Thread-safe."""
        # every trampoline stays alive until it has been CALLED: a request that replaces a pending one may arrive after the render thread has
        # already copied the old pointer
        keep = self.__dict__.setdefault("_capture_keepalive", [])
        slot = []

        def tramp(done, user):
            try:
                fn(int(done))
            finally:
                if slot and slot[0] in keep:
                    keep.remove(slot[0])
        cb = CAPTURE_CB(tramp)
        slot.append(cb)
        keep.append(cb)
        if len(keep) > 64:   # (requests that were replaced before they ran are never called: bound the list, oldest first)
            del keep[0]
        _check(load_library().wtgpu_capture_intermediate(self._h, cb, None))

    def join(self, stream=None):
        _check(load_library().wtgpu_join(self._h, C.c_void_p(stream) if stream else None))

    def trace_rays(self, rays):
        """rays: [n,8] f32 {o, d, tmin, tmax} (numpy) -> (dist, tuid, bary, front) numpy; device arrays are torch tensors."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        n = len(rays)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays, dtype=np.float32)).to(dev)
        dist = torch.zeros(n, dtype=torch.float32, device=dev)
        tuid = torch.zeros(n, dtype=torch.int32, device=dev)
        bary = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        front = torch.zeros(n, dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_trace_rays(self._h, None, d_rays.data_ptr(), n, dist.data_ptr(), tuid.data_ptr(), bary.data_ptr(), front.data_ptr()))
        torch.cuda.synchronize(dev)
        return dist.cpu().numpy(), tuid.cpu().numpy().view(np.uint32), bary.cpu().numpy(), front.cpu().numpy().view(np.uint32)

    def traverse_cones(self, cones, cap=64):
        """cones: [n,10] f32 {o, d, tan_alpha, x0, ecc, lambda_m} -> (dist, flags, ntris, tris[n,cap] sorted)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        n = len(cones)
        d_cones = torch.from_numpy(np.ascontiguousarray(cones, dtype=np.float32)).to(dev)
        dist = torch.zeros(n, dtype=torch.float32, device=dev)
        flags = torch.zeros(n, dtype=torch.int32, device=dev)
        ntris = torch.zeros(n, dtype=torch.int32, device=dev)
        tris = torch.zeros((n, cap), dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_traverse_cones(self._h, None, d_cones.data_ptr(), n, cap, dist.data_ptr(), flags.data_ptr(), ntris.data_ptr(),
                                                   tris.data_ptr()))
        torch.cuda.synchronize(dev)
        return (dist.cpu().numpy(), flags.cpu().numpy().view(np.uint32), ntris.cpu().numpy().view(np.uint32),
                tris.cpu().numpy().view(np.uint32))

    def query_regions(self, cones, edge_cap=96):
        """cones: [n,10] f32 -> dict of numpy arrays: dist, flags, primary, ntris, nedges, edges[n,edge_cap] (sorted, 0xFFFFFFFF padded), flux."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        n = len(cones)
        d_cones = torch.from_numpy(np.ascontiguousarray(cones, dtype=np.float32)).to(dev)
        dist = torch.zeros(n, dtype=torch.float32, device=dev)
        flux = torch.zeros(n, dtype=torch.float32, device=dev)
        flags, primary, ntris, nedges = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
        edges = torch.full((n, edge_cap), -1, dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_query_regions(self._h, None, d_cones.data_ptr(), n, edge_cap, dist.data_ptr(), flags.data_ptr(), primary.data_ptr(),
                                                  ntris.data_ptr(), nedges.data_ptr(), edges.data_ptr(), flux.data_ptr()))
        torch.cuda.synchronize(dev)
        u = lambda t: t.cpu().numpy().view(np.uint32)
        return {"dist": dist.cpu().numpy(), "flags": u(flags), "primary": u(primary), "ntris": u(ntris), "nedges": u(nedges), "edges": u(edges),
                "flux": flux.cpu().numpy()}

    def fsd_apertures(self, cones, sk, ids, n_ids, pool_cap=4096, mode=0):
        """Test hook (wtgpu_test_hooks.h): one Fraunhofer aperture per query.  cones [n,10], sk [n,3] = (sigma.x, sigma.y, k), ids [n,id_cap] edge ids,
        n_ids [n]; mode 0 = coop_build_aperture, 1 = the sequential build.  -> (hdr [n,8] u32, segs [n,pool_cap,7] f32); layouts: wt/diffraction_probe.h."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n, id_cap = ids.shape
        n_ids = np.ascontiguousarray(n_ids, dtype=np.uint32)
        assert len(cones) == n and len(sk) == n and len(n_ids) == n and (n_ids <= id_cap).all()
        n_edges = self.info.n_edges
        assert all((ids[i, :n_ids[i]] < n_edges).all() for i in range(n)), "edge id out of range"
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        d_cones, d_sk = t(cones, np.float32), t(sk, np.float32)
        d_ids, d_nids = t(ids.view(np.int32), np.int32), t(n_ids.view(np.int32), np.int32)
        hdr = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        segs = torch.zeros((n, pool_cap, 7), dtype=torch.float32, device=dev)
        _check(load_library().wtgpu_test_fsd_apertures(self._h, None, d_cones.data_ptr(), d_sk.data_ptr(), d_ids.data_ptr(), d_nids.data_ptr(), n, id_cap,
                                                       pool_cap, mode, hdr.data_ptr(), segs.data_ptr()))
        torch.cuda.synchronize(dev)
        return hdr.cpu().numpy().view(np.uint32), segs.cpu().numpy()

    def utd_sums(self, queries, ids, n_ids, utd_cap=48):
        """Test hook (wtgpu_test_hooks.h): one UTD aperture per query [n,32] (wt/diffraction_probe.h) from ids [n,id_cap] / n_ids [n], its per-wedge
        terms and the coherent sums of coop_do_fsd<1,8,64> and path_do_fsd.  -> (hdr [n,8] u32, edges [n,utd_cap,8] u32, recs [n,utd_cap,3] u32)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        n, id_cap = ids.shape
        n_ids = np.ascontiguousarray(n_ids, dtype=np.uint32)
        assert len(queries) == n and len(n_ids) == n and (n_ids <= id_cap).all()
        n_edges = self.info.n_edges
        assert all((ids[i, :n_ids[i]] < n_edges).all() for i in range(n)), "edge id out of range"
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        d_q, d_ids, d_nids = t(queries, np.float32), t(ids.view(np.int32), np.int32), t(n_ids.view(np.int32), np.int32)
        hdr = torch.zeros((n, 8), dtype=torch.int32, device=dev)
        edges = torch.zeros((n, utd_cap, 8), dtype=torch.int32, device=dev)
        recs = torch.zeros((n, utd_cap, 3), dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_test_utd_sums(self._h, None, d_q.data_ptr(), d_ids.data_ptr(), d_nids.data_ptr(), n, id_cap, utd_cap, recs.data_ptr(),
                                                  hdr.data_ptr(), edges.data_ptr()))
        torch.cuda.synchronize(dev)
        u = lambda x: x.cpu().numpy().view(np.uint32)
        return u(hdr), u(edges), u(recs)

    def bsdf_queries(self, queries, form=-1):
        """Test hook (wtgpu_test_hooks.h): the material layer per query.  queries [n,18] u32 (wt/bsdf_probe.h); form -1 = generic, 0 / 1 / 2 = the
        class form of diffuse / dielectric / surface_spm.  -> out [n,48] u32 (f32 bits except flags and the draw count)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        n = q.shape[0]
        assert q.shape == (n, 18) and (q[:, 0] < self.info.n_materials).all(), "material id out of range"
        d_q = torch.from_numpy(q.view(np.int32)).to(dev)
        out = torch.zeros((n, 48), dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_test_bsdf_queries(self._h, None, d_q.data_ptr(), n, int(form), out.data_ptr()))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)

    def source_queries(self, queries):
        """Test hook (wtgpu_test_hooks.h): the emitter / sensor / wavenumber layer per query.  queries [n,24] u32 (wt/sources_probe.h) -> out
        [n,80] u32 (f32 bits except the discrete words).  An op, emitter index or tuid out of range raises (WTGPU_ERR_INVALID)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        n = q.shape[0]
        assert q.shape == (n, 24)
        d_q = torch.from_numpy(q.view(np.int32)).to(dev)
        out = torch.zeros((n, 80), dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_test_source_queries(self._h, None, d_q.data_ptr(), n, out.data_ptr()))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)

    def flux_queries(self, queries):
        """Test hook (wtgpu_test_hooks.h): the region power integral per query.  queries [n,20] u32 (wt/flux_probe.h) -> out [n,36] u32 (f32 bits
        except the discrete words).  An op or tuid out of range raises (WTGPU_ERR_INVALID)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        q = np.ascontiguousarray(queries, dtype=np.uint32)
        n = q.shape[0]
        assert q.shape == (n, 20)
        d_q = torch.from_numpy(q.view(np.int32)).to(dev)
        out = torch.zeros((n, 36), dtype=torch.int32, device=dev)
        _check(load_library().wtgpu_test_flux_queries(self._h, None, d_q.data_ptr(), n, out.data_ptr()))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy().view(np.uint32)

    @property
    def shape_ids(self):
        """The element id of every shape, in shape order (scene files: the element's `id`, "__unnamed_$<n>" for unnamed enabled top-level
        elements, src/scene/loader/loader.cpp:131-133; bundled scenes and descriptions: empty strings)."""
        lib, out = load_library(), []
        for i in range(self.info.n_shapes):
            p = C.c_char_p()
            _check(lib.wtgpu_scene_shape_id(self._h, i, C.byref(p)))
            out.append(p.value.decode())
        return out

    @property
    def sensor_mask_spec(self):
        """The scene file's <sensor_mask type="by-geometry"> (src/sensor/mask.cpp:76-108): None, or {"regex", "samples" (always 32: the
        reference's loader drops the attribute), "shapes": uint8 numpy array, 1 where the shape's id matches the regex}."""
        import numpy as np
        s = SensorMaskSpec()
        _check(load_library().wtgpu_scene_sensor_mask_spec(self._h, C.byref(s)))
        if not s.present:
            return None
        flags = np.ctypeslib.as_array(s.shape_flags, (s.n_shapes,)).copy() if s.n_shapes else np.zeros(0, np.uint8)
        return {"regex": s.regex.decode(), "samples": int(s.samples), "shapes": flags}

    def _mask_args(self, samples, shapes):
        import numpy as np
        if samples is None:
            spec = self.sensor_mask_spec
            samples = spec["samples"] if spec else 32
        if shapes is None:
            return int(samples), None
        flags = np.ascontiguousarray(np.asarray(shapes) != 0, dtype=np.uint8)
        if flags.shape != (self.info.n_shapes,):
            raise ValueError(f"shapes: one flag per shape expected ({self.info.n_shapes}), got shape {flags.shape}")
        return int(samples), flags

    def sensor_mask(self, samples=None, seed=1, shapes=None, stream=None):
        """mask_t::create_mask on the scene's device (wtgpu_sensor_mask): an H x W float32 torch tensor, per pixel the share of `samples`
        primary rays whose first hit is on a shape that does NOT match the mask.  samples: None = the scene file's (32).  shapes: None = the
        scene file's flags, else one flag per shape (true = matches the regex: not counted).  Enqueued on `stream` (default: torch's current)."""
        import torch
        dev = self._uploaded_device("sensor_mask")
        n, flags = self._mask_args(samples, shapes)
        out = torch.empty((self.height, self.width), dtype=torch.float32, device=dev)
        _check(load_library().wtgpu_sensor_mask(self._h, self._stream_arg(stream, dev), None if flags is None else flags.ctypes.data, n, int(seed),
                                                out.data_ptr()))
        return out

    def sensor_mask_host(self, samples=None, seed=1, shapes=None, threads=0):
        """The same mask on host threads (wtgpu_sensor_mask_host; threads 0 = all cores), as numpy: bit for bit the device's."""
        import numpy as np
        n, flags = self._mask_args(samples, shapes)
        out = np.zeros((self.height, self.width), np.float32)
        _check(load_library().wtgpu_sensor_mask_host(self._h, None if flags is None else flags.ctypes.data, n, int(seed), int(threads), out.ctypes.data))
        return out

    def _uploaded_device(self, who):
        import torch
        if self.device is None:
            raise WtgpuError(f"{who}: upload(device) first")
        return torch.device("cuda", self.device)

    @staticmethod
    def _first_hit_args(samples, seed, maps, ids):
        """-> (wtgpu_first_hit_spec, the layouts of the maps and of the ids, (K, Ki)); names in any order, memory in bit order."""
        mbits, mlay, K = _bit_groups(maps, FIRST_HIT_MAPS, "map", "first_hit")
        ibits, ilay, Ki = _bit_groups(ids, FIRST_HIT_IDS, "id", "first_hit")
        return FirstHitSpec(int(samples), mbits, ibits, 0, int(seed)), (mlay, ilay), (K, Ki)

    def first_hit(self, samples=0, seed=1, maps=("coverage", "depth", "position", "normal_geo", "normal_shading", "uv", "facing"), ids=("shape", "triangle"),
                  stream=None):
        """First-hit maps of the perspective sensor on the scene's device (wtgpu_first_hit): {name: torch tensor [H, W] or [H, W, n]}, f32 maps
        (coverage, depth, position 3, normal_geo 3, normal_shading 3, uv 2, facing) and int32 ids holding the u32 bits (shape: the index
        shape_ids is listed by; triangle: within the shape; -1 = 0xFFFFFFFF without a hit) — views of one allocation per group.  samples 0:
        the ray through every pixel's centre; n >= 1: the n rays of sensor_mask(samples=n, seed), the maps their means over the rays that hit,
        the ids the first hitting ray's.  Enqueued on `stream` (default: torch's current)."""
        dev = self._uploaded_device("first_hit")
        spec, layouts, Ks = self._first_hit_args(samples, seed, maps, ids)
        arrays, (m, i) = _map_outputs([(self.height, self.width, K) for K in Ks], dev)
        _check(load_library().wtgpu_first_hit(self._h, self._stream_arg(stream, dev), C.byref(spec), m, i))
        return _views(layouts, arrays)

    def first_hit_host(self, samples=0, seed=1, maps=("coverage", "depth", "position", "normal_geo", "normal_shading", "uv", "facing"),
                       ids=("shape", "triangle"), threads=0):
        """The same maps on host threads (wtgpu_first_hit_host; threads 0 = all cores), as numpy (ids: uint32): bit for bit the device's."""
        spec, layouts, Ks = self._first_hit_args(samples, seed, maps, ids)
        arrays, (m, i) = _map_outputs([(self.height, self.width, K) for K in Ks])
        _check(load_library().wtgpu_first_hit_host(self._h, C.byref(spec), int(threads), m, i))
        return _views(layouts, arrays)

    def channel_wavenumbers(self):
        """One wavenumber [1/mm] per spectral channel (wtgpu_scene_channel_wavenumbers), numpy f32 [spectral_channels]: the line of a discrete
        response, the response-weighted mean over the knots of a tabulated one.  A constant or all-zero response is refused."""
        import numpy as np
        k = np.zeros(4, np.float32)
        _check(load_library().wtgpu_scene_channel_wavenumbers(self._h, k.ctypes.data))
        return k[:self.spectral_channels].copy()

    def _first_hit_material_args(self, samples, seed, k, maps, ids):
        """-> (wtgpu_first_hit_material_spec, the layouts of the maps and of the ids, (K, Ki)); names in any order, memory in bit order."""
        import numpy as np
        k = self.channel_wavenumbers() if k is None else np.atleast_1d(np.asarray(k, dtype=np.float32))
        if k.ndim != 1:
            raise ValueError("first_hit_material: k: a sequence of wavenumbers [1/mm] expected")
        mbits, mlay, K = _bit_groups(maps, FIRST_HIT_MATERIAL_MAPS, "map", "first_hit_material", n_k=int(k.size))
        ibits, ilay, Ki = _bit_groups(ids, FIRST_HIT_MATERIAL_IDS, "id", "first_hit_material")
        kk = (C.c_float * 4)(*[float(x) for x in k[:4]])
        return FirstHitMaterialSpec(int(samples), mbits, ibits, int(k.size), kk, int(seed)), (mlay, ilay), (K, Ki)

    def first_hit_material(self, samples=0, seed=1, k=None, maps=("albedo", "specular", "opacity", "roughness", "emission"), ids=("material", "type"),
                           stream=None):
        """First-hit material maps of the perspective sensor on the scene's device (wtgpu_first_hit_material): {name: torch tensor}, f32 maps
        [H, W, n_k] (albedo, specular reflectance of the smooth interface, mask opacity, roughness, emitted radiance — one value per wavenumber
        of `k`, 1 .. 4 of them in 1/mm; None: channel_wavenumbers()) and int32 ids [H, W] holding the u32 bits (material: its index; type: the
        leaf type at k[0]; -1 = 0xFFFFFFFF without a hit) — views of one allocation per group.  The rays are first_hit's for the same samples and
        seed; the maps are means over the rays that hit, the ids the first hitting ray's.  Enqueued on `stream` (default: torch's current)."""
        dev = self._uploaded_device("first_hit_material")
        spec, layouts, Ks = self._first_hit_material_args(samples, seed, k, maps, ids)
        arrays, (m, i) = _map_outputs([(self.height, self.width, K) for K in Ks], dev)
        _check(load_library().wtgpu_first_hit_material(self._h, self._stream_arg(stream, dev), C.byref(spec), m, i))
        return _views(layouts, arrays)

    def first_hit_material_host(self, samples=0, seed=1, k=None, maps=("albedo", "specular", "opacity", "roughness", "emission"),
                                ids=("material", "type"), threads=0):
        """The same maps on host threads (wtgpu_first_hit_material_host; threads 0 = all cores), as numpy (ids: uint32): bit for bit the device's."""
        spec, layouts, Ks = self._first_hit_material_args(samples, seed, k, maps, ids)
        arrays, (m, i) = _map_outputs([(self.height, self.width, K) for K in Ks])
        _check(load_library().wtgpu_first_hit_material_host(self._h, C.byref(spec), int(threads), m, i))
        return _views(layouts, arrays)

    def _los_args(self, samples, seed, emitters, maps, elem, ids, front_only, t_min):
        """-> (wtgpu_los_spec, the layouts of the pair maps, the element maps and the ids, their [H, W, ...] shapes); names in any order, memory
        in bit order."""
        mbits, mlay, K = _bit_groups(maps, LOS_MAPS, "map", "line_of_sight")
        ebits, elay, Ke = _bit_groups(elem, LOS_ELEM, "element map", "line_of_sight")
        ibits, ilay, Ki = _bit_groups(ids, LOS_IDS, "id", "line_of_sight")
        if emitters is None:
            sel = []
            E = sum(1 for e in self.emitter_summary() if e["type"] != "area")
        else:
            sel = [int(e) for e in ([emitters] if isinstance(emitters, int) else emitters)]
            E = len(sel)
            if E == 0 or E > LOS_MAX_EMITTERS or min(sel) < 0:
                raise ValueError(f"line_of_sight: 1 .. {LOS_MAX_EMITTERS} emitter indices expected (None: every emitter that is not an area emitter)")
        spec = LosSpec(int(samples), mbits, ebits, ibits, LOS_FRONT_ONLY if front_only else 0, len(sel), (C.c_uint32 * 32)(*sel), float(t_min), 0, int(seed))
        return spec, (mlay, elay, ilay), [(self.height, self.width, E, K), (self.height, self.width, Ke), (self.height, self.width, Ki)]

    def line_of_sight(self, samples=0, seed=1, emitters=None, maps=("visible", "distance"), elem=(), ids=("n_visible", "nearest"), front_only=True,
                      points=None, normals=None, mask=None, t_min=0.0, stream=None):
        """Line-of-sight maps on the scene's device (wtgpu_line_of_sight): which of the selected emitters every element sees.  {name: torch
        tensor}: the pair maps [H, W, E] (visible: the share of the element's samples that see the emitter; distance; cos) or [H, W, E, 3]
        (direction), means over all samples; the element maps point [H, W, 3] and nearest_distance [H, W]; the ids n_visible and nearest [H, W],
        int32 holding the u32 bits (nearest: the index within the selection, -1 = 0xFFFFFFFF where no emitter is seen) — views of one
        allocation per group.  emitters: None = every emitter that is not an area emitter, in the order of emitter_summary(), or indices in
        that order.  points: None = the elements of the virtual-plane sensor (samples 0: their centres; n >= 1: n points per element drawn
        from `seed`), or a contiguous f32 tensor [H, W, 3] on the device (Scene.first_hit's position), with normals the same or None;
        front_only and cos need a normal.  mask: None or f32 [H, W] there, elements with mask <= 0 trace nothing and hold 0 / -1.  t_min: the
        start of the rays' range (a surface point must not shadow itself).  Enqueued on `stream` (default: torch's current)."""
        import torch
        dev = self._uploaded_device("line_of_sight")
        n = self.width * self.height
        for t, name, numel in ((points, "points", 3 * n), (normals, "normals", 3 * n), (mask, "mask", n)):
            if t is not None and not (t.is_cuda and t.device.index == self.device and t.dtype == torch.float32 and t.numel() == numel and t.is_contiguous()):
                raise ValueError(f"line_of_sight: {name}: a contiguous torch.float32 tensor of {numel} elements on cuda:{self.device} expected")
        spec, layouts, shapes = self._los_args(samples, seed, emitters, maps, elem, ids, front_only, t_min)
        arrays, (m, e, i) = _map_outputs(shapes, dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        _check(load_library().wtgpu_line_of_sight(self._h, self._stream_arg(stream, dev), C.byref(spec), ptr(points), ptr(normals), ptr(mask), m, e, i))
        return _views(layouts, arrays)

    def line_of_sight_host(self, samples=0, seed=1, emitters=None, maps=("visible", "distance"), elem=(), ids=("n_visible", "nearest"), front_only=True,
                           points=None, normals=None, mask=None, t_min=0.0, threads=0):
        """The same maps on host threads (wtgpu_line_of_sight_host; threads 0 = all cores) from numpy points / normals / mask, as numpy (ids:
        uint32): bit for bit the device's."""
        import numpy as np
        n = self.width * self.height
        points, normals, mask = (None if t is None else np.ascontiguousarray(t, dtype=np.float32) for t in (points, normals, mask))
        for t, name, numel in ((points, "points", 3 * n), (normals, "normals", 3 * n), (mask, "mask", n)):
            if t is not None and t.size != numel:
                raise ValueError(f"line_of_sight_host: {name}: {numel} floats expected")
        spec, layouts, shapes = self._los_args(samples, seed, emitters, maps, elem, ids, front_only, t_min)
        arrays, (m, e, i) = _map_outputs(shapes)
        ptr = lambda t: None if t is None else t.ctypes.data
        _check(load_library().wtgpu_line_of_sight_host(self._h, C.byref(spec), ptr(points), ptr(normals), ptr(mask), int(threads), m, e, i))
        return _views(layouts, arrays)

    @property
    def tonemap_spec(self):
        """The <tonemap> of the scene file's <response> (tonemap_t::load, src/sensor/response/tonemap.cpp:127-176) as a dict: present, op (linear |
        gamma | sRGB | dB | function), mode (select | normal | colourmap), gamma, db_range, colourmap (the map's name), function.  present =
        False (no node, or no file): the response's default — sRGB / normal for an RGB film, linear / select for a monochromatic one, map Magma."""
        s = TonemapSpec()
        _check(load_library().wtgpu_scene_tonemap_spec(self._h, C.byref(s)))
        return {"present": bool(s.present), "op": TONEMAP_OPS[s.op], "mode": TONEMAP_MODES[s.mode], "gamma": float(s.gamma),
                "db_range": (float(s.db_min), float(s.db_max)), "colourmap": s.colourmap.decode(), "function": s.function.decode()}

    @staticmethod
    def _tonemap_struct(tm):
        """tm: None (the scene's own spec) or a dict like tonemap_spec's with an optional "table" ([n,3] f32) -> (wtgpu_tonemap or None, keepalive)."""
        import numpy as np
        if tm is None:
            return None, None
        table = tm.get("table")
        tab = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
        if tab is not None and (tab.ndim != 2 or tab.shape[1] != 3):
            raise ValueError(f"table: [n, 3] expected, got shape {tab.shape}")
        db = tm.get("db_range", (0.0, 0.0))
        st = Tonemap(TONEMAP_OPS.index(tm.get("op", "linear")), TONEMAP_MODES.index(tm.get("mode", "select")), float(tm.get("gamma", 2.2)),
                     float(db[0]), float(db[1]), None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_float)), 0 if tab is None else len(tab))
        return st, tab

    @staticmethod
    def _stream_arg(stream, dev):
        """The void* a device entry point takes for `stream` (None: torch's current stream on `dev`; its null stream goes as NULL)."""
        import torch
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        return C.c_void_p(st) if st else None

    def _host_films(self, what, value, weight, light, mask=None):
        """_device_films' numpy mirror for the host twins: contiguous f64 films (and an f32 mask or None) of the scene's size, or a refusal."""
        import numpy as np
        v, w, l = (np.ascontiguousarray(t, dtype=np.float64) for t in (value, weight, light))
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        n = self.width * self.height
        if v.size != n * self.channels or l.size != v.size or w.size != n or (m is not None and m.size != n):
            raise ValueError(f"{what}: films of the scene's size expected")
        return v, w, l, m

    def _device_films(self, what, value, weight, light, mask=None):
        """The device entry points read the films by their sizes: refuse tensors of another size, type or device before a kernel does."""
        import torch
        if self.device is None:
            raise WtgpuError(f"{what}: upload(device) first")
        n = self.width * self.height
        for t, name, numel, dtype in ((value, "value", n * self.channels, torch.float64), (weight, "weight", n, torch.float64),
                                      (light, "light", n * self.channels, torch.float64), (mask, "mask", n, torch.float32)):
            if t is None and name == "mask":
                continue
            if not (t.is_cuda and t.device.index == self.device and t.dtype == dtype and t.numel() == numel and t.is_contiguous()):
                raise ValueError(f"{what}: {name}: a contiguous {dtype} tensor of {numel} elements on cuda:{self.device} expected")
        return torch.device("cuda", self.device)

    # ---- a film source (wtgpu_film_source): the accumulators (value, weight, light) with spe, or ONE developed f32 film ----
    def _device_source(self, what, films, spe, mask=None):
        """films: the (value, weight, light) f64 tensors with spe, or one developed f32 tensor of the scene's planes (develop_device's, the
        denoiser's "film" or "residual") -> (FilmSource, torch device).  A film of another dtype, size, device or layout is refused here."""
        import torch
        if isinstance(films, (tuple, list)):
            value, weight, light = films
            dev = self._device_films(what, value, weight, light, mask)
            return FilmSource(value.data_ptr(), weight.data_ptr(), light.data_ptr(), int(spe), None), dev
        if self.device is None:
            raise WtgpuError(f"{what}: upload(device) first")
        n = self.width * self.height
        if not (isinstance(films, torch.Tensor) and films.is_cuda and films.device.index == self.device and films.dtype == torch.float32
                and films.numel() == n * self.channels and films.is_contiguous()):
            raise ValueError(f"{what}: film: a contiguous torch.float32 tensor [{self.height}, {self.width}, {self.spectral_channels}, {self.stokes}] "
                             f"({n * self.channels} elements) on cuda:{self.device} expected")
        if mask is not None and not (mask.is_cuda and mask.device.index == self.device and mask.dtype == torch.float32 and mask.numel() == n and mask.is_contiguous()):
            raise ValueError(f"{what}: mask: a contiguous torch.float32 tensor of {n} elements on cuda:{self.device} expected")
        return FilmSource(None, None, None, 0, films.data_ptr()), torch.device("cuda", self.device)

    def _host_source(self, what, films, spe, mask=None):
        """_device_source's numpy mirror for the host twins -> (FilmSource, the f32 mask or None, the arrays the pointers live in).  A developed film
        is taken as it is — a contiguous float32 array of the scene's planes — never converted: its bits are the input."""
        import numpy as np
        if isinstance(films, (tuple, list)):
            v, w, l, m = self._host_films(what, *films, mask)
            return FilmSource(v.ctypes.data, w.ctypes.data, l.ctypes.data, int(spe), None), m, (v, w, l, m)
        n = self.width * self.height
        if not (isinstance(films, np.ndarray) and films.dtype == np.float32 and films.size == n * self.channels and films.flags.c_contiguous):
            raise ValueError(f"{what}: film: a contiguous float32 array [{self.height}, {self.width}, {self.spectral_channels}, {self.stokes}] "
                             f"({n * self.channels} elements) expected")
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        if m is not None and m.size != n:
            raise ValueError(f"{what}: a mask of the scene's size expected")
        return FilmSource(None, None, None, 0, films.ctypes.data), m, (films, m)

    def develop_device(self, value, weight, light, spe, stream=None):
        """wtgpu_develop on the scene's device (wtgpu_develop_device): value / weight / light are the torch f64 films there; returns the developed
        film as a torch f32 tensor shaped like `value`, bit for bit render.develop's.  Enqueued on `stream` (default: torch's current)."""
        import torch
        dev = self._device_films("develop_device", value, weight, light)
        out = torch.empty(tuple(value.shape), dtype=torch.float32, device=dev)
        _check(load_library().wtgpu_develop_device(self._h, self._stream_arg(stream, dev), value.data_ptr(), weight.data_ptr(), light.data_ptr(), int(spe),
                                                   out.data_ptr()))
        return out

    def _tonemap_device(self, what, films, spe, tm, stokes_component, mask, fmt, stream):
        import torch
        src, dev = self._device_source(what, films, spe, mask)
        st_tm, keep = self._tonemap_struct(tm)
        dtype = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.int16}[fmt]
        out = torch.empty((self.height, self.width, 4 if mask is not None else 3), dtype=dtype, device=dev)
        _check(load_library().wtgpu_tonemap_source_device(self._h, self._stream_arg(stream, dev), C.byref(src), None if st_tm is None else C.byref(st_tm),
                                                          int(stokes_component), None if mask is None else mask.data_ptr(), TONEMAP_FORMATS[fmt], out.data_ptr()))
        del keep
        return out

    def _tonemap_host(self, what, films, spe, tm, stokes_component, mask, fmt, threads):
        import numpy as np
        src, m, keep_films = self._host_source(what, films, spe, mask)
        st_tm, keep = self._tonemap_struct(tm)
        out = np.zeros((self.height, self.width, 4 if m is not None else 3), {"f32": np.float32, "u8": np.uint8, "u16": np.uint16}[fmt])
        _check(load_library().wtgpu_tonemap_source_host(self._h, C.byref(src), None if st_tm is None else C.byref(st_tm), int(stokes_component),
                                                        None if m is None else m.ctypes.data, TONEMAP_FORMATS[fmt], int(threads), out.ctypes.data))
        del keep, keep_films
        return out

    def tonemap_device(self, value, weight, light, spe, tm=None, stokes_component=0, mask=None, fmt="f32", stream=None):
        """Develops and tonemaps one Stokes component of the films on the scene's device in one kernel (wtgpu_tonemap_device).  tm: None = the
        scene's own tonemap_spec, else a dict {op, mode, gamma, db_range, table} (table: [n,3] f32 colour map, imageio.colour_table).  mask: an
        H x W f32 torch tensor on the device (sensor_mask) that becomes the alpha.  fmt: f32 | u8 | u16.  Returns a torch tensor H x W x 3 (x 4
        with a mask) of float32 / uint8 / int16 (the 16-bit codes: view them as unsigned)."""
        return self._tonemap_device("tonemap_device", (value, weight, light), spe, tm, stokes_component, mask, fmt, stream)

    def tonemap_host(self, value, weight, light, spe, tm=None, stokes_component=0, mask=None, fmt="f32", threads=0):
        """The same computation on host threads from numpy films (wtgpu_tonemap_host; threads 0 = all cores): a numpy array H x W x 3 (x 4 with
        a mask) of float32 / uint8 / uint16.  No device needed."""
        return self._tonemap_host("tonemap_host", (value, weight, light), spe, tm, stokes_component, mask, fmt, threads)

    def tonemap_developed_device(self, film, tm=None, stokes_component=0, mask=None, fmt="f32", stream=None):
        """tonemap_device of a DEVELOPED film where it is (wtgpu_tonemap_source_device): film a torch f32 tensor [H, W, channels, stokes] on the scene's
        device — develop_device's result, film_denoise_device's "film" or "residual".  The other arguments and the result are tonemap_device's; on
        develop_device's output of a set of accumulators the picture is tonemap_device's of those accumulators."""
        return self._tonemap_device("tonemap_developed_device", film, 0, tm, stokes_component, mask, fmt, stream)

    def tonemap_developed_host(self, film, tm=None, stokes_component=0, mask=None, fmt="f32", threads=0):
        """tonemap_developed_device's twin on host threads (wtgpu_tonemap_source_host): film a contiguous numpy float32 array of the scene's planes."""
        return self._tonemap_host("tonemap_developed_host", film, 0, tm, stokes_component, mask, fmt, threads)

    # ---- film statistics (wtgpu_film_stats_*; csrc/wt/film_stats.h) ----
    def _film_stats(self, what, call, stokes_component, scale, range, bins, abs, luminance):
        """The one or two passes of film_stats_device / film_stats_host.  call(spec, records, hist_pointer_or_None) runs one pass."""
        import numpy as np
        if scale not in FILM_STATS_SCALES:
            raise ValueError(f"{what}: scale 'dB' or 'linear' expected, got {scale!r}")
        planes = self.spectral_channels + (1 if luminance else 0)
        flags = (FILM_STATS_ABS if abs else 0) | (FILM_STATS_LUMINANCE if luminance else 0)

        def one_pass(lo, hi, nbins):
            spec = FilmStatsSpec(int(stokes_component), FILM_STATS_SCALES.index(scale), int(nbins), flags, float(lo), float(hi))
            rec = (FilmStats * max(planes, 1))()
            hist = np.zeros((planes, min(int(nbins), FILM_STATS_MAX_BINS)), dtype=np.uint64)
            call(spec, rec, hist.ctypes.data if hist.size else None)
            return spec, rec, hist

        if range is None:
            # the range pass: no bins; then the histogram from the smallest positive (dB) or smallest (linear) to the largest element of all planes
            _, rec, _ = one_pass(0.0, 0.0, 0)
            lows = np.array([r.min_positive if scale == "dB" else r.min for r in rec], dtype=np.float64)
            highs = np.array([r.max for r in rec], dtype=np.float64)
            if np.isnan(lows).all() or not np.isfinite(np.nanmax(highs)):
                raise ValueError(f"{what}: range=None needs a finite {'positive ' if scale == 'dB' else ''}element to take the range from; pass a range")
            lo, hi = float(np.nanmin(lows)), float(np.nanmax(highs))
            if scale == "dB":
                # a margin of 1e-3 dB (2e-4 of the value, far above f32 rounding) keeps both ends inside the bins
                lo, hi = 10.0 * math.log10(lo) - 1e-3, 10.0 * math.log10(hi) + 1e-3
            else:
                pad = max(math.fabs(lo), math.fabs(hi), 1e-30) * 1e-6
                lo, hi = lo - pad, hi + pad
            range = (lo, hi)
        spec, rec, hist = one_pass(range[0], range[1], bins)
        edges = np.zeros(spec.bins + 1, dtype=np.float32)
        _check(load_library().wtgpu_film_stats_edges(C.byref(spec), edges.ctypes.data))
        out = {name: np.array([getattr(r, name) for r in rec], dtype=dt) for name, dt in
               (("n", np.uint64), ("n_nan", np.uint64), ("n_negative", np.uint64), ("n_zero", np.uint64), ("n_below", np.uint64), ("n_above", np.uint64),
                ("min", np.float32), ("max", np.float32), ("min_positive", np.float32), ("sum", np.float64))}
        out.update(hist=hist, edges=edges, scale=scale, range=(float(spec.lo), float(spec.hi)), bins=int(spec.bins))
        return out

    def _film_stats_device(self, what, films, spe, stokes_component, scale, range, bins, abs, luminance, mask, stream):
        src, dev = self._device_source(what, films, spe, mask)
        st = self._stream_arg(stream, dev)
        lib = load_library()

        def call(spec, rec, hist):
            _check(lib.wtgpu_film_stats_source_device(self._h, st, C.byref(src), C.byref(spec), None if mask is None else mask.data_ptr(), C.cast(rec, C.c_void_p), hist))
        return self._film_stats(what, call, stokes_component, scale, range, bins, abs, luminance)

    def _film_stats_host(self, what, films, spe, stokes_component, scale, range, bins, abs, luminance, mask, threads):
        src, m, keep = self._host_source(what, films, spe, mask)
        lib = load_library()

        def call(spec, rec, hist):
            _check(lib.wtgpu_film_stats_source_host(self._h, C.byref(src), C.byref(spec), None if m is None else m.ctypes.data, int(threads), C.cast(rec, C.c_void_p), hist))
        out = self._film_stats(what, call, stokes_component, scale, range, bins, abs, luminance)
        del keep
        return out

    def film_stats_device(self, value, weight, light, spe, *, stokes_component=0, scale="dB", range=None, bins=256, abs=False, luminance=False, mask=None,
                          stream=None):
        """Range, histogram and sum of the developed planes of one Stokes component, computed where the films are (wtgpu_film_stats_device): value /
        weight / light are the torch f64 films on the scene's device, mask an H x W f32 tensor there (sensor_mask; elements of pixels with
        mask > 0 count) or None.  One record per channel, plus the BT.709 luminance of an RGB film with luminance=True; abs=True takes |x|.
        scale / range / bins: the histogram's axis, `bins` equal steps from range[0] to range[1] in dB (10 log10 x) or linear units.
        range=None: two passes, the first without bins for the smallest positive (dB) or smallest (linear) and the largest element.
        Returns a dict of numpy arrays indexed by plane: n, n_nan, n_negative, n_zero, n_below, n_above (uint64), min, max, min_positive
        (float32), sum (float64), hist [planes, bins] uint64; and edges [bins + 1] float32, scale, range, bins.  imageio.percentiles reads it."""
        return self._film_stats_device("film_stats_device", (value, weight, light), spe, stokes_component, scale, range, bins, abs, luminance, mask, stream)

    def film_stats_host(self, value, weight, light, spe, *, stokes_component=0, scale="dB", range=None, bins=256, abs=False, luminance=False, mask=None,
                        threads=0):
        """film_stats_device's twin on host threads from numpy films (wtgpu_film_stats_host; threads 0 = all cores): the same dict, every field bit
        for bit the device's.  No device needed."""
        return self._film_stats_host("film_stats_host", (value, weight, light), spe, stokes_component, scale, range, bins, abs, luminance, mask, threads)

    def film_stats_developed_device(self, film, *, stokes_component=0, scale="dB", range=None, bins=256, abs=False, luminance=False, mask=None, stream=None):
        """film_stats_device of a DEVELOPED film where it is (wtgpu_film_stats_source_device): film a torch f32 tensor [H, W, channels, stokes] on the
        scene's device (develop_device's result, film_denoise_device's "film" or "residual"); the elements are its values as they lie there.  The
        other arguments and the dict are film_stats_device's."""
        return self._film_stats_device("film_stats_developed_device", film, 0, stokes_component, scale, range, bins, abs, luminance, mask, stream)

    def film_stats_developed_host(self, film, *, stokes_component=0, scale="dB", range=None, bins=256, abs=False, luminance=False, mask=None, threads=0):
        """film_stats_developed_device's twin on host threads (wtgpu_film_stats_source_host): film a contiguous numpy float32 array of the scene's planes."""
        return self._film_stats_host("film_stats_developed_host", film, 0, stokes_component, scale, range, bins, abs, luminance, mask, threads)

    # ---- zonal film statistics (wtgpu_film_zonal_*; csrc/wt/film_zonal.h) ----
    def _film_zonal(self, what, xp_zones, call, n_zones, stokes_component, scale, range, bins, abs, luminance, paint):
        """What film_zonal_device / film_zonal_host share: the spec, the records as a dict.  xp_zones: the zone plane's ids below 0xFFFFFFFF as a
        callable giving their maximum (or None where there is none); call(spec, rec, hist_or_None, n_outside, planes) runs the pass."""
        import numpy as np
        if scale not in FILM_STATS_SCALES:
            raise ValueError(f"{what}: scale 'dB' or 'linear' expected, got {scale!r}")
        if n_zones is None:
            top = xp_zones()
            n_zones = 1 if top is None else top + 1
            if n_zones > FILM_ZONAL_MAX_ZONES:
                raise ValueError(f"{what}: the zone plane holds id {top}: more than {FILM_ZONAL_MAX_ZONES} zones (pass n_zones, or relabel)")
        planes = self.spectral_channels + (1 if luminance else 0)
        flags = (FILM_STATS_ABS if abs else 0) | (FILM_STATS_LUMINANCE if luminance else 0)
        lo, hi = (0.0, 0.0) if range is None else range
        if range is None and bins:
            raise ValueError(f"{what}: bins > 0 needs a range (lo, hi) in the scale's units")
        spec = FilmZonalSpec(int(stokes_component), FILM_STATS_SCALES.index(scale), int(bins), flags, int(n_zones), float(lo), float(hi))
        zones_ok = 0 < spec.n_zones <= FILM_ZONAL_MAX_ZONES and spec.bins <= FILM_STATS_MAX_BINS and spec.n_zones * spec.bins <= 1 << 20   # (the library says why not)
        rec = np.zeros((spec.n_zones if zones_ok else 1, max(planes, 1)), dtype=np.dtype(FILM_ZONAL_FIELDS))
        hist = np.zeros((spec.n_zones, planes, spec.bins) if zones_ok else (0, planes, 0), dtype=np.uint64)
        n_outside = C.c_uint64(0)
        extra = call(spec, rec, hist.ctypes.data if hist.size else None, n_outside, planes)
        out = {name: np.ascontiguousarray(rec[name]) for name, _ in FILM_ZONAL_FIELDS}
        n_finite = (out["n"] - out["n_nan"] - out["n_inf"]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean"] = out["sum"] / n_finite
        edges = np.zeros(spec.bins + 1, dtype=np.float32)
        fs = FilmStatsSpec(spec.stokes_component, spec.scale, spec.bins, spec.flags, spec.lo, spec.hi)
        _check(load_library().wtgpu_film_stats_edges(C.byref(fs), edges.ctypes.data))
        out.update(hist=hist, edges=edges, n_outside=int(n_outside.value), n_zones=int(spec.n_zones), scale=scale, range=(float(spec.lo), float(spec.hi)), bins=int(spec.bins))
        if paint:
            out["paint"] = extra
        return out

    def film_zonal_device(self, film, spe, zones, n_zones=None, *, stokes_component=0, abs=False, luminance=False, mask=None, scale="linear", range=None, bins=0,
                          paint=False, stream=None):
        """Statistics per zone of a label plane in ONE pass where the films are (wtgpu_film_zonal_device): film is the (value, weight, light) triple of
        torch f64 tensors on the scene's device, developed with spe samples per element, or one developed f32 film there (spe is then not read), as
        film_compare_device takes its operands; zones a contiguous torch int32 tensor [H, W] there holding the u32 ids (first_hit's shape /
        triangle, first_hit_material's, line_of_sight's n_visible / nearest, render.zones_from_edges, render.cell_zones; torch.uint32 is taken too).
        A pixel with mask > 0 (or any, without a mask) and an id below n_zones belongs to that zone, any other to none (counted in n_outside);
        n_zones=None: the largest id below 0xFFFFFFFF plus one.  stokes_component / abs / luminance / scale / range / bins: film_stats_device's
        (range is needed only with bins > 0; without bins, range[0] — default 0 — splits the positive elements into below and above).
        Returns a dict of numpy arrays [n_zones, planes]: n, n_nan, n_inf, n_negative, n_zero, n_below, n_above (uint64), min, max (float32), sum
        (float64: the EXACT sum of the zone's finite elements rounded once, math.fsum's) and mean = sum / (n - n_nan - n_inf); hist [n_zones,
        planes, bins] uint64; edges, n_outside, n_zones, scale, range, bins.  paint=True adds "paint": a torch f32 tensor [H, W, planes] on the
        device, every pixel holding its zone's mean (0 outside the mask and the zones) — a developed film that render.view shows."""
        import torch
        src, dev = self._device_source("film_zonal_device", film, spe or 0, mask)
        n = self.width * self.height
        if not (isinstance(zones, torch.Tensor) and zones.is_cuda and zones.device.index == self.device and zones.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))
                and tuple(zones.shape) == (self.height, self.width) and zones.is_contiguous()):
            raise ValueError(f"film_zonal_device: zones: a contiguous torch.int32 (or uint32) tensor [{self.height}, {self.width}] ({n} ids) on cuda:{self.device} expected")
        st = self._stream_arg(stream, dev)

        def top():
            z = zones.view(torch.int32).reshape(-1)
            z = z[z != -1]
            if z.numel() == 0:
                return None
            return int(z.to(torch.int64).remainder(1 << 32).max().item())

        def call(spec, rec, hist, n_outside, planes):
            d_paint = torch.empty((self.height, self.width, planes), dtype=torch.float32, device=dev) if paint else None
            _check(load_library().wtgpu_film_zonal_device(self._h, st, C.byref(src), C.byref(spec), zones.data_ptr(), None if mask is None else mask.data_ptr(),
                                                          rec.ctypes.data, hist, C.byref(n_outside), None if d_paint is None else d_paint.data_ptr()))
            return d_paint
        return self._film_zonal("film_zonal_device", top, call, n_zones, stokes_component, scale, range, bins, abs, luminance, paint)

    def film_zonal_host(self, film, spe, zones, n_zones=None, *, stokes_component=0, abs=False, luminance=False, mask=None, scale="linear", range=None, bins=0,
                        paint=False, threads=0):
        """film_zonal_device's twin on host threads from numpy arrays (wtgpu_film_zonal_host; threads 0 = all cores): the same dict, every field bit for
        bit the device's, "paint" a numpy array.  zones: a contiguous int32 or uint32 array [H, W].  No device needed."""
        import numpy as np
        src, m, keep = self._host_source("film_zonal_host", film, spe or 0, mask)
        if not (isinstance(zones, np.ndarray) and zones.dtype in (np.int32, np.uint32) and zones.shape == (self.height, self.width) and zones.flags.c_contiguous):
            raise ValueError(f"film_zonal_host: zones: a contiguous int32 or uint32 array [{self.height}, {self.width}] expected")

        def top():
            z = zones.view(np.uint32)
            z = z[z != FILM_ZONAL_NO_ZONE]
            return int(z.max()) if z.size else None

        def call(spec, rec, hist, n_outside, planes):
            out = np.zeros((self.height, self.width, planes), dtype=np.float32) if paint else None
            _check(load_library().wtgpu_film_zonal_host(self._h, C.byref(src), C.byref(spec), zones.ctypes.data, None if m is None else m.ctypes.data, int(threads),
                                                        rec.ctypes.data, hist, C.byref(n_outside), None if out is None else out.ctypes.data))
            return out
        out = self._film_zonal("film_zonal_host", top, call, n_zones, stokes_component, scale, range, bins, abs, luminance, paint)
        del keep
        return out

    # ---- connected segments of a label plane (wtgpu_film_segments_*; csrc/wt/film_segments.h) ----
    def _film_segments(self, what, call, diagonal, min_area, max_records):
        """What film_segments_device / film_segments_host share: the spec, the info and the records as a dict.  call(spec, info, rec) runs the pass and
        returns the segment plane."""
        import numpy as np
        if int(min_area) < 0 or int(max_records) < 0:
            raise ValueError(f"{what}: min_area and max_records must not be negative")
        n_rec = min(int(max_records), self.width * self.height)       # (there are never more segments than pixels)
        spec = FilmSegmentsSpec(FILM_SEGMENTS_DIAGONAL if diagonal else 0, int(min_area), n_rec, 0)
        info = FilmSegmentsInfo()
        rec = np.zeros(n_rec, dtype=np.dtype(FILM_SEGMENT_FIELDS))
        segments = call(spec, info, rec.ctypes.data if n_rec else None)
        rec = rec[:min(int(info.n_segments), n_rec)]
        area = rec["area"].astype(np.float64)
        return {"segments": segments, "n_segments": int(info.n_segments), "n_dropped": int(info.n_dropped), "n_members": int(info.n_members),
                "n_dropped_pixels": int(info.n_dropped_pixels), "klass": np.ascontiguousarray(rec["klass"]), "area": np.ascontiguousarray(rec["area"]),
                "first": np.ascontiguousarray(rec["first"]), "bbox": np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], axis=1),
                "centroid": np.stack([rec["sum_x"] / area, rec["sum_y"] / area], axis=1)}

    def film_segments_device(self, classes=None, *, mask=None, diagonal=False, min_area=1, max_records=65536, stream=None):
        """The connected segments of a label plane where it is (wtgpu_film_segments_device): which REGION a pixel lies in, where the id maps say which
        class.  classes: a contiguous torch int32 tensor [H, W] on the scene's device holding the u32 ids (first_hit's, line_of_sight's, a zone
        plane; torch.uint32 is taken too), or None: every pixel has class 0.  A pixel is a member iff mask > 0 (or any, without a mask: a torch f32
        tensor [H, W] there) and its class is not 0xFFFFFFFF; members of one class that are edge neighbours — diagonal=True: or corner
        neighbours — are linked, and a segment is a connected component.  Segments of at least max(min_area, 1) pixels are kept and numbered
        from 0 in the order of their first (smallest row-major) pixel.  Returns a dict: "segments", a torch int32 tensor [H, W] there holding the
        number of the pixel's segment, -1 (0xFFFFFFFF) for no member or a dropped segment — film_zonal_device takes it as zones as it is;
        n_segments, n_dropped, n_members, n_dropped_pixels (int); and of the first min(n_segments, max_records) segments the numpy arrays klass, area,
        first (uint32), bbox [K', 4] (x0, y0, x1, y1, inclusive) and centroid [K', 2] (x, y; float64)."""
        import torch
        if self.device is None:
            raise WtgpuError("film_segments_device: upload(device) first")
        dev = torch.device("cuda", self.device)

        def plane(t, name, dtypes, words):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype in dtypes
                                      and tuple(t.shape) == (self.height, self.width) and t.is_contiguous()):
                raise ValueError(f"film_segments_device: {name}: a contiguous {words} tensor [{self.height}, {self.width}] on cuda:{self.device} expected")
            return None if t is None else t.data_ptr()
        d_classes = plane(classes, "classes", (torch.int32, getattr(torch, "uint32", torch.int32)), "torch.int32 (or uint32)")
        d_mask = plane(mask, "mask", (torch.float32,), "torch.float32")
        st = self._stream_arg(stream, dev)

        def call(spec, info, rec):
            out = torch.empty((self.height, self.width), dtype=torch.int32, device=dev)
            _check(load_library().wtgpu_film_segments_device(self._h, st, C.byref(spec), d_classes, d_mask, out.data_ptr(), C.byref(info), rec))
            return out
        return self._film_segments("film_segments_device", call, diagonal, min_area, max_records)

    def film_segments_host(self, classes=None, *, mask=None, diagonal=False, min_area=1, max_records=65536, threads=0):
        """film_segments_device's twin on the host from numpy arrays (wtgpu_film_segments_host): the same dict, every field bit for bit the device's,
        "segments" a numpy uint32 array.  classes: a contiguous int32 or uint32 array [H, W] or None; mask: a contiguous float32 array [H, W] or
        None.  The result does not depend on threads.  No device needed."""
        import numpy as np

        def plane(t, name, dtypes, words):
            if t is not None and not (isinstance(t, np.ndarray) and t.dtype in dtypes and t.shape == (self.height, self.width) and t.flags.c_contiguous):
                raise ValueError(f"film_segments_host: {name}: a contiguous {words} array [{self.height}, {self.width}] expected")
            return None if t is None else t.ctypes.data
        p_classes = plane(classes, "classes", (np.int32, np.uint32), "int32 or uint32")
        p_mask = plane(mask, "mask", (np.float32,), "float32")

        def call(spec, info, rec):
            out = np.zeros((self.height, self.width), dtype=np.uint32)
            _check(load_library().wtgpu_film_segments_host(self._h, C.byref(spec), p_classes, p_mask, int(threads), out.ctypes.data, C.byref(info), rec))
            return out
        return self._film_segments("film_segments_host", call, diagonal, min_area, max_records)

    # ---- distance transform of a label plane (wtgpu_film_distance_*; csrc/wt/film_distance.h) ----
    def film_distance_device(self, classes=None, *, mask=None, invert=False, nearest=False, stream=None):
        """The exact Euclidean distance transform of a label plane where it is (wtgpu_film_distance_device): how FAR each pixel lies from the nearest
        site, and which site that is.  classes: a contiguous torch int32 tensor [H, W] on the scene's device holding the u32 ids (torch.uint32 is
        taken too), or None: every pixel has class 0; mask: a torch f32 tensor [H, W] there or None.  A pixel is a member as for
        film_segments_device (mask > 0, or any without a mask, and a class other than 0xFFFFFFFF); the sites are the members, with invert=True the
        pixels that are none.  The film's outside holds no site.  Returns a dict: "dist2", a torch int32 tensor [H, W] there holding the u32 bits of
        the squared pixel distance to the nearest site (0 on a site; -1, 0xFFFFFFFF, everywhere where there is no site); "nearest", with nearest=True
        the same kind of tensor holding the row-major index of that site (of several equally far the smallest index; -1 without a site), else None;
        n_sites, max_dist2 (the largest dist2) and argmax (the lowest pixel index that attains it) as int."""
        import torch
        if self.device is None:
            raise WtgpuError("film_distance_device: upload(device) first")
        dev = torch.device("cuda", self.device)

        def plane(t, name, dtypes, words):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device.index == self.device and t.dtype in dtypes
                                      and tuple(t.shape) == (self.height, self.width) and t.is_contiguous()):
                raise ValueError(f"film_distance_device: {name}: a contiguous {words} tensor [{self.height}, {self.width}] on cuda:{self.device} expected")
            return None if t is None else t.data_ptr()
        d_classes = plane(classes, "classes", (torch.int32, getattr(torch, "uint32", torch.int32)), "torch.int32 (or uint32)")
        d_mask = plane(mask, "mask", (torch.float32,), "torch.float32")
        st = self._stream_arg(stream, dev)
        spec, info = FilmDistanceSpec(FILM_DISTANCE_INVERT if invert else 0), FilmDistanceInfo()
        dist2 = torch.empty((self.height, self.width), dtype=torch.int32, device=dev)
        near = torch.empty((self.height, self.width), dtype=torch.int32, device=dev) if nearest else None
        _check(load_library().wtgpu_film_distance_device(self._h, st, C.byref(spec), d_classes, d_mask, dist2.data_ptr(), near.data_ptr() if nearest else None, C.byref(info)))
        return {"dist2": dist2, "nearest": near, "n_sites": int(info.n_sites), "max_dist2": int(info.max_dist2), "argmax": int(info.argmax)}

    def film_distance_host(self, classes=None, *, mask=None, invert=False, nearest=False, threads=0):
        """film_distance_device's twin on the host from numpy arrays (wtgpu_film_distance_host): the same dict, every field bit for bit the device's,
        "dist2" and "nearest" numpy uint32 arrays.  classes: a contiguous int32 or uint32 array [H, W] or None; mask: a contiguous float32 array
        [H, W] or None.  The result does not depend on threads.  No device needed."""
        import numpy as np

        def plane(t, name, dtypes, words):
            if t is not None and not (isinstance(t, np.ndarray) and t.dtype in dtypes and t.shape == (self.height, self.width) and t.flags.c_contiguous):
                raise ValueError(f"film_distance_host: {name}: a contiguous {words} array [{self.height}, {self.width}] expected")
            return None if t is None else t.ctypes.data
        p_classes = plane(classes, "classes", (np.int32, np.uint32), "int32 or uint32")
        p_mask = plane(mask, "mask", (np.float32,), "float32")
        spec, info = FilmDistanceSpec(FILM_DISTANCE_INVERT if invert else 0), FilmDistanceInfo()
        dist2 = np.zeros((self.height, self.width), dtype=np.uint32)
        near = np.zeros((self.height, self.width), dtype=np.uint32) if nearest else None
        _check(load_library().wtgpu_film_distance_host(self._h, C.byref(spec), p_classes, p_mask, int(threads), dist2.ctypes.data, near.ctypes.data if nearest else None,
                                                       C.byref(info)))
        return {"dist2": dist2, "nearest": near, "n_sites": int(info.n_sites), "max_dist2": int(info.max_dist2), "argmax": int(info.argmax)}

    # ---- film comparison (wtgpu_film_compare_*; csrc/wt/film_compare.h) ----
    def _film_compare(self, call, stokes_component, abs, luminance, eps):
        """What film_compare_device / film_compare_host share: the spec, the records as a dict, the values derived from the sums."""
        import numpy as np
        planes = self.spectral_channels + (1 if luminance else 0)
        spec = FilmCompareSpec(int(stokes_component), (FILM_STATS_ABS if abs else 0) | (FILM_STATS_LUMINANCE if luminance else 0), float(eps))
        rec = (FilmCompare * max(planes, 1))()
        call(spec, rec, planes)
        out = {name: np.array([getattr(r, name) for r in rec], dtype=np.uint64 if t is C.c_uint64 else np.float64) for name, t in FILM_COMPARE_FIELDS}
        finite = (out["n"] - out["n_nonfinite"]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["rmse"] = np.sqrt(out["sum_sq"] / finite)
            out["mean_abs"] = out["sum_abs"] / finite
            out["rel_l2"] = np.sqrt(out["sum_sq"] / out["sum_b_sq"])
            out["rel_mse"] = out["sum_rel"] / finite
        return out

    def film_compare_device(self, films_a, spe_a, films_b, spe_b, *, stokes_component=0, abs=False, luminance=False, mask=None, eps=1e-4, diff=False, stream=None):
        """Difference statistics of two sets of films where they are (wtgpu_film_compare_device): films_a / films_b are (value, weight, light), torch f64
        tensors on the scene's device (the same tensors twice are fine), developed with spe_a / spe_b samples per element; mask an H x W f32 tensor there
        (pixels with mask > 0 count) or None.  One record per channel of Stokes component `stokes_component`, plus the BT.709 luminance of an RGB film
        with luminance=True; abs=True compares |xa| with |xb|.  Returns a dict of numpy arrays indexed by plane: n, n_nonfinite, n_nonfinite_mismatch,
        n_differ, argmax (uint64; the row-major pixel of max_abs, 2^64 - 1 where nothing differs), max_abs, sum_abs, sum_sq, sum_a_sq, sum_b_sq, sum_rel
        (float64; over the pairs of finite values, d = xa - xb) and, derived here from the sums, rmse, mean_abs, rel_l2 = sqrt(sum_sq / sum_b_sq) and
        rel_mse = sum_rel / (n - n_nonfinite) with sum_rel's addends d d / (xb xb + eps) (NaN where there is nothing to divide by).  diff=True adds
        "diff": xa - xb as a torch f32 tensor H x W x planes on the device, 0 where the mask excludes.
        Either operand may instead be ONE developed film, a torch f32 tensor [H, W, channels, stokes] there (develop_device's result, the denoiser's
        "film"): its values are compared as they lie there and its spe is not read (None will do) — a denoised film against a long render's
        accumulators (wtgpu_film_compare_source_device)."""
        import torch
        src_a, dev = self._device_source("film_compare_device", films_a, spe_a or 0, mask)
        src_b, _ = self._device_source("film_compare_device", films_b, spe_b or 0)
        st = self._stream_arg(stream, dev)
        d = {}

        def call(spec, rec, planes):
            if diff:
                d["diff"] = torch.empty((self.height, self.width, planes), dtype=torch.float32, device=dev)
            _check(load_library().wtgpu_film_compare_source_device(self._h, st, C.byref(src_a), C.byref(src_b), C.byref(spec), None if mask is None else mask.data_ptr(),
                                                                   C.cast(rec, C.c_void_p), d["diff"].data_ptr() if diff else None))
        out = self._film_compare(call, stokes_component, abs, luminance, eps)
        out.update(d)
        return out

    def film_compare_host(self, films_a, spe_a, films_b, spe_b, *, stokes_component=0, abs=False, luminance=False, mask=None, eps=1e-4, diff=False, threads=0):
        """film_compare_device's twin on host threads from numpy films (wtgpu_film_compare_host; threads 0 = all cores): the same dict, every field bit
        for bit the device's, "diff" a numpy array.  No device needed.  Either operand may be one developed film, a contiguous numpy float32 array of the scene's
        planes, as film_compare_device's (wtgpu_film_compare_source_host)."""
        import numpy as np
        src_a, _, keep_a = self._host_source("film_compare_host", films_a, spe_a or 0)
        src_b, _, keep_b = self._host_source("film_compare_host", films_b, spe_b or 0)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        if m is not None and m.size != self.width * self.height:
            raise ValueError("film_compare_host: a mask of the scene's size expected")
        d = {}

        def call(spec, rec, planes):
            if diff:
                d["diff"] = np.zeros((self.height, self.width, planes), dtype=np.float32)
            _check(load_library().wtgpu_film_compare_source_host(self._h, C.byref(src_a), C.byref(src_b), C.byref(spec), None if m is None else m.ctypes.data,
                                                                 int(threads), C.cast(rec, C.c_void_p), d["diff"].ctypes.data if diff else None))
        out = self._film_compare(call, stokes_component, abs, luminance, eps)
        out.update(d)
        del keep_a, keep_b
        return out

    # ---- the polarisation view of a Stokes film (wtgpu_film_polar_*; csrc/wt/film_polar.h) ----
    def _film_polar(self, what, call, luminance, maps, analyser, c2s2, picture, picture_plane, tm, fmt, sat_gain, masked):
        """What film_polar_device / film_polar_host share: the spec, the records as a dict, the values derived from the sums, the maps by name.
        call(spec, records, maps_shape_or_None, picture_shape_or_None) runs the pass and returns (maps array or None, picture or None)."""
        import numpy as np
        names = [maps] if isinstance(maps, str) else list(maps)
        for m in names:
            if m not in FILM_POLAR_MAPS:
                raise ValueError(f"{what}: maps of {FILM_POLAR_MAPS} expected, got {m!r}")
        if fmt not in TONEMAP_FORMATS:
            raise ValueError(f"{what}: fmt f32, u8 or u16 expected, got {fmt!r}")
        names = [m for m in FILM_POLAR_MAPS if m in names]
        planes = self.spectral_channels + (1 if luminance else 0)
        c2, s2 = (math.cos(2.0 * analyser), math.sin(2.0 * analyser)) if c2s2 is None else c2s2
        st_tm, _ = self._tonemap_struct(dict(tm or {"op": "linear"}, table=None))
        spec = FilmPolarSpec(FILM_STATS_LUMINANCE if luminance else 0, sum(1 << FILM_POLAR_MAPS.index(m) for m in names), int(picture_plane), TONEMAP_FORMATS[fmt],
                             float(c2), float(s2), float(sat_gain), 0.0, st_tm)
        rec = (FilmPolar * max(planes, 1))()
        got_maps, got_picture = call(spec, rec, (self.height, self.width, planes, len(names)) if names else None,
                                     (self.height, self.width, 4 if masked else 3) if picture else None)
        out = {name: np.array([getattr(r, name) for r in rec][:planes], dtype=np.uint64 if t is C.c_uint64 else np.float64) for name, t in FILM_POLAR_FIELDS}
        with np.errstate(divide="ignore", invalid="ignore"):
            out["dop_total"] = np.sqrt(out["sum_q"] ** 2 + out["sum_u"] ** 2 + out["sum_v"] ** 2) / out["sum_i"]
            out["aolp_total"] = 0.5 * np.arctan2(out["sum_u"], out["sum_q"])
            out["mean_dolp"] = out["sum_lin"] / out["sum_i"]
            out["mean_dop"] = out["sum_pol"] / out["sum_i"]
        out["maps"] = {m: got_maps[..., k] for k, m in enumerate(names)}
        out["picture"] = got_picture
        return out

    def _film_polar_device(self, what, films, spe, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, stream):
        import torch
        src, dev = self._device_source(what, films, spe, mask)
        st = self._stream_arg(stream, dev)

        def call(spec, rec, maps_shape, picture_shape):
            m = None if maps_shape is None else torch.empty(maps_shape, dtype=torch.float32, device=dev)
            p = None if picture_shape is None else torch.empty(picture_shape, dtype={"f32": torch.float32, "u8": torch.uint8, "u16": torch.int16}[fmt], device=dev)
            _check(load_library().wtgpu_film_polar_source_device(self._h, st, C.byref(src), C.byref(spec), None if mask is None else mask.data_ptr(),
                                                                 C.cast(rec, C.c_void_p), None if m is None else m.data_ptr(), None if p is None else p.data_ptr()))
            return m, p
        return self._film_polar(what, call, luminance, maps, analyser, c2s2, picture, picture_plane, tm, fmt, sat_gain, mask is not None)

    def _film_polar_host(self, what, films, spe, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, threads):
        import numpy as np
        src, m, keep = self._host_source(what, films, spe, mask)

        def call(spec, rec, maps_shape, picture_shape):
            mp = None if maps_shape is None else np.zeros(maps_shape, dtype=np.float32)
            p = None if picture_shape is None else np.zeros(picture_shape, dtype={"f32": np.float32, "u8": np.uint8, "u16": np.uint16}[fmt])
            _check(load_library().wtgpu_film_polar_source_host(self._h, C.byref(src), C.byref(spec), None if m is None else m.ctypes.data, int(threads),
                                                               C.cast(rec, C.c_void_p), None if mp is None else mp.ctypes.data, None if p is None else p.ctypes.data))
            return mp, p
        out = self._film_polar(what, call, luminance, maps, analyser, c2s2, picture, picture_plane, tm, fmt, sat_gain, m is not None)
        del keep
        return out

    def film_polar_device(self, value, weight, light, spe, *, luminance=False, maps=(), analyser=0.0, c2s2=None, mask=None, picture=False, picture_plane=0, tm=None,
                          fmt="f32", sat_gain=1.0, stream=None):
        """The polarisation view of a polarimetric film where it is (wtgpu_film_polar_device): value / weight / light are the torch f64 films on the
        scene's device, mask an H x W f32 tensor there (pixels with mask > 0 count) or None.  One record per channel, plus the Stokes vector of the
        BT.709 luminance of an RGB film with luminance=True.  Returns a dict of numpy arrays indexed by plane: n, n_nonfinite, n_dark, n_over, argmax
        (uint64; the row-major pixel of max_dop, 2^64 - 1 where no pixel is lit), max_dop, sum_i, sum_q, sum_u, sum_v, sum_lin, sum_pol (float64; over
        the lit pixels: finite, I > 0) and, derived here from the sums, dop_total = sqrt(sum_q^2 + sum_u^2 + sum_v^2) / sum_i, aolp_total =
        atan2(sum_u, sum_q) / 2, mean_dolp = sum_lin / sum_i and mean_dop = sum_pol / sum_i (NaN where there is nothing to divide by).
        maps: names of dolp, dop, docp, aolp, chi, analyser -> "maps": {name: torch f32 tensor H x W x planes on the device}, 0 where the mask excludes;
        analyser: the analyser's angle theta in radians (c2s2 = (cos 2 theta, sin 2 theta) overrides it).  picture=True adds "picture": the false-colour
        view of plane picture_plane (hue: the angle of linear polarisation, saturation: dolp x sat_gain, value: the intensity through the operator of
        tm = {op, gamma, db_range}), a torch tensor H x W x 3 (x 4 with a mask) of float32 / uint8 / int16 as tonemap_device's."""
        return self._film_polar_device("film_polar_device", (value, weight, light), spe, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, stream)

    def film_polar_host(self, value, weight, light, spe, *, luminance=False, maps=(), analyser=0.0, c2s2=None, mask=None, picture=False, picture_plane=0, tm=None,
                        fmt="f32", sat_gain=1.0, threads=0):
        """film_polar_device's twin on host threads from numpy films (wtgpu_film_polar_host; threads 0 = all cores): the same dict, every field and every
        map bit for bit the device's, the maps and the picture numpy arrays (the picture of float32 / uint8 / uint16).  No device needed."""
        return self._film_polar_host("film_polar_host", (value, weight, light), spe, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, threads)

    def film_polar_developed_device(self, film, *, luminance=False, maps=(), analyser=0.0, c2s2=None, mask=None, picture=False, picture_plane=0, tm=None, fmt="f32",
                                    sat_gain=1.0, stream=None):
        """film_polar_device of a DEVELOPED polarimetric film where it is (wtgpu_film_polar_source_device): film a torch f32 tensor [H, W, channels, 4]
        on the scene's device (develop_device's result, film_denoise_device's "film": how much polarisation the filter left).  The other arguments
        and the dict are film_polar_device's."""
        return self._film_polar_device("film_polar_developed_device", film, 0, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, stream)

    def film_polar_developed_host(self, film, *, luminance=False, maps=(), analyser=0.0, c2s2=None, mask=None, picture=False, picture_plane=0, tm=None, fmt="f32",
                                  sat_gain=1.0, threads=0):
        """film_polar_developed_device's twin on host threads (wtgpu_film_polar_source_host): film a contiguous numpy float32 array of the scene's planes."""
        return self._film_polar_host("film_polar_developed_host", film, 0, luminance, maps, analyser, c2s2, mask, picture, picture_plane, tm, fmt, sat_gain, threads)

    # ---- denoising a film from its two half-films (wtgpu_film_denoise_*; csrc/wt/film_denoise.h) ----
    @staticmethod
    def _film_denoise_spec(window, patch, k, alpha, eps):
        return FilmDenoiseSpec(int(window), int(patch), 0, 0, float(k), float(alpha), float(eps), 0.0)

    def _film_denoise_guides(self, what, guide, guide_scale, ids, device):
        """guide / guide_scale / ids of film_denoise_device (device: the torch device) or film_denoise_host (None) -> (wtgpu_film_denoise_guides, the
        guide [H, W, G] f32 or None, the ids [H, W] holding u32 bits or None), contiguous and of the scene's size, or a refusal.  What only the entry
        point can judge — the scales' values, the count against 8 — goes there."""
        import numpy as np
        n = self.width * self.height
        if guide is None and guide_scale is not None:
            raise ValueError(f"{what}: guide_scale without a guide")
        G, g, i = 0, None, None
        if guide is not None:
            if device is None:
                g = np.ascontiguousarray(guide, dtype=np.float32)
                ok = g.ndim in (2, 3)
            else:
                import torch
                ok = isinstance(guide, torch.Tensor) and guide.is_cuda and guide.device == device and guide.dtype == torch.float32 and guide.dim() in (2, 3)
                g = guide.contiguous() if ok else None
            if not ok or tuple(g.shape[:2]) != (self.height, self.width):
                raise ValueError(f"{what}: guide: [H, W] or [H, W, G] f32 of the scene's size expected" + ("" if device is None else f", a tensor on {device}"))
            G = 1 if len(g.shape) == 2 else int(g.shape[2])
        if ids is not None:
            if device is None:
                i = np.ascontiguousarray(ids)
                ok = i.dtype in (np.dtype(np.int32), np.dtype(np.uint32)) and i.size == n
            else:
                import torch
                ok = isinstance(ids, torch.Tensor) and ids.is_cuda and ids.device == device and ids.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) \
                    and ids.numel() == n
                i = ids.contiguous() if ok else None
            if not ok:
                raise ValueError(f"{what}: ids: [H, W] int32 or uint32 of the scene's size expected" + ("" if device is None else f", a tensor on {device}"))
        scales = np.zeros(0, np.float32) if guide is None else np.ones(G, np.float32) if guide_scale is None else np.atleast_1d(np.asarray(guide_scale, dtype=np.float32))
        if guide is not None and scales.size == 1 and G > 1:
            scales = np.repeat(scales, G)
        if scales.ndim != 1 or scales.size != G:
            raise ValueError(f"{what}: guide_scale: a scalar or {G} values expected, got {scales.size}")
        spec = FilmDenoiseGuides(G, FILM_DENOISE_SAME_ID if i is not None else 0)
        for j, s in enumerate(scales[:FILM_DENOISE_MAX_GUIDES]):
            spec.scale[j] = float(s)
        return spec, g, i

    def film_denoise_device(self, films_a, spe_a, films_b, spe_b, *, window=7, patch=2, k=0.45, alpha=1.0, eps=1e-10, mask=None, residual=False, stream=None,
                            guide=None, guide_scale=None, ids=None):
        """Denoises the film that two half-films add up to, where they are (wtgpu_film_denoise_device): the dual-buffer non-local-means filter of
        Rousselle, Knaus and Zwicker 2012.  films_a / films_b are (value, weight, light), torch f64 tensors on the scene's device, of two renders over
        disjoint sample ranges (render_to_noise(..., halves=True)), developed with spe_a / spe_b samples per element; mask an H x W f32 tensor there
        (pixels with mask > 0 are filtered and serve as candidates; the others come back as the merged film) or None.  window: the radius r of the
        search window (0 .. 10: (2 r + 1)^2 candidates), patch: the radius f of the patches compared (0 .. 3), k: the filter strength, alpha: how much
        of the noise variance is taken off a squared difference, eps: what keeps the quotient finite where there is no variance.  All planes of a pixel
        are filtered with one set of weights, computed from Stokes component 0 of each channel of the OTHER half.  Returns {"film": torch f32
        [H, W, channels, stokes] on the device, (fa + fb) / 2 of the two filtered halves; "residual": (fa - fb) / 2 the same way with residual=True —
        an estimate of the error that is left — or None}.  Enqueued on `stream` (default: torch's current); nothing crosses to the host.
        Guided (wtgpu_film_denoise_guided_device; with guide, guide_scale and ids all None the call is exactly the unguided one): guide a torch f32
        tensor [H, W] or [H, W, G] there, G <= 8 noise-free feature planes (render.first_hit_guides builds one from Scene.first_hit); guide_scale a
        scalar or G values >= 0 (default 1): the squared difference of plane g counts scale[g] times; a candidate's weight comes from the LARGER of
        the colour distance and the feature distance.  ids: an int32 / uint32 tensor [H, W]; only pixels with the pixel's own id are candidates."""
        import torch
        dev = self._device_films("film_denoise_device", *films_a, mask)
        self._device_films("film_denoise_device", *films_b)
        shape = (self.height, self.width, self.spectral_channels, self.stokes)
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        res = torch.empty(shape, dtype=torch.float32, device=dev) if residual else None
        spec = self._film_denoise_spec(window, patch, k, alpha, eps)
        if guide is not None or guide_scale is not None or ids is not None:
            gspec, g, i = self._film_denoise_guides("film_denoise_device", guide, guide_scale, ids, dev)
            _check(load_library().wtgpu_film_denoise_guided_device(self._h, self._stream_arg(stream, dev), *(t.data_ptr() for t in films_a), int(spe_a),
                                                                   *(t.data_ptr() for t in films_b), int(spe_b), C.byref(spec), C.byref(gspec),
                                                                   None if g is None else g.data_ptr(), None if i is None else i.data_ptr(),
                                                                   None if mask is None else mask.data_ptr(), out.data_ptr(), None if res is None else res.data_ptr()))
            return {"film": out, "residual": res}
        _check(load_library().wtgpu_film_denoise_device(self._h, self._stream_arg(stream, dev), *(t.data_ptr() for t in films_a), int(spe_a),
                                                        *(t.data_ptr() for t in films_b), int(spe_b), C.byref(spec), None if mask is None else mask.data_ptr(),
                                                        out.data_ptr(), None if res is None else res.data_ptr()))
        return {"film": out, "residual": res}

    def film_denoise_host(self, films_a, spe_a, films_b, spe_b, *, window=7, patch=2, k=0.45, alpha=1.0, eps=1e-10, mask=None, residual=False, threads=0,
                          guide=None, guide_scale=None, ids=None):
        """film_denoise_device's twin on host threads from numpy films (wtgpu_film_denoise_host; threads 0 = all cores): the same dict, "film" and
        "residual" numpy arrays, bit for bit the device's.  No device needed.  Naive per pixel and candidate: what the device is held to, not a fast path.
        guide, guide_scale, ids: as film_denoise_device's, numpy arrays (wtgpu_film_denoise_guided_host)."""
        import numpy as np
        sets = [self._host_films("film_denoise_host", *films)[:3] for films in (films_a, films_b)]
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        if m is not None and m.size != self.width * self.height:
            raise ValueError("film_denoise_host: a mask of the scene's size expected")
        shape = (self.height, self.width, self.spectral_channels, self.stokes)
        out = np.zeros(shape, dtype=np.float32)
        res = np.zeros(shape, dtype=np.float32) if residual else None
        spec = self._film_denoise_spec(window, patch, k, alpha, eps)
        if guide is not None or guide_scale is not None or ids is not None:
            gspec, g, i = self._film_denoise_guides("film_denoise_host", guide, guide_scale, ids, None)
            _check(load_library().wtgpu_film_denoise_guided_host(self._h, *(t.ctypes.data for t in sets[0]), int(spe_a), *(t.ctypes.data for t in sets[1]), int(spe_b),
                                                                 C.byref(spec), C.byref(gspec), None if g is None else g.ctypes.data,
                                                                 None if i is None else i.ctypes.data, None if m is None else m.ctypes.data, int(threads),
                                                                 out.ctypes.data, None if res is None else res.ctypes.data))
            return {"film": out, "residual": res}
        _check(load_library().wtgpu_film_denoise_host(self._h, *(t.ctypes.data for t in sets[0]), int(spe_a), *(t.ctypes.data for t in sets[1]), int(spe_b),
                                                      C.byref(spec), None if m is None else m.ctypes.data, int(threads), out.ctypes.data,
                                                      None if res is None else res.ctypes.data))
        return {"film": out, "residual": res}

    def profile_counters(self, n=8):
        """Test hook (wtgpu_test_hooks.h): the first n WTGPU_PROFILE scratch counters, accumulated since upload."""
        out = (C.c_uint64 * n)()
        _check(load_library().wtgpu_test_profile_counters(self._h, out, n))
        return [int(v) for v in out]

    def pass_c_tiers(self):
        """Test hook: what pass C in tiers (WTGPU_PASS_C_TIERS=1; kernels_fsd.hip) counted since the counters were reset — the walks settled by
        the prep / wide / hard kernel, the pass-C walks, the rounds that had a pass-C queue, those whose queue was no multiple of 8 / shorter
        than 8, and the lengths of the first queues (wtgpu_kernels.h: kPassCTierSlot ...)."""
        p = self.profile_counters(224)
        rounds = p[164]
        return {"prep": p[160], "wide": p[161], "hard": p[162], "walks": p[163], "rounds": rounds, "rounds_not_multiple_of_8": p[165],
                "rounds_shorter_than_8": p[166], "queue_lengths": p[168:168 + min(rounds, 56)]}

    def connect_class_items(self, slice=0, max_items=1 << 22):
        """Test hook (wtgpu_test_hooks.h): what the last batch connected by k_connect_class on state slice `slice` left behind — (start of every
        class in the flattened item space, samples per class, key per class), all in the device's class order, and the samples in that order."""
        import numpy as np
        lib = load_library()
        lib.wtgpu_test_connect_class_items.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        n_keys = connect_class_order()[0].size
        table = np.zeros(3 * n_keys + 1, np.uint32)
        items = np.zeros(max_items, np.uint32)
        n = C.c_uint32(0)
        _check(lib.wtgpu_test_connect_class_items(self._h, slice, table.ctypes.data, items.ctypes.data, items.size, C.byref(n)))
        return table[:n_keys + 1].copy(), table[n_keys + 1:2 * n_keys + 1].copy(), table[2 * n_keys + 1:].copy(), items[:n.value].copy()

    def counters(self):
        c = Counters()
        _check(load_library().wtgpu_get_counters(self._h, C.byref(c)))
        return c.as_dict()

    def reset_counters(self):
        _check(load_library().wtgpu_reset_counters(self._h))

    def trace_ab_stats(self):
        """Test hook (WTGPU_TRACE_AB=n at upload: the first n rounds of every batch replay their trace queue through both per-lane trace kernels)."""
        a, b, d, w, r = C.c_double(0), C.c_double(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(load_library().wtgpu_trace_ab_stats(self._h, C.byref(a), C.byref(b), C.byref(d), C.byref(w), C.byref(r)))
        return {"ms_refill": a.value, "ms_sm": b.value, "differing_words": int(d.value), "walks": int(w.value), "rounds": int(r.value)}

    def timings(self):
        t = (C.c_float * 12)()
        _check(load_library().wtgpu_last_render_timings(self._h, C.byref(t)))
        return {"generate_ms": t[0], "trace_ms": t[1], "interact_ms": t[2], "connect_ms": t[3], "rounds": int(t[4]),
                "trace_launches": int(t[5]), "batches": int(t[6]), "trace_heavy_ms": t[7], "interact_b_ms": t[8], "flux_ms": t[9],
                "interact_c_ms": t[10], "rounds_per_batch": float(t[11])}

    def close(self):
        if self._h:
            load_library().wtgpu_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """RCCL communicator of the C-ABI (wtgpu_comm_*): one process per GPU, films summed onto a root rank."""

    def __init__(self, world, rank, device, unique_id):
        h = C.c_void_p()
        self._id = C.create_string_buffer(bytes(unique_id), 128)
        _check(load_library().wtgpu_comm_create(int(world), int(rank), int(device), self._id, C.byref(h)))
        self._h = h

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load_library().wtgpu_comm_unique_id(buf))
        return buf.raw

    def film_reduce(self, value, weight, light, root=0, stream=None):
        sp = C.c_void_p(stream) if stream else None
        _check(load_library().wtgpu_film_reduce(self._h, sp, value.data_ptr(), weight.data_ptr(), light.data_ptr(), value.numel(), weight.numel(), int(root)))

    def close(self):
        if self._h:
            load_library().wtgpu_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
