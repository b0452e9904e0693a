"""ctypes binding of libmobilert_amd.so (include/mobilert_amd.h).

This is the stub a Python front end (or the test-suite) uses in place of the reference's
native bindings; INTEGRATION.md shows the JNI / Qt equivalents.  The library is built
in-tree by ``__graft_entry__.build()`` (``make -C mobileraytracer_amd/csrc``).  There is no
CPU fallback: if the shared object is missing, importing this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MOBILERT_LIB: another build of the library (A/B of compile-time variants, tools/build_ab.sh)
LIB_PATH = os.environ.get("MOBILERT_LIB") or os.path.join(_HERE, "libmobilert_amd.so")

# Symbols the C-ABI exports (include/mobilert_amd.h + mobilert_amd.hpp).
EXPORTED_SYMBOLS = (
    "mrt_last_error", "mrt_build_stamp", "mrt_create", "mrt_destroy", "mrt_render_frame", "mrt_render_frame_device",
    "mrt_unpack_gathered", "mrt_stop_render", "mrt_get_sample", "mrt_get_total_casted_rays",
    "mrt_get_scene_info", "mrt_set_profiling", "mrt_get_frame_stats", "mrt_primary_hits", "mrt_set_tuning",
    "mrt_get_tuning", "mrt_triangle_bvh", "mrt_walk_tree", "mrt_decode_texture", "mrt_kat_slab", "mrt_kat_triangle",
    "mrt_trace_rays", "mrt_sample_tables", "mrt_regular_grid", "mrt_grid_box_test", "mrt_create_from_memory",
    "mrt_preview_arrays", "mrt_wave_log", "mrt_set_camera", "mrt_set_pixel_sampler", "mrt_set_max_point",
    "mrt_android_read_file", "mrt_android_initialize", "mrt_android_render_into_bitmap",
    "mrt_android_render_into_bitmap_cb", "mrt_android_wait_render", "mrt_android_start_render",
    "mrt_android_stop_render", "mrt_android_finish_render", "mrt_android_state", "mrt_android_fps",
    "mrt_android_time_renderer", "mrt_android_sample", "mrt_android_number_of_lights", "mrt_android_resize",
    "mrt_android_vertices", "mrt_android_colors", "mrt_android_camera", "mrt_android_reset",
    "mrt_get_queue_info", "mrt_plan_queues", "mrt_render_views", "mrt_render_views_device",
    "mrt_kat_accumulate", "mrt_cast_rays_device", "mrt_walk_stack", "mrt_plan_spill",
    "mrt_path_key", "mrt_shade_rays_device", "mrt_camera_rays_device",
    "mrt_cast_hits_device", "mrt_cast_multi_hits_device", "mrt_scene_triangles", "mrt_scene_planes", "mrt_scene_spheres", "mrt_scene_materials",
    "mrt_scene_lights", "mrt_nearest_points_device", "mrt_point_distance", "mrt_kat_point_distance",
    "mrt_neighbours_device", "mrt_overlap_boxes_device", "mrt_box_overlap", "mrt_kat_box_overlap",
    "mrt_sweep_spheres_device", "mrt_sphere_sweep", "mrt_kat_sphere_sweep",
    "mrt_overlap_triangles_device", "mrt_triangle_overlap", "mrt_kat_triangle_overlap",
    "RayTrace", "stopRender",
)


class MrtConfig(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("threads", ctypes.c_int32),
        ("shader", ctypes.c_int32), ("sceneIndex", ctypes.c_int32), ("samplesPixel", ctypes.c_int32),
        ("samplesLight", ctypes.c_int32), ("repeats", ctypes.c_int32), ("accelerator", ctypes.c_int32),
        ("printStdOut", ctypes.c_int32),
        ("objFilePath", ctypes.c_char_p), ("mtlFilePath", ctypes.c_char_p), ("camFilePath", ctypes.c_char_p),
        ("maxDepth", ctypes.c_int32), ("rankIndex", ctypes.c_int32), ("rankCount", ctypes.c_int32),
        ("device", ctypes.c_int32), ("cull", ctypes.c_int32), ("maxPathsPerPass", ctypes.c_int32),
        ("progressive", ctypes.c_int32), ("devices", ctypes.POINTER(ctypes.c_int32)), ("deviceCount", ctypes.c_int32),
    ]


class MrtAndroidConfig(ctypes.Structure):  # include/mobilert_android.h
    _fields_ = [(n, ctypes.c_int32) for n in (
        "scene", "shader", "accelerator", "width", "height", "samplesPixel", "samplesLight")] + [
        ("objFilePath", ctypes.c_char_p)]


class MrtBlob(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("bytes", ctypes.c_char_p), ("size", ctypes.c_int64)]


class MrtView(ctypes.Structure):  # mrt_view: the arguments of mrt_set_camera
    _fields_ = [("kind", ctypes.c_int32), ("position", ctypes.c_float * 3), ("lookAt", ctypes.c_float * 3),
                ("up", ctypes.c_float * 3), ("a", ctypes.c_float), ("b", ctypes.c_float)]


class MrtRayBatch(ctypes.Structure):  # mrt_ray_batch: a device-resident batch of rays (mrt_cast_rays_device)
    _fields_ = [("orig", ctypes.c_void_p), ("dir", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("origStride", ctypes.c_int64), ("dirStride", ctypes.c_int64), ("n", ctypes.c_int64)]


# mrt_hit_records: the fields in the header's order, (name, dtype, floats or ints per ray)
HIT_FIELDS = (("kind", "int32", 1), ("index", "int32", 1), ("t", "float32", 1), ("bary", "float32", 2),
              ("point", "float32", 3), ("normal", "float32", 3), ("texCoord", "float32", 2), ("material", "int32", 1),
              ("kd", "float32", 3), ("ks", "float32", 3), ("kt", "float32", 3), ("le", "float32", 3), ("ior", "float32", 1))


class MrtHitRecords(ctypes.Structure):  # mrt_hit_records: device arrays of a surface-record query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in HIT_FIELDS]


MULTI_HITS_MAX = 16  # MRT_MULTI_HITS_MAX
# mrt_multi_hits: the fields in the header's order, (name, dtype, entries per ray: 0 = one per ray, else
# floats or ints per list entry)
MULTI_HIT_FIELDS = (("count", "int32", 0), ("kind", "int32", 1), ("index", "int32", 1), ("t", "float32", 1),
                    ("bary", "float32", 2))


class MrtMultiHits(ctypes.Structure):  # mrt_multi_hits: device arrays of a multi-hit query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in MULTI_HIT_FIELDS]


class MrtPointBatch(ctypes.Structure):  # mrt_point_batch: a device-resident batch of points (mrt_nearest_points_device)
    _fields_ = [("point", ctypes.c_void_p), ("dist", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("stride", ctypes.c_int64), ("n", ctypes.c_int64)]


# mrt_nearest: the fields in the header's order, (name, dtype, floats or ints per point)
NEAREST_FIELDS = (("kind", "int32", 1), ("index", "int32", 1), ("dist2", "float32", 1), ("point", "float32", 3),
                  ("bary", "float32", 2), ("tests", "int32", 1))


class MrtNearest(ctypes.Structure):  # mrt_nearest: device arrays of a nearest-point query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in NEAREST_FIELDS]


NEIGHBOURS_MAX = 16  # MRT_NEIGHBOURS_MAX
# mrt_neighbours: the fields in the header's order, (name, dtype, entries per point: 0 = one per point, else
# floats or ints per list entry)
NEIGHBOUR_FIELDS = (("count", "int32", 0), ("kind", "int32", 1), ("index", "int32", 1), ("dist2", "float32", 1),
                    ("point", "float32", 3), ("bary", "float32", 2), ("tests", "int32", 0))


class MrtNeighbours(ctypes.Structure):  # mrt_neighbours: device arrays of a neighbour query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in NEIGHBOUR_FIELDS]


OVERLAP_MAX = 16  # MRT_OVERLAP_MAX
# mrt_overlaps: the fields in the header's order, (name, dtype, entries per box: 0 = one per box, else ints
# per list entry)
OVERLAP_FIELDS = (("any", "int32", 0), ("count", "int32", 0), ("kind", "int32", 1), ("index", "int32", 1),
                  ("tests", "int32", 0))


class MrtBoxBatch(ctypes.Structure):  # mrt_box_batch: a device-resident batch of boxes (mrt_overlap_boxes_device)
    _fields_ = [("mn", ctypes.c_void_p), ("mx", ctypes.c_void_p), ("mnStride", ctypes.c_int64),
                ("mxStride", ctypes.c_int64), ("n", ctypes.c_int64)]


class MrtTriangleBatch(ctypes.Structure):  # mrt_triangle_batch: device-resident query triangles (mrt_overlap_triangles_device)
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("c", ctypes.c_void_p), ("aStride", ctypes.c_int64),
                ("bStride", ctypes.c_int64), ("cStride", ctypes.c_int64), ("n", ctypes.c_int64)]


class MrtOverlaps(ctypes.Structure):  # mrt_overlaps: device arrays of an overlap query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in OVERLAP_FIELDS]


# mrt_sweeps: the fields in the header's order, (name, dtype, floats or ints per ray)
SWEEP_FIELDS = (("hit", "int32", 1), ("kind", "int32", 1), ("index", "int32", 1), ("t", "float32", 1),
                ("centre", "float32", 3), ("point", "float32", 3), ("bary", "float32", 2), ("tests", "int32", 1))


class MrtSweeps(ctypes.Structure):  # mrt_sweeps: device arrays of a sweep query, NULL = not wanted
    _fields_ = [(name, ctypes.c_void_p) for name, _, _ in SWEEP_FIELDS]


class MrtShadeBatch(ctypes.Structure):  # mrt_shade_batch: rays and their path keys (mrt_shade_rays_device)
    _fields_ = [("rays", MrtRayBatch), ("key", ctypes.c_void_p)]


class MrtSceneInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "triangles", "lights", "planes", "spheres", "materials", "triangleNodes", "triangleBvhDepth",
        "pixelSlots", "pixelSlotsMax", "deviceBytes", "shadowStreamConcurrent", "shadowStreamsTried", "deviceCount")]


class MrtFrameStats(ctypes.Structure):
    _fields_ = [
        ("rays", ctypes.c_uint64), ("shadowRays", ctypes.c_uint64), ("primaryRays", ctypes.c_uint64),
        ("nodeRecords", ctypes.c_uint64), ("triTests", ctypes.c_uint64),
        ("shadowNodeRecords", ctypes.c_uint64), ("shadowTriTests", ctypes.c_uint64),
        ("traceMs", ctypes.c_double), ("shadowMs", ctypes.c_double), ("frameMs", ctypes.c_double),
        ("traceLaunches", ctypes.c_int64), ("shadowLaunches", ctypes.c_int64),
        ("shadeMs", ctypes.c_double),
        ("levelRays", ctypes.c_uint64 * 16), ("levelShadowRays", ctypes.c_uint64 * 16),
        ("levelTraceMs", ctypes.c_double * 16), ("levelShadowMs", ctypes.c_double * 16),
        ("maxNodeRecordsPerRay", ctypes.c_uint64),
        ("walkedRays", ctypes.c_uint64), ("shadedVertices", ctypes.c_uint64), ("shadeLaunches", ctypes.c_int64),
        ("leafRecords", ctypes.c_uint64), ("shadowLeafRecords", ctypes.c_uint64),
        ("levelNodeRecords", ctypes.c_uint64 * 16), ("levelTriTests", ctypes.c_uint64 * 16),
        ("levelLeafRecords", ctypes.c_uint64 * 16),
        ("fusedMs", ctypes.c_double), ("fusedLaunches", ctypes.c_int64),
        ("levelShadedVertices", ctypes.c_uint64 * 16),
        ("shadowOccluded", ctypes.c_uint64),
        ("walkPhases", ctypes.c_uint64 * 16),
        ("packetWaveRecords", ctypes.c_uint64 * 3),
    ]


QUEUE_LEVELS = 16  # MRT_QUEUE_LEVELS


class MrtQueueInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "chunkSlots", "passes", "queueBytes", "budgetBytes", "replans", "replansLastFrame", "worstCase")] + [
        (n, ctypes.c_int64 * QUEUE_LEVELS) for n in ("rayCap", "shadowCap", "requestedRays", "requestedShadows")]


class MrtQueuePlanRequest(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "levels", "branching", "samplesPixel", "samplesLight", "textured", "segments", "growthPct", "slack",
        "worstCase", "hasDemand")] + [
        ("pixelSlots", ctypes.c_int64), ("pathBudget", ctypes.c_int64), ("byteBudget", ctypes.c_int64),
        ("overflowMask", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("demandChunkSlots", ctypes.c_int64), ("demandPaths", ctypes.c_int64),
        ("segDemand", ctypes.c_int64 * QUEUE_LEVELS), ("shadowSegDemand", ctypes.c_int64 * QUEUE_LEVELS),
        ("prevChunkSlots", ctypes.c_int64),
        ("prevSegCap", ctypes.c_int64 * QUEUE_LEVELS), ("prevShadowSegCap", ctypes.c_int64 * QUEUE_LEVELS)]


class MrtQueuePlan(ctypes.Structure):
    _fields_ = [("chunkSlots", ctypes.c_int64), ("segCap", ctypes.c_int64 * QUEUE_LEVELS),
                ("shadowSegCap", ctypes.c_int64 * QUEUE_LEVELS), ("bytes", ctypes.c_int64),
                ("worstCase", ctypes.c_int64)]


def _preload_torch_hip_runtime():
    """One HIP runtime per process: if PyTorch-ROCm is installed, load its libamdhip64 first
    (by full path, without importing torch) so this library and torch share it whichever is
    imported first.  Both carry the SONAME libamdhip64.so.7."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(rt):
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the MI355X path has no CPU fallback)")
    _preload_torch_hip_runtime()
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    vp = ctypes.c_void_p
    sig = {
        "mrt_last_error": (ctypes.c_char_p, []),
        "mrt_build_stamp": (ctypes.c_char_p, []),
        "mrt_create": (ctypes.c_int, [P(MrtConfig), P(vp)]),
        "mrt_destroy": (None, [vp]),
        "mrt_render_frame": (ctypes.c_int, [vp, vp]),
        "mrt_render_frame_device": (ctypes.c_int, [vp, vp, vp, vp]),
        "mrt_render_views": (ctypes.c_int, [vp, P(MrtView), ctypes.c_int32, vp]),
        "mrt_render_views_device": (ctypes.c_int, [vp, P(MrtView), ctypes.c_int32, vp, vp, vp]),
        "mrt_unpack_gathered": (ctypes.c_int, [vp, vp, vp, vp]),
        "mrt_stop_render": (ctypes.c_int, [vp]),
        "mrt_get_sample": (ctypes.c_int32, [vp]),
        "mrt_get_total_casted_rays": (ctypes.c_uint64, [vp]),
        "mrt_get_scene_info": (ctypes.c_int, [vp, P(MrtSceneInfo)]),
        "mrt_set_profiling": (ctypes.c_int, [vp, ctypes.c_int32]),
        "mrt_get_frame_stats": (ctypes.c_int, [vp, P(MrtFrameStats)]),
        "mrt_get_queue_info": (ctypes.c_int, [vp, vp, ctypes.c_size_t]),
        "mrt_plan_queues": (ctypes.c_int, [P(MrtQueuePlanRequest), P(MrtQueuePlan)]),
        "mrt_wave_log": (ctypes.c_int64, [vp, vp]),
        "mrt_primary_hits": (ctypes.c_int, [vp, vp, vp, vp]),
        "mrt_set_tuning": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_int32]),
        "mrt_get_tuning": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]),
        "mrt_triangle_bvh": (ctypes.c_int64, [vp, vp, vp, vp, vp]),
        "mrt_walk_tree": (ctypes.c_int64, [vp, vp, vp, vp]),
        "mrt_walk_stack": (ctypes.c_int, [vp, vp]),
        "mrt_plan_spill": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64]),
        "mrt_decode_texture": (ctypes.c_int64, [ctypes.c_char_p, vp, vp]),
        "mrt_regular_grid": (ctypes.c_int64, [vp, ctypes.c_int32, vp, vp, vp]),
        "mrt_grid_box_test": (ctypes.c_int, [ctypes.c_int32, vp, vp]),
        "mrt_create_from_memory": (ctypes.c_int, [P(MrtConfig), ctypes.c_char_p, ctypes.c_int64, ctypes.c_char_p,
                                                  ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64, vp, ctypes.c_int32,
                                                  P(vp)]),
        "mrt_preview_arrays": (ctypes.c_int64, [vp, vp, vp, vp]),
        "mrt_set_camera": (ctypes.c_int, [vp, ctypes.c_int32, vp, vp, vp, ctypes.c_float, ctypes.c_float]),
        "mrt_set_pixel_sampler": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_float]),
        "mrt_set_max_point": (ctypes.c_int, [vp, vp]),
        "mrt_android_read_file": (None, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int64]),
        "mrt_android_initialize": (ctypes.c_int32, [P(MrtAndroidConfig)]),
        "mrt_android_render_into_bitmap": (None, [vp, ctypes.c_int32]),
        "mrt_android_render_into_bitmap_cb": (None, [vp, ctypes.c_int32, vp, vp]),
        "mrt_android_wait_render": (None, []),
        "mrt_android_start_render": (None, [ctypes.c_int32]),
        "mrt_android_stop_render": (None, [ctypes.c_int32]),
        "mrt_android_finish_render": (None, []),
        "mrt_android_state": (ctypes.c_int32, []),
        "mrt_android_fps": (ctypes.c_float, []),
        "mrt_android_time_renderer": (ctypes.c_int64, []),
        "mrt_android_sample": (ctypes.c_int32, []),
        "mrt_android_number_of_lights": (ctypes.c_int32, []),
        "mrt_android_resize": (ctypes.c_int32, [ctypes.c_int32]),
        "mrt_android_vertices": (ctypes.c_int64, [vp]),
        "mrt_android_colors": (ctypes.c_int64, [vp]),
        "mrt_android_camera": (ctypes.c_int64, [vp]),
        "mrt_android_reset": (None, []),
        "mrt_sample_tables": (ctypes.c_int, [vp, vp, vp]),
        "mrt_kat_slab": (ctypes.c_int, [vp, vp, vp, ctypes.c_int32, vp]),
        "mrt_kat_triangle": (ctypes.c_int, [vp, vp, vp, ctypes.c_int32, vp, vp]),
        "mrt_kat_accumulate": (ctypes.c_int, [vp] + [ctypes.c_int32] * 6 + [vp, P(ctypes.c_int32)]),
        "mrt_trace_rays": (ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp]),
        "mrt_cast_rays_device": (ctypes.c_int, [vp, P(MrtRayBatch), ctypes.c_int32, vp, vp, vp, vp]),
        "mrt_cast_hits_device": (ctypes.c_int, [vp, P(MrtRayBatch), P(MrtHitRecords), ctypes.c_size_t, vp]),
        "mrt_cast_multi_hits_device": (ctypes.c_int, [vp, P(MrtRayBatch), ctypes.c_int32, P(MrtMultiHits),
                                                      ctypes.c_size_t, vp]),
        "mrt_nearest_points_device": (ctypes.c_int, [vp, P(MrtPointBatch), P(MrtNearest), ctypes.c_size_t, vp]),
        "mrt_neighbours_device": (ctypes.c_int, [vp, P(MrtPointBatch), ctypes.c_int32, P(MrtNeighbours),
                                                 ctypes.c_size_t, vp]),
        "mrt_overlap_boxes_device": (ctypes.c_int, [vp, P(MrtBoxBatch), ctypes.c_int32, P(MrtOverlaps),
                                                    ctypes.c_size_t, vp]),
        "mrt_box_overlap": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int64, vp]),
        "mrt_kat_box_overlap": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int32, vp]),
        "mrt_overlap_triangles_device": (ctypes.c_int, [vp, P(MrtTriangleBatch), ctypes.c_int32, P(MrtOverlaps),
                                                        ctypes.c_size_t, vp]),
        "mrt_triangle_overlap": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int64, vp]),
        "mrt_kat_triangle_overlap": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int32, vp]),
        "mrt_sweep_spheres_device": (ctypes.c_int, [vp, P(MrtRayBatch), vp, P(MrtSweeps), ctypes.c_size_t, vp]),
        "mrt_sphere_sweep": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int64, vp, vp, vp, vp, vp]),
        "mrt_kat_sphere_sweep": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp]),
        "mrt_point_distance": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int64, vp, vp, vp]),
        "mrt_kat_point_distance": (ctypes.c_int, [ctypes.c_int32, vp, vp, ctypes.c_int32, vp, vp, vp]),
        "mrt_scene_triangles": (ctypes.c_int64, [vp, vp, vp, vp, vp]),
        "mrt_scene_planes": (ctypes.c_int64, [vp, vp, vp]),
        "mrt_scene_spheres": (ctypes.c_int64, [vp, vp, vp]),
        "mrt_scene_materials": (ctypes.c_int64, [vp, vp, vp]),
        "mrt_scene_lights": (ctypes.c_int64, [vp, vp, vp, vp]),
        "mrt_path_key": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32]),
        "mrt_shade_rays_device": (ctypes.c_int, [vp, P(MrtShadeBatch), vp, ctypes.c_int64, P(ctypes.c_uint64), vp]),
        "mrt_camera_rays_device": (ctypes.c_int64, [vp, P(MrtView), ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("MOBILERT_LIB") and not hasattr(lib, name):
            continue  # an older A/B build without a newer test entry point
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = load_library()
    return _LIB


def source_stamp():
    """The digest the Makefile embeds (mrt_build_stamp) for the csrc sources in this tree."""
    import hashlib
    d = os.path.join(_HERE, "csrc")
    srcs = ["mrt_scene.cpp", "mrt_grid.cpp", "mrt_texture.cpp", "mrt_android.cpp", "mrt_queue_plan.cpp", "mrt_kernels.hip",
            "mrt_renderer.hip",
            "mrt_common.hpp", "mrt_device.hpp", "mrt_kernels.hpp", "mrt_trace_ww.hpp", "mrt_trace_packet.hpp",
            "mrt_multi_hit.hpp", "mrt_nearest.hpp", "mrt_neighbours.hpp", "mrt_overlap.hpp", "mrt_sweep.hpp", "mrt_triangle_overlap.hpp", "mrt_scene.hpp", "mrt_queue_plan.hpp", "../../include/mobilert_amd.h", "../../include/mobilert_amd.hpp",
            "../../include/mobilert_android.h"]
    h = hashlib.sha256()
    for f in srcs:
        with open(os.path.join(d, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def build_is_current(library=None):
    """True when the loaded library was built from this tree's sources (no extra flags)."""
    return (library or lib()).mrt_build_stamp().decode() == source_stamp()


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().mrt_last_error().decode(errors="replace"))
