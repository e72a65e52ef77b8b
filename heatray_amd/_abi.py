"""ctypes view of the headers under include/: their constants, their structs and, in PROTOTYPES, the prototype of every function they
declare.  Pure declarations; heatray_amd._ffi binds them to a library and holds the calls.  tests/test_prototypes.py reads the
headers and holds this file to them."""
import ctypes as C

import numpy as np

HR_OK = 0
HR_MAX_LIGHTS = 5
HR_NUM_RANDOM_SEQUENCES = 16

HR_CTX_COLLECT_STATS = 1
HR_CTX_TIME_KERNELS = 2
HR_KERNEL_NAMES = ("raygen", "trace", "shade", "resolve")

HR_TRIANGLES, HR_TRIANGLE_STRIP = 0, 1
HR_TEX_U8, HR_TEX_F32 = 0, 1
HR_WRAP_REPEAT, HR_WRAP_CLAMP_TO_EDGE = 0, 1
HR_FILTER_NEAREST, HR_FILTER_LINEAR = 0, 1
HR_MAT_PBR, HR_MAT_GLASS = 0, 1

HR_MF_HAS_BASE_COLOR_TEXTURE = 1 << 0
HR_MF_HAS_METALLIC_ROUGHNESS_TEXTURE = 1 << 1
HR_MF_HAS_EMISSIVE_TEXTURE = 1 << 2
HR_MF_HAS_NORMALMAP = 1 << 3
HR_MF_HAS_CLEARCOAT_TEXTURE = 1 << 4
HR_MF_HAS_CLEARCOAT_ROUGHNESS_TEXTURE = 1 << 5
HR_MF_HAS_CLEARCOAT_NORMALMAP = 1 << 6
HR_MF_DOUBLE_SIDED = 1 << 7
HR_MF_ALPHA_MASK = 1 << 8
HR_MF_VERTEX_COLORS = 1 << 9

HR_SAMPLE_RANDOM, HR_SAMPLE_HALTON, HR_SAMPLE_HAMMERSLEY, HR_SAMPLE_BLUE_NOISE, HR_SAMPLE_SOBOL = range(5)
HR_BOKEH_CIRCULAR, HR_BOKEH_PENTAGON, HR_BOKEH_HEXAGON, HR_BOKEH_OCTAGON = range(4)

HR_ESTIMATOR_REFERENCE, HR_ESTIMATOR_ENV_MIS, HR_ESTIMATOR_ALL_LIGHTS = 0, 1, 2
HR_TEXTURE_LOD_BASE, HR_TEXTURE_LOD_CONE = 0, 1
(HR_VIS_NONE, HR_VIS_GEOMETRIC_NORMALS, HR_VIS_UVS, HR_VIS_TANGENTS, HR_VIS_BITANGENTS, HR_VIS_NORMALMAP,
 HR_VIS_FINAL_NORMALS, HR_VIS_BASE_COLOR, HR_VIS_ROUGHNESS, HR_VIS_METALLIC, HR_VIS_EMISSIVE, HR_VIS_CLEARCOAT,
 HR_VIS_CLEARCOAT_ROUGHNESS, HR_VIS_CLEARCOAT_NORMALMAP, HR_VIS_SHADER) = range(15)

P = C.POINTER
f32p = P(C.c_float)
u32p = P(C.c_uint32)
i32p = P(C.c_int32)
u8p = P(C.c_uint8)
u64p = P(C.c_uint64)


class Struct(C.Structure):
    """A struct of the headers, field by field; `_cname_` is its C type."""

    def as_dict(self):
        """The fields in order, as Python ints and floats; `reserved` is left out and a nested struct is its own dict."""
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        return {k: v.as_dict() if isinstance(v, Struct) else v for k, v in d.items()}


# -- include/hrcore.h
HR_ABI_VERSION = 6  # checked against the loaded library before the first call (Engine.__init__)


class CtxDesc(Struct):
    _cname_ = "hr_ctx_desc"
    _fields_ = [("device_id", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("tile_size", C.c_int32),
                ("stream", C.c_void_p), ("flags", C.c_uint32), ("memory_budget", C.c_uint64)]


class MeshDesc(Struct):
    _cname_ = "hr_mesh_desc"
    _fields_ = [("positions", f32p), ("normals", f32p), ("uvs", f32p), ("tangents", f32p), ("bitangents", f32p),
                ("colors", f32p), ("position_stride", C.c_int32), ("normal_stride", C.c_int32),
                ("uv_stride", C.c_int32), ("tangent_stride", C.c_int32), ("bitangent_stride", C.c_int32),
                ("color_stride", C.c_int32), ("n_vertices", C.c_int32), ("indices", u32p), ("n_indices", C.c_int32),
                ("mode", C.c_int32), ("world_from_entity", C.c_float * 16), ("front_face_cw", C.c_int32),
                ("is_occluder", C.c_int32), ("material_id", C.c_int32)]


class SceneInfo(Struct):
    _cname_ = "hr_scene_info"
    _fields_ = [("n_triangles", C.c_uint64), ("n_nodes", C.c_uint64), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("ray_epsilon", C.c_float), ("build_ms", C.c_float),
                ("bvh_levels", C.c_uint32), ("refitted", C.c_uint32),
                ("box_area_ratio", C.c_float), ("builder", C.c_uint32), ("cost_radix", C.c_float), ("cost_ploc", C.c_float)]


class TextureDesc(Struct):
    _cname_ = "hr_texture_desc"
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("dtype", C.c_int32),
                ("wrap_s", C.c_int32), ("wrap_t", C.c_int32), ("filter", C.c_int32)]


class Material(Struct):
    _cname_ = "hr_material"
    _fields_ = [("type", C.c_int32), ("flags", C.c_uint32), ("base_color_texture", C.c_int32),
                ("metallic_roughness_texture", C.c_int32), ("emissive_texture", C.c_int32), ("normalmap", C.c_int32),
                ("clear_coat_texture", C.c_int32), ("clear_coat_roughness_texture", C.c_int32),
                ("clear_coat_normalmap", C.c_int32), ("multiscatter_lut", C.c_int32), ("base_color", C.c_float * 3),
                ("emissive_color", C.c_float * 3), ("metallic", C.c_float), ("roughness", C.c_float),
                ("specular_f0", C.c_float), ("roughness_alpha", C.c_float), ("clear_coat", C.c_float),
                ("clear_coat_roughness", C.c_float), ("clear_coat_roughness_alpha", C.c_float), ("ior", C.c_float),
                ("density", C.c_float)]


V3x5 = (C.c_float * 3) * HR_MAX_LIGHTS
V2x5 = (C.c_float * 2) * HR_MAX_LIGHTS


class Lights(Struct):
    _cname_ = "hr_lights"
    _fields_ = [("n_directional", C.c_int32), ("directional_directions", V3x5), ("directional_colors", V3x5),
                ("n_point", C.c_int32), ("point_positions", V3x5), ("point_colors", V3x5), ("n_spot", C.c_int32),
                ("spot_positions", V3x5), ("spot_directions", V3x5), ("spot_colors", V3x5), ("spot_angles", V2x5),
                ("env_enabled", C.c_int32), ("env_texture", C.c_int32), ("env_exposure", C.c_float),
                ("env_theta_rotation", C.c_float)]


class PassParams(Struct):
    _cname_ = "hr_pass_params"
    _fields_ = [("sample_index", C.c_int32), ("max_ray_depth", C.c_int32), ("max_channel_value", C.c_float),
                ("fov_tan", C.c_float), ("aspect_ratio", C.c_float), ("focus_distance", C.c_float),
                ("aperture_radius", C.c_float), ("view_matrix", C.c_float * 16), ("interactive_mode", C.c_int32),
                ("block_size", C.c_int32 * 2), ("current_block_pixel", C.c_int32 * 2), ("max_sample_index", C.c_float),
                ("enable_visualizer", C.c_int32), ("visualizer_mode", C.c_int32),
                ("enable_accumulator_visualizer", C.c_int32), ("show_nans", C.c_int32), ("show_inf", C.c_int32),
                ("estimator", C.c_int32), ("texture_lod", C.c_int32)]


class PassStats(Struct):
    _cname_ = "hr_pass_stats"
    _fields_ = [("ms", C.c_float), ("paths", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_any", C.c_uint64),
                ("shaded_hits", C.c_uint64), ("accumulates", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("node_visits_any", C.c_uint64), ("tri_tests_any", C.c_uint64)]


class StepRecord(Struct):
    _cname_ = "hr_step_record"
    _fields_ = [("start_ms", C.c_double), ("trace_ms", C.c_float), ("passes_in_flight", C.c_int32), ("passes_injected", C.c_int32), ("group", C.c_int32)]


class KernelTimes(Struct):
    _cname_ = "hr_kernel_times"
    _fields_ = [("ms", C.c_float * 4), ("launches", C.c_uint32 * 4), ("trace_clock_ms", C.c_float), ("trace_clock_launches", C.c_uint32),
                ("camera_packets", C.c_uint32), ("packet_union", C.c_float)]


class DisplayParams(Struct):
    """HeatrayRenderer.h:104-117 PostProcessingParams as DisplayProgram::bind uploads them."""
    _cname_ = "hr_display_params"
    _fields_ = [("tonemapping_enabled", C.c_int32), ("camera_exposure", C.c_float), ("brightness", C.c_float),
                ("contrast", C.c_float), ("hue", C.c_float), ("saturation", C.c_float), ("vibrance", C.c_float),
                ("red", C.c_float), ("green", C.c_float), ("blue", C.c_float), ("vignette_intensity", C.c_float),
                ("vignette_falloff", C.c_float)]


HR_DISPLAY_RGBA8, HR_DISPLAY_RGBA32F, HR_DISPLAY_HDR_RGBA32F = 0, 1, 2
HR_DISPLAY_PROGRESSIVE = 0x100


class Hit(Struct):
    _cname_ = "hr_hit"
    _fields_ = [("prim", C.c_int32), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float)]


HIT_DTYPE = np.dtype([("prim", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])

# -- include/hrcore_group.h (context groups; a library without them still loads, create_group then fails)
HR_GROUP_API_VERSION = 1
HR_GROUP_MAX_MEMBERS = 16


class GroupInfo(Struct):
    _cname_ = "hr_group_info"
    _fields_ = [("n_members", C.c_int32), ("device_ids", C.c_int32 * HR_GROUP_MAX_MEMBERS), ("owned_pixels", C.c_uint64 * HR_GROUP_MAX_MEMBERS)]


# -- include/hrcore_aov.h (AOVs).  This header's functions and those of every header below are optional (FEATURES): a library without them
# (the CPU oracle) still makes an Engine, and their calls raise EngineError
HR_AOV_API_VERSION = 1
HR_AOV_SURFACE, HR_AOV_MOMENTS = 1, 2
HR_AOV_PLANE_ALBEDO, HR_AOV_PLANE_NORMAL_DEPTH, HR_AOV_PLANE_MOMENTS = 0, 1, 2
AOV_PLANE_NAMES = ("albedo", "normal_depth", "moments")

# -- include/hrcore_denoise.h (the denoiser over the AOV planes)
HR_DENOISE_API_VERSION = 1
HR_DENOISE_MAX_ITERATIONS, HR_DENOISE_MAX_NORMAL_POWER = 8, 16
HR_DENOISE_KERNEL_AUTO, HR_DENOISE_KERNEL_PLAIN, HR_DENOISE_KERNEL_TILED = 0, 1, 2


class DenoiseParams(Struct):
    _cname_ = "hr_denoise_params"
    _fields_ = [("iterations", C.c_int32), ("normal_power", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("kernel", C.c_int32), ("reserved", C.c_uint32 * 3)]


# -- include/hrcore_denoise_spatial.h (the denoiser with a spatial variance estimate for pixels with few samples)
HR_DENOISE_SPATIAL_API_VERSION = 1
HR_DENOISE_SPATIAL_BELOW_LOWEST, HR_DENOISE_SPATIAL_BELOW_HIGHEST = 2, 64
HR_DENOISE_SPATIAL_MIN_TAPS_LOWEST, HR_DENOISE_SPATIAL_MIN_TAPS_HIGHEST = 2, 49


class DenoiseSpatialParams(Struct):
    _cname_ = "hr_denoise_spatial_params"
    _fields_ = [("below", C.c_int32), ("min_taps", C.c_int32), ("reserved", C.c_uint32 * 6)]


class DenoiseSpatialResult(Struct):
    _cname_ = "hr_denoise_spatial_result"
    _fields_ = [("spatial_pixels", C.c_uint64), ("estimated_pixels", C.c_uint64), ("starved_pixels", C.c_uint64)]


# -- include/hrcore_adaptive.h (the sample mask and the error estimate that builds it)
HR_ADAPTIVE_API_VERSION = 1
HR_ADAPTIVE_MIN_SAMPLES_LOWEST, HR_ADAPTIVE_MIN_SAMPLES_HIGHEST, HR_ADAPTIVE_MAX_RADIUS = 2, 65536, 4


class AdaptiveParams(Struct):
    _cname_ = "hr_adaptive_params"
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_int32), ("radius", C.c_int32), ("reserved", C.c_uint32 * 4)]


class AdaptiveResult(Struct):
    _cname_ = "hr_adaptive_result"
    _fields_ = [("unconverged_pixels", C.c_uint64), ("active_pixels", C.c_uint64), ("max_error", C.c_float), ("passes", C.c_uint32)]


# -- include/hrcore_history.h (history reprojection across a camera change)
HR_HISTORY_API_VERSION = 1
HR_HISTORY_MAX_HISTORY_LOWEST, HR_HISTORY_MAX_HISTORY_HIGHEST = 1, 65536


class HistoryParams(Struct):
    _cname_ = "hr_history_params"
    _fields_ = [("max_history", C.c_int32), ("normal_cos", C.c_float), ("plane_tol", C.c_float), ("min_weight", C.c_float), ("reserved", C.c_uint32 * 4)]


class HistoryResult(Struct):
    _cname_ = "hr_history_result"
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("history_passes", C.c_uint32),
                ("passes", C.c_uint32)]


# -- include/hrcore_reproject.h (the progressive history merge and the preview of unsampled pixels)
HR_REPROJECT_API_VERSION = 1


class ReprojectResult(Struct):
    _cname_ = "hr_reproject_result"
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("pending_pixels", C.c_uint64),
                ("examined_pixels", C.c_uint64), ("history_passes", C.c_uint32), ("passes", C.c_uint32)]


class ReprojectPreviewResult(Struct):
    _cname_ = "hr_reproject_preview_result"
    _fields_ = [("own_pixels", C.c_uint64), ("previewed_pixels", C.c_uint64), ("empty_pixels", C.c_uint64)]


# -- include/hrcore_tree.h (what the last tree build did to the radix tree's bottom subtrees; since 2: the committed tree read back)
HR_TREE_API_VERSION = 2
HR_TREE_NODE4, HR_TREE_NODE32, HR_TREE_LEAF_KEYS, HR_TREE_TRIS, HR_TREE_NODE_BOX, HR_TREE_SLOT_OF_PRIM = range(6)
HR_TREE_ARRAYS = 6


class TreeInfo(Struct):
    _cname_ = "hr_tree_info"
    _fields_ = [("cost_before", C.c_float), ("cost_after", C.c_float), ("subtrees_found", C.c_uint32), ("subtrees_replaced", C.c_uint32),
                ("max_triangles", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class TreeLayout(Struct):
    _cname_ = "hr_tree_layout"
    _fields_ = [("n_nodes", C.c_uint64), ("n_triangles", C.c_uint64), ("tri_slots", C.c_uint64), ("root_leaf_count", C.c_uint32), ("levels", C.c_uint32),
                ("level_start", C.c_uint32 * 65), ("grid_cell_exp", C.c_uint32 * 3), ("pad", C.c_float), ("hit_pad", C.c_float), ("ray_epsilon", C.c_float),
                ("grid_lo", C.c_float * 3), ("grid_cell", C.c_float * 3), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("reserved", C.c_uint32),
                ("bytes", C.c_uint64 * HR_TREE_ARRAYS)]


# -- include/hrcore_exposure.h (auto-exposure: the luminance histogram, its reduce and the metered display)
HR_EXPOSURE_API_VERSION = 1
HR_EXPOSURE_BINS = 256
HR_EXPOSURE_EMPTY, HR_EXPOSURE_CLAMPED_LOW, HR_EXPOSURE_CLAMPED_HIGH, HR_EXPOSURE_ADAPTED = 1, 2, 4, 8


class ExposureParams(Struct):
    _cname_ = "hr_exposure_params"
    _fields_ = [("key", C.c_float), ("low_permille", C.c_int32), ("high_permille", C.c_int32), ("min_scale", C.c_float), ("max_scale", C.c_float),
                ("adapt", C.c_float), ("window", C.c_int32 * 4), ("reserved", C.c_uint32 * 6)]


class ExposureResult(Struct):
    _cname_ = "hr_exposure_result"
    _fields_ = [("scale", C.c_float), ("target", C.c_float), ("key_luminance", C.c_float), ("position", C.c_uint32), ("counted", C.c_uint64),
                ("used", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64), ("nonfinite", C.c_uint64), ("invalid", C.c_uint64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


# -- include/hrcore_metric.h (the convergence metric: exact relative L2 against a reference, or predicted from the sample moments)
HR_METRIC_API_VERSION = 1
HR_METRIC_BINS = 256
HR_METRIC_COMPARE, HR_METRIC_ESTIMATE = 0, 1
HR_METRIC_EMPTY, HR_METRIC_ZERO_DENOMINATOR = 1, 2


class MetricParams(Struct):
    _cname_ = "hr_metric_params"
    _fields_ = [("window", C.c_int32 * 4), ("reserved", C.c_uint32 * 4)]


class MetricResult(Struct):
    _cname_ = "hr_metric_result"
    _fields_ = [("num", C.c_double), ("den", C.c_double), ("value", C.c_double), ("mse", C.c_double), ("counted", C.c_uint64), ("differing", C.c_uint64),
                ("nonfinite", C.c_uint64), ("skipped", C.c_uint64), ("max_abs", C.c_float), ("passes", C.c_uint32), ("kind", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


# -- include/hrcore_despeckle.h (firefly suppression: the outlier clamp ahead of the denoiser)
HR_DESPECKLE_API_VERSION = 1
HR_DESPECKLE_RANK_HIGHEST, HR_DESPECKLE_TAPS = 4, 24


class DespeckleParams(Struct):
    _cname_ = "hr_despeckle_params"
    _fields_ = [("rank", C.c_int32), ("min_taps", C.c_int32), ("ratio", C.c_float), ("sigmas", C.c_float), ("floor", C.c_float), ("reserved", C.c_uint32 * 3)]


class DespeckleResult(Struct):
    _cname_ = "hr_despeckle_result"
    _fields_ = [("valid_pixels", C.c_uint64), ("clamped_pixels", C.c_uint64), ("kept_pixels", C.c_uint64), ("starved_pixels", C.c_uint64),
                ("nonfinite_pixels", C.c_uint64), ("reserved", C.c_uint64 * 3)]


# -- include/hrcore_mesh.h (mesh preparation: smooth normals and tangent frames for a mesh without them)
HR_MESH_API_VERSION = 1
HR_MESH_WEIGHT_ANGLE, HR_MESH_WEIGHT_AREA, HR_MESH_WEIGHT_UNIFORM = 0, 1, 2
HR_MESH_WANT_NORMALS, HR_MESH_WANT_TANGENTS = 1, 2


class MeshParams(Struct):
    _cname_ = "hr_mesh_params"
    _fields_ = [("weight", C.c_int32), ("weld", C.c_int32), ("want", C.c_int32), ("reserved", C.c_int32 * 5)]


class MeshResult(Struct):
    _cname_ = "hr_mesh_result"
    _fields_ = [("triangles", C.c_uint64), ("degenerate_triangles", C.c_uint64), ("degenerate_uv_triangles", C.c_uint64), ("weld_groups", C.c_uint64),
                ("unreferenced_vertices", C.c_uint64), ("cancelled_vertices", C.c_uint64), ("fallback_tangents", C.c_uint64), ("max_valence", C.c_uint64)]


# -- include/hrcore_deform.h (deformable meshes: vertex updates in place, device posing, attribute read-back)
HR_DEFORM_API_VERSION = 1
(HR_GEOM_POSITIONS, HR_GEOM_NORMALS, HR_GEOM_UVS, HR_GEOM_TANGENTS, HR_GEOM_BITANGENTS, HR_GEOM_COLORS) = range(6)
HR_DEFORM_NORMALS, HR_DEFORM_TANGENTS = 1, 2
HR_DEFORM_MAX_MORPH, HR_DEFORM_MAX_JOINTS = 8, 1024


class DeformParams(Struct):
    _cname_ = "hr_deform_params"
    _fields_ = [("regenerate", C.c_int32), ("weight", C.c_int32), ("weld", C.c_int32), ("reserved", C.c_int32 * 5)]


class DeformRig(Struct):
    _cname_ = "hr_deform_rig"
    _fields_ = [("morph_positions", f32p), ("morph_normals", f32p), ("joints", u32p), ("weights", f32p), ("n_morph", C.c_int32), ("n_joints", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class DeformResult(Struct):
    _cname_ = "hr_deform_result"
    _fields_ = [("vertices", C.c_uint64), ("triangles", C.c_uint64), ("rejected_vertices", C.c_uint64), ("kept_directions", C.c_uint64),
                ("regenerated", C.c_uint32), ("posed", C.c_uint32), ("mesh", MeshResult)]


# -- include/hrcore_query.h (ray queries: the caller's rays traced on the device, with surface records)
HR_QUERY_API_VERSION = 1
HR_QUERY_ANY_HIT = 1
HR_QUERY_INVALID_RAY = -2
HR_QUERY_SF_FRONT, HR_QUERY_SF_HAS_UV, HR_QUERY_SF_NON_OCCLUDER = 1, 2, 4


class QuerySurface(Struct):
    _cname_ = "hr_query_surface"
    _fields_ = [("geom", C.c_int32), ("material", C.c_int32), ("prim_in_geom", C.c_int32), ("flags", C.c_uint32), ("position", C.c_float * 3),
                ("normal", C.c_float * 3), ("geometric_normal", C.c_float * 3), ("uv", C.c_float * 2), ("reserved", C.c_float)]


SURFACE_DTYPE = np.dtype([("geom", np.int32), ("material", np.int32), ("prim_in_geom", np.int32), ("flags", np.uint32), ("position", np.float32, (3,)),
                          ("normal", np.float32, (3,)), ("geometric_normal", np.float32, (3,)), ("uv", np.float32, (2,)), ("reserved", np.float32)])


class QueryDesc(Struct):
    _cname_ = "hr_query_desc"
    _fields_ = [("n", C.c_int32), ("flags", C.c_uint32), ("origins", C.c_void_p), ("directions", C.c_void_p), ("tmax", C.c_void_p), ("skip_prim", C.c_void_p),
                ("origin_stride", C.c_int32), ("direction_stride", C.c_int32), ("tmax_stride", C.c_int32), ("skip_stride", C.c_int32), ("tmin", C.c_float),
                ("reserved", C.c_uint32 * 3), ("hits", C.c_void_p), ("surfaces", C.c_void_p)]


class QueryResult(Struct):
    _cname_ = "hr_query_result"
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("invalid", C.c_uint64), ("reserved", C.c_uint64 * 5)]


# -- include/hrcore_motion.h (motion reprojection: the history gathered where a moved or deformed surface was)
HR_MOTION_API_VERSION = 1


class MotionTraceResult(Struct):
    _cname_ = "hr_motion_trace_result"
    _fields_ = [("surface_pixels", C.c_uint64), ("sky_pixels", C.c_uint64), ("unmatched_pixels", C.c_uint64), ("reserved", C.c_uint64)]


class MotionResult(Struct):
    _cname_ = "hr_motion_result"
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("history_passes", C.c_uint32),
                ("passes", C.c_uint32), ("surface_pixels", C.c_uint64), ("sky_pixels", C.c_uint64), ("unmatched_pixels", C.c_uint64)]


class MotionInfo(Struct):
    _cname_ = "hr_motion_info_t"
    _fields_ = [("snapshot", C.c_int32), ("traced", C.c_int32), ("triangles", C.c_uint32), ("meshes", C.c_uint32), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {"snapshot": bool(self.snapshot), "traced": bool(self.traced), "triangles": int(self.triangles), "meshes": int(self.meshes), "bytes": int(self.bytes)}


# -- the prototypes: header -> {function (the suffix after the library's prefix): its argtypes}, every function the header declares, in the
# header's order of features.  The result is an int status, but for <x>_version (uint32_t), <x>_default_params (void) and last_error (char*):
# restype().  Kinds: ctx = hr_ctx* (opaque); P(Struct) = a pointer to that struct, in or out; f32p / u8p / i32p / u32p / u64p = arrays and
# scalar outs; P(f32p) / P(vp) = a pointer the library hands out; vp = void* (a device pointer, a stream, host pixels); cp = char*;
# i32 (also hr_geom_id, hr_tex_id) and u32 by value.  query_pixels takes its numpy record arrays as P(Hit) / P(QuerySurface) like debug_trace,
# not as void*.  motion_vectors' device_out is a float* in the header, so a raw device address is cast at the call
ctx, vp, cp, i32, u32 = C.c_void_p, C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32
PROTOTYPES = {
    "hrcore.h": {
        "abi_version": (),
        "ctx_create": (P(CtxDesc), P(ctx)),
        "ctx_destroy": (ctx,),
        "last_error": (ctx,),
        "ctx_set_stream": (ctx, vp),
        "frame_resize": (ctx, i32, i32),
        "frame_bind_external": (ctx, vp),
        "frame_device_ptr": (ctx, P(vp)),
        "geom_add": (ctx, P(MeshDesc), i32p),
        "geom_remove": (ctx, i32),
        "geom_set_transform": (ctx, i32, f32p),
        "scene_clear": (ctx,),
        "scene_commit": (ctx,),
        "scene_get_info": (ctx, P(SceneInfo)),
        "texture_create": (ctx, P(TextureDesc), vp, i32p),
        "texture_destroy": (ctx, i32),
        "material_set": (ctx, i32, P(Material)),
        "lights_set": (ctx, P(Lights)),
        "sequences_set": (ctx, f32p, f32p, i32, i32),
        "seq_offsets_set": (ctx, f32p, i32),
        "qmc_generate": (ctx, i32, u32, u32, i32, f32p),
        "aperture_generate": (ctx, i32, u32, u32, f32p),
        "sequences_generate": (ctx, i32, i32, i32),
        "seq_offsets_generate": (ctx,),
        "multiscatter_lut_generate": (ctx, f32p, i32p),
        "clear": (ctx,),
        "render_pass": (ctx, P(PassParams)),
        "flush": (ctx,),
        "get_stats": (ctx, P(PassStats)),
        "get_kernel_times": (ctx, P(KernelTimes)),
        "readback": (ctx, P(f32p), i32p, i32p),
        "synchronize": (ctx,),
        "debug_trace": (ctx, i32, f32p, f32p, f32p, i32p, i32, P(Hit)),
        "display": (ctx, P(DisplayParams), i32, vp, u32p),
        "display_readback": (ctx, P(DisplayParams), i32, P(vp), i32p, i32p, u32p),
        "frame_passes_resolved": (ctx, u64p),
        "get_step_log": (ctx, P(StepRecord), i32, i32p),
        "readback_progressive": (ctx, P(f32p), i32p, i32p, u32p),
        "frame_packed_slots": (ctx, i32, i32, u64p),
        "frame_pack_owned": (ctx, vp, vp),
        "frame_unpack": (ctx, i32, i32, vp, vp, vp),
        "frame_pass_batch": (ctx, i32, i32p),
        "interactive_blocks_set": (ctx, i32p, i32, i32),
        "scene_cache": (ctx, cp),
    },
    "hrcore_group.h": {
        "group_api_version": (),
        "ctx_create_group": (P(CtxDesc), i32p, i32, P(ctx)),
        "group_get_info": (ctx, P(GroupInfo)),
        "group_member_stats": (ctx, i32, P(PassStats), P(KernelTimes)),
    },
    "hrcore_aov.h": {
        "aov_api_version": (),
        "aov_enable": (ctx, u32),
        "aov_mask": (ctx, u32p),
        "aov_readback": (ctx, i32, P(f32p), i32p, i32p, u64p),
        "aov_copy": (ctx, i32, vp, vp),
    },
    "hrcore_denoise.h": {
        "denoise_api_version": (),
        "denoise_default_params": (P(DenoiseParams),),
        "denoise": (ctx, P(DenoiseParams), vp, vp, u32p),
        "denoise_readback": (ctx, P(DenoiseParams), P(f32p), i32p, i32p, u32p),
        "denoise_display": (ctx, P(DenoiseParams), P(DisplayParams), i32, vp, u32p),
    },
    "hrcore_denoise_spatial.h": {
        "denoise_spatial_api_version": (),
        "denoise_spatial_default_params": (P(DenoiseSpatialParams),),
        "denoise_spatial": (ctx, P(DenoiseParams), P(DenoiseSpatialParams), vp, vp, u32p, P(DenoiseSpatialResult)),
        "denoise_spatial_readback": (ctx, P(DenoiseParams), P(DenoiseSpatialParams), P(f32p), i32p, i32p, u32p, P(DenoiseSpatialResult)),
        "denoise_spatial_display": (ctx, P(DenoiseParams), P(DenoiseSpatialParams), P(DisplayParams), i32, vp, u32p),
        "denoise_spatial_variance": (ctx, P(DenoiseParams), P(DenoiseSpatialParams), f32p, P(DenoiseSpatialResult)),
    },
    "hrcore_adaptive.h": {
        "adaptive_api_version": (),
        "sample_mask_set": (ctx, u8p),
        "sample_mask_get": (ctx, u8p, i32p),
        "adaptive_default_params": (P(AdaptiveParams),),
        "adaptive_update": (ctx, P(AdaptiveParams), i32, P(AdaptiveResult)),
        "adaptive_error_copy": (ctx, vp, vp),
        "adaptive_error_readback": (ctx, f32p),
    },
    "hrcore_history.h": {
        "history_api_version": (),
        "history_default_params": (P(HistoryParams),),
        "history_capture": (ctx, P(PassParams)),
        "history_merge": (ctx, P(PassParams), P(HistoryParams), P(HistoryResult)),
        "history_drop": (ctx,),
        "history_info": (ctx, i32p, u32p),
        "history_readback": (ctx, f32p),
    },
    "hrcore_reproject.h": {
        "reproject_api_version": (),
        "reproject_merge": (ctx, P(PassParams), P(HistoryParams), P(ReprojectResult)),
        "reproject_examined_get": (ctx, u8p),
        "reproject_preview": (ctx, P(PassParams), P(HistoryParams), vp, vp, P(ReprojectPreviewResult)),
        "reproject_preview_readback": (ctx, P(PassParams), P(HistoryParams), P(f32p), i32p, i32p, P(ReprojectPreviewResult)),
    },
    "hrcore_tree.h": {
        "tree_api_version": (),
        "scene_get_tree_info": (ctx, P(TreeInfo)),
        "scene_tree_layout": (ctx, P(TreeLayout)),
        "scene_tree_read": (ctx, i32, vp, C.c_uint64),
    },
    "hrcore_exposure.h": {
        "exposure_api_version": (),
        "exposure_default_params": (P(ExposureParams),),
        "exposure_meter": (ctx, P(ExposureParams), vp, P(ExposureResult)),
        "exposure_display": (ctx, P(ExposureParams), P(DisplayParams), i32, vp, vp, u32p),
        "exposure_last": (ctx, P(ExposureResult), u64p),
        "exposure_reset": (ctx,),
    },
    "hrcore_metric.h": {
        "metric_api_version": (),
        "metric_default_params": (P(MetricParams),),
        "metric_compare": (ctx, P(MetricParams), vp, vp, P(MetricResult)),
        "metric_estimate": (ctx, P(MetricParams), P(MetricResult)),
        "metric_last": (ctx, P(MetricResult), u64p, u64p),
    },
    "hrcore_despeckle.h": {
        "despeckle_api_version": (),
        "despeckle_default_params": (P(DespeckleParams),),
        "despeckle": (ctx, P(DespeckleParams), vp, vp, vp, vp, vp, u32p, P(DespeckleResult)),
        "despeckle_readback": (ctx, P(DespeckleParams), P(f32p), P(f32p), i32p, i32p, u32p, P(DespeckleResult)),
        "despeckle_denoise": (ctx, P(DespeckleParams), P(DenoiseParams), i32, P(DenoiseSpatialParams), vp, vp, u32p, P(DespeckleResult)),
        "despeckle_denoise_readback": (ctx, P(DespeckleParams), P(DenoiseParams), i32, P(DenoiseSpatialParams), P(f32p), i32p, i32p, u32p,
                                       P(DespeckleResult)),
    },
    "hrcore_mesh.h": {
        "mesh_api_version": (),
        "mesh_default_params": (P(MeshParams),),
        "mesh_prepare": (ctx, P(MeshDesc), P(MeshParams), f32p, f32p, f32p, P(MeshResult)),
        "mesh_last": (ctx, P(MeshResult)),
    },
    "hrcore_deform.h": {
        "deform_api_version": (),
        "deform_default_params": (P(DeformParams),),
        "geom_update": (ctx, i32, P(MeshDesc), P(DeformParams), P(DeformResult)),
        "geom_get_attribute": (ctx, i32, i32, f32p),
        "deform_bind": (ctx, i32, P(DeformRig)),
        "deform_pose": (ctx, i32, f32p, f32p, P(DeformParams), P(DeformResult)),
        "deform_unbind": (ctx, i32),
        "deform_last": (ctx, P(DeformResult)),
    },
    "hrcore_query.h": {
        "query_api_version": (),
        "query_trace": (ctx, P(QueryDesc), vp),
        "query_trace_host": (ctx, P(QueryDesc)),
        "query_pixels": (ctx, P(PassParams), i32, f32p, P(Hit), P(QuerySurface), f32p),
        "query_last": (ctx, P(QueryResult)),
    },
    "hrcore_motion.h": {
        "motion_api_version": (),
        "motion_default_params": (P(HistoryParams),),
        "motion_snapshot": (ctx,),
        "motion_trace": (ctx, P(PassParams), P(MotionTraceResult)),
        "motion_merge": (ctx, P(PassParams), P(HistoryParams), P(MotionResult)),
        "motion_vectors": (ctx, P(PassParams), f32p, vp),
        "motion_vectors_readback": (ctx, P(PassParams), f32p),
        "motion_readback": (ctx, f32p),
        "motion_snapshot_readback": (ctx, f32p),
        "motion_drop": (ctx,),
        "motion_info": (ctx, P(MotionInfo)),
    },
}


def restype(name):
    return C.c_uint32 if name.endswith("_version") else None if name.endswith("_default_params") else cp if name == "last_error" else C.c_int


# every symbol each header declares (suffix after the prefix): the keys of its prototypes
(ABI_SYMBOLS, GROUP_SYMBOLS, AOV_SYMBOLS, DENOISE_SYMBOLS, DENOISE_SPATIAL_SYMBOLS, ADAPTIVE_SYMBOLS, HISTORY_SYMBOLS, REPROJECT_SYMBOLS, TREE_SYMBOLS,
 EXPOSURE_SYMBOLS, METRIC_SYMBOLS, DESPECKLE_SYMBOLS, MESH_SYMBOLS, DEFORM_SYMBOLS, QUERY_SYMBOLS, MOTION_SYMBOLS) = (list(p) for p in PROTOTYPES.values())

# The optional headers: feature ->(its symbols, the version the binding was written against, what "this library has no ..." calls it);
# the version function is <feature>_api_version.  Engine._feature_call checks a feature on its first call
FEATURES = {
    "aov": (AOV_SYMBOLS, HR_AOV_API_VERSION, "AOVs"),
    "denoise": (DENOISE_SYMBOLS, HR_DENOISE_API_VERSION, "denoiser"),
    "denoise_spatial": (DENOISE_SPATIAL_SYMBOLS, HR_DENOISE_SPATIAL_API_VERSION, "spatial variance estimate"),
    "adaptive": (ADAPTIVE_SYMBOLS, HR_ADAPTIVE_API_VERSION, "adaptive sampling"),
    "history": (HISTORY_SYMBOLS, HR_HISTORY_API_VERSION, "history reprojection"),
    "reproject": (REPROJECT_SYMBOLS, HR_REPROJECT_API_VERSION, "progressive history merge"),
    "tree": (TREE_SYMBOLS, HR_TREE_API_VERSION, "tree build report"),
    "exposure": (EXPOSURE_SYMBOLS, HR_EXPOSURE_API_VERSION, "auto-exposure"),
    "metric": (METRIC_SYMBOLS, HR_METRIC_API_VERSION, "convergence metric"),
    "despeckle": (DESPECKLE_SYMBOLS, HR_DESPECKLE_API_VERSION, "firefly suppression"),
    "mesh": (MESH_SYMBOLS, HR_MESH_API_VERSION, "mesh preparation"),
    "deform": (DEFORM_SYMBOLS, HR_DEFORM_API_VERSION, "deformable meshes"),
    "query": (QUERY_SYMBOLS, HR_QUERY_API_VERSION, "ray queries"),
    "motion": (MOTION_SYMBOLS, HR_MOTION_API_VERSION, "motion reprojection"),
}
