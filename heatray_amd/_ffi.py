"""ctypes view of include/hrcore.h.

`Engine` drives any shared library that exports the C-ABI of include/hrcore.h under
a given symbol prefix.  The product binds it to libhrcore.so (prefix ``hr_``, see
heatray_amd.core); the test-suite binds the same class to the CPU oracle (prefix
``ora_``) so both are fed identical POD inputs.  Nothing in this package loads the
oracle.
"""
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

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)


class CtxDesc(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("tile_size", C.c_int32),
                ("stream", C.c_void_p), ("flags", C.c_uint32), ("memory_budget", C.c_uint64)]


class MeshDesc(C.Structure):
    _fields_ = [("positions", f32p), ("normals", f32p), ("uvs", f32p), ("tangents", f32p), ("bitangents", f32p),
                ("colors", f32p), ("position_stride", C.c_int32), ("normal_stride", C.c_int32),
                ("uv_stride", C.c_int32), ("tangent_stride", C.c_int32), ("bitangent_stride", C.c_int32),
                ("color_stride", C.c_int32), ("n_vertices", C.c_int32), ("indices", u32p), ("n_indices", C.c_int32),
                ("mode", C.c_int32), ("world_from_entity", C.c_float * 16), ("front_face_cw", C.c_int32),
                ("is_occluder", C.c_int32), ("material_id", C.c_int32)]


class SceneInfo(C.Structure):
    _fields_ = [("n_triangles", C.c_uint64), ("n_nodes", C.c_uint64), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("ray_epsilon", C.c_float), ("build_ms", C.c_float),
                ("bvh_levels", C.c_uint32), ("refitted", C.c_uint32),
                ("box_area_ratio", C.c_float), ("builder", C.c_uint32), ("cost_radix", C.c_float), ("cost_ploc", C.c_float)]


class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("dtype", C.c_int32),
                ("wrap_s", C.c_int32), ("wrap_t", C.c_int32), ("filter", C.c_int32)]


class Material(C.Structure):
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


class Lights(C.Structure):
    _fields_ = [("n_directional", C.c_int32), ("directional_directions", V3x5), ("directional_colors", V3x5),
                ("n_point", C.c_int32), ("point_positions", V3x5), ("point_colors", V3x5), ("n_spot", C.c_int32),
                ("spot_positions", V3x5), ("spot_directions", V3x5), ("spot_colors", V3x5), ("spot_angles", V2x5),
                ("env_enabled", C.c_int32), ("env_texture", C.c_int32), ("env_exposure", C.c_float),
                ("env_theta_rotation", C.c_float)]


class PassParams(C.Structure):
    _fields_ = [("sample_index", C.c_int32), ("max_ray_depth", C.c_int32), ("max_channel_value", C.c_float),
                ("fov_tan", C.c_float), ("aspect_ratio", C.c_float), ("focus_distance", C.c_float),
                ("aperture_radius", C.c_float), ("view_matrix", C.c_float * 16), ("interactive_mode", C.c_int32),
                ("block_size", C.c_int32 * 2), ("current_block_pixel", C.c_int32 * 2), ("max_sample_index", C.c_float),
                ("enable_visualizer", C.c_int32), ("visualizer_mode", C.c_int32),
                ("enable_accumulator_visualizer", C.c_int32), ("show_nans", C.c_int32), ("show_inf", C.c_int32),
                ("estimator", C.c_int32), ("texture_lod", C.c_int32)]


class PassStats(C.Structure):
    _fields_ = [("ms", C.c_float), ("paths", C.c_uint64), ("rays_closest", C.c_uint64), ("rays_any", C.c_uint64),
                ("shaded_hits", C.c_uint64), ("accumulates", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("node_visits_any", C.c_uint64), ("tri_tests_any", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class StepRecord(C.Structure):
    _fields_ = [("start_ms", C.c_double), ("trace_ms", C.c_float), ("passes_in_flight", C.c_int32), ("passes_injected", C.c_int32), ("group", C.c_int32)]


class KernelTimes(C.Structure):
    _fields_ = [("ms", C.c_float * 4), ("launches", C.c_uint32 * 4), ("trace_clock_ms", C.c_float), ("trace_clock_launches", C.c_uint32),
                ("camera_packets", C.c_uint32), ("packet_union", C.c_float)]


class DisplayParams(C.Structure):
    """hr_display_params: HeatrayRenderer.h:104-117 PostProcessingParams as DisplayProgram::bind uploads them."""
    _fields_ = [("tonemapping_enabled", C.c_int32), ("camera_exposure", C.c_float), ("brightness", C.c_float),
                ("contrast", C.c_float), ("hue", C.c_float), ("saturation", C.c_float), ("vibrance", C.c_float),
                ("red", C.c_float), ("green", C.c_float), ("blue", C.c_float), ("vignette_intensity", C.c_float),
                ("vignette_falloff", C.c_float)]


def display_params(tonemapping_enabled=False, exposure=0.0, brightness=0.0, contrast=1.0, hue=1.0, saturation=1.0,
                   vibrance=0.0, red=1.0, green=1.0, blue=1.0, vignette_intensity=0.0, vignette_falloff=1.0):
    """Defaults = the reference's PostProcessingParams defaults; camera_exposure = 2^exposure (computed in binary32 by
    repeated doubling / halving for integral exposures, else through numpy's float32 power, as std::powf would)."""
    return DisplayParams(int(bool(tonemapping_enabled)), float(np.float32(2.0) ** np.float32(exposure)), brightness, contrast, hue,
                         saturation, vibrance, red, green, blue, vignette_intensity, vignette_falloff)


HR_DISPLAY_RGBA8, HR_DISPLAY_RGBA32F, HR_DISPLAY_HDR_RGBA32F = 0, 1, 2
HR_DISPLAY_PROGRESSIVE = 0x100


class Hit(C.Structure):
    _fields_ = [("prim", C.c_int32), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float)]


HIT_DTYPE = np.dtype([("prim", np.int32), ("t", np.float32), ("u", np.float32), ("v", np.float32)])

# every symbol include/hrcore.h declares (suffix after the prefix)
HR_ABI_VERSION = 6  # include/hrcore.h: checked against the loaded library before the first call (Engine.__init__)
ABI_SYMBOLS = [
    "abi_version", "ctx_create", "ctx_destroy", "last_error", "ctx_set_stream", "frame_resize", "frame_bind_external",
    "frame_device_ptr", "geom_add", "geom_remove", "geom_set_transform", "scene_clear", "scene_commit",
    "scene_get_info", "texture_create", "texture_destroy", "material_set", "lights_set", "sequences_set",
    "seq_offsets_set", "qmc_generate", "aperture_generate", "sequences_generate", "seq_offsets_generate", "multiscatter_lut_generate",
    "clear", "render_pass", "flush", "get_stats", "get_kernel_times", "readback", "synchronize", "debug_trace",
    "display", "display_readback", "frame_passes_resolved", "get_step_log", "readback_progressive", "frame_packed_slots", "frame_pack_owned", "frame_unpack",
    "frame_pass_batch", "interactive_blocks_set", "scene_cache",
]

# every symbol include/hrcore_group.h declares (context groups; a library without them still loads, create_group then fails)
HR_GROUP_API_VERSION = 1
HR_GROUP_MAX_MEMBERS = 16
GROUP_SYMBOLS = ["group_api_version", "ctx_create_group", "group_get_info", "group_member_stats"]


# every symbol include/hrcore_aov.h declares (AOVs).  Resolved lazily, on the first AOV call: a library without them (the CPU oracle)
# still makes an Engine, and its AOV calls raise EngineError
HR_AOV_API_VERSION = 1
HR_AOV_SURFACE, HR_AOV_MOMENTS = 1, 2
HR_AOV_PLANE_ALBEDO, HR_AOV_PLANE_NORMAL_DEPTH, HR_AOV_PLANE_MOMENTS = 0, 1, 2
AOV_PLANE_NAMES = ("albedo", "normal_depth", "moments")
AOV_SYMBOLS = ["aov_api_version", "aov_enable", "aov_mask", "aov_readback", "aov_copy"]


# every symbol include/hrcore_denoise.h declares (the denoiser over the AOV planes).  Resolved lazily like the AOV symbols
HR_DENOISE_API_VERSION = 1
HR_DENOISE_MAX_ITERATIONS, HR_DENOISE_MAX_NORMAL_POWER = 8, 16
HR_DENOISE_KERNEL_AUTO, HR_DENOISE_KERNEL_PLAIN, HR_DENOISE_KERNEL_TILED = 0, 1, 2
DENOISE_SYMBOLS = ["denoise_api_version", "denoise_default_params", "denoise", "denoise_readback", "denoise_display"]


class DenoiseParams(C.Structure):
    """hr_denoise_params"""
    _fields_ = [("iterations", C.c_int32), ("normal_power", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("kernel", C.c_int32), ("reserved", C.c_uint32 * 3)]


# every symbol include/hrcore_denoise_spatial.h declares (the denoiser with a spatial variance estimate for pixels with few samples).
# Resolved lazily like the AOV symbols
HR_DENOISE_SPATIAL_API_VERSION = 1
HR_DENOISE_SPATIAL_BELOW_LOWEST, HR_DENOISE_SPATIAL_BELOW_HIGHEST = 2, 64
HR_DENOISE_SPATIAL_MIN_TAPS_LOWEST, HR_DENOISE_SPATIAL_MIN_TAPS_HIGHEST = 2, 49
DENOISE_SPATIAL_SYMBOLS = ["denoise_spatial_api_version", "denoise_spatial_default_params", "denoise_spatial", "denoise_spatial_readback", "denoise_spatial_display",
                           "denoise_spatial_variance"]


class DenoiseSpatialParams(C.Structure):
    """hr_denoise_spatial_params"""
    _fields_ = [("below", C.c_int32), ("min_taps", C.c_int32), ("reserved", C.c_uint32 * 6)]


class DenoiseSpatialResult(C.Structure):
    """hr_denoise_spatial_result"""
    _fields_ = [("spatial_pixels", C.c_uint64), ("estimated_pixels", C.c_uint64), ("starved_pixels", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/hrcore_adaptive.h declares (the sample mask and the error estimate that builds it).  Resolved lazily like the AOV symbols
HR_ADAPTIVE_API_VERSION = 1
HR_ADAPTIVE_MIN_SAMPLES_LOWEST, HR_ADAPTIVE_MIN_SAMPLES_HIGHEST, HR_ADAPTIVE_MAX_RADIUS = 2, 65536, 4
ADAPTIVE_SYMBOLS = ["adaptive_api_version", "sample_mask_set", "sample_mask_get", "adaptive_default_params", "adaptive_update", "adaptive_error_copy", "adaptive_error_readback"]


class AdaptiveParams(C.Structure):
    """hr_adaptive_params"""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_int32), ("radius", C.c_int32), ("reserved", C.c_uint32 * 4)]


class AdaptiveResult(C.Structure):
    """hr_adaptive_result"""
    _fields_ = [("unconverged_pixels", C.c_uint64), ("active_pixels", C.c_uint64), ("max_error", C.c_float), ("passes", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/hrcore_history.h declares (history reprojection across a camera change).  Resolved lazily like the AOV symbols
HR_HISTORY_API_VERSION = 1
HR_HISTORY_MAX_HISTORY_LOWEST, HR_HISTORY_MAX_HISTORY_HIGHEST = 1, 65536
HISTORY_SYMBOLS = ["history_api_version", "history_default_params", "history_capture", "history_merge", "history_drop", "history_info", "history_readback"]


class HistoryParams(C.Structure):
    """hr_history_params"""
    _fields_ = [("max_history", C.c_int32), ("normal_cos", C.c_float), ("plane_tol", C.c_float), ("min_weight", C.c_float), ("reserved", C.c_uint32 * 4)]


class HistoryResult(C.Structure):
    """hr_history_result"""
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("history_passes", C.c_uint32),
                ("passes", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/hrcore_reproject.h declares (the progressive history merge and the preview of unsampled pixels).  Resolved lazily
# like the AOV symbols
HR_REPROJECT_API_VERSION = 1
REPROJECT_SYMBOLS = ["reproject_api_version", "reproject_merge", "reproject_examined_get", "reproject_preview", "reproject_preview_readback"]


class ReprojectResult(C.Structure):
    """hr_reproject_result"""
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("pending_pixels", C.c_uint64),
                ("examined_pixels", C.c_uint64), ("history_passes", C.c_uint32), ("passes", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReprojectPreviewResult(C.Structure):
    """hr_reproject_preview_result"""
    _fields_ = [("own_pixels", C.c_uint64), ("previewed_pixels", C.c_uint64), ("empty_pixels", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/hrcore_tree.h declares (what the last tree build did to the radix tree's bottom subtrees)
HR_TREE_API_VERSION = 1
TREE_SYMBOLS = ["tree_api_version", "scene_get_tree_info"]


class TreeInfo(C.Structure):
    """hr_tree_info"""
    _fields_ = [("cost_before", C.c_float), ("cost_after", C.c_float), ("subtrees_found", C.c_uint32), ("subtrees_replaced", C.c_uint32),
                ("max_triangles", C.c_uint32), ("reserved", C.c_uint32 * 3)]


# every symbol include/hrcore_exposure.h declares (auto-exposure: the luminance histogram, its reduce and the metered display).  Resolved
# lazily like the AOV symbols
HR_EXPOSURE_API_VERSION = 1
HR_EXPOSURE_BINS = 256
HR_EXPOSURE_EMPTY, HR_EXPOSURE_CLAMPED_LOW, HR_EXPOSURE_CLAMPED_HIGH, HR_EXPOSURE_ADAPTED = 1, 2, 4, 8
EXPOSURE_SYMBOLS = ["exposure_api_version", "exposure_default_params", "exposure_meter", "exposure_display", "exposure_last", "exposure_reset"]


class ExposureParams(C.Structure):
    """hr_exposure_params"""
    _fields_ = [("key", C.c_float), ("low_permille", C.c_int32), ("high_permille", C.c_int32), ("min_scale", C.c_float), ("max_scale", C.c_float),
                ("adapt", C.c_float), ("window", C.c_int32 * 4), ("reserved", C.c_uint32 * 6)]


class ExposureResult(C.Structure):
    """hr_exposure_result"""
    _fields_ = [("scale", C.c_float), ("target", C.c_float), ("key_luminance", C.c_float), ("position", C.c_uint32), ("counted", C.c_uint64),
                ("used", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64), ("nonfinite", C.c_uint64), ("invalid", C.c_uint64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# every symbol include/hrcore_metric.h declares (the convergence metric: exact relative L2 against a reference, or predicted from the sample
# moments).  Resolved lazily like the AOV symbols
HR_METRIC_API_VERSION = 1
HR_METRIC_BINS = 256
HR_METRIC_COMPARE, HR_METRIC_ESTIMATE = 0, 1
HR_METRIC_EMPTY, HR_METRIC_ZERO_DENOMINATOR = 1, 2
METRIC_SYMBOLS = ["metric_api_version", "metric_default_params", "metric_compare", "metric_estimate", "metric_last"]


class MetricParams(C.Structure):
    """hr_metric_params"""
    _fields_ = [("window", C.c_int32 * 4), ("reserved", C.c_uint32 * 4)]


class MetricResult(C.Structure):
    """hr_metric_result"""
    _fields_ = [("num", C.c_double), ("den", C.c_double), ("value", C.c_double), ("mse", C.c_double), ("counted", C.c_uint64), ("differing", C.c_uint64),
                ("nonfinite", C.c_uint64), ("skipped", C.c_uint64), ("max_abs", C.c_float), ("passes", C.c_uint32), ("kind", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# every symbol include/hrcore_despeckle.h declares (firefly suppression: the outlier clamp ahead of the denoiser).  Resolved lazily like
# the AOV symbols
HR_DESPECKLE_API_VERSION = 1
HR_DESPECKLE_RANK_HIGHEST, HR_DESPECKLE_TAPS = 4, 24
DESPECKLE_SYMBOLS = ["despeckle_api_version", "despeckle_default_params", "despeckle", "despeckle_readback", "despeckle_denoise", "despeckle_denoise_readback"]


class DespeckleParams(C.Structure):
    """hr_despeckle_params"""
    _fields_ = [("rank", C.c_int32), ("min_taps", C.c_int32), ("ratio", C.c_float), ("sigmas", C.c_float), ("floor", C.c_float), ("reserved", C.c_uint32 * 3)]


class DespeckleResult(C.Structure):
    """hr_despeckle_result"""
    _fields_ = [("valid_pixels", C.c_uint64), ("clamped_pixels", C.c_uint64), ("kept_pixels", C.c_uint64), ("starved_pixels", C.c_uint64),
                ("nonfinite_pixels", C.c_uint64), ("reserved", C.c_uint64 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


# every symbol include/hrcore_mesh.h declares (mesh preparation: smooth normals and tangent frames for a mesh without them).  Resolved
# lazily like the AOV symbols
HR_MESH_API_VERSION = 1
HR_MESH_WEIGHT_ANGLE, HR_MESH_WEIGHT_AREA, HR_MESH_WEIGHT_UNIFORM = 0, 1, 2
HR_MESH_WANT_NORMALS, HR_MESH_WANT_TANGENTS = 1, 2
MESH_SYMBOLS = ["mesh_api_version", "mesh_default_params", "mesh_prepare", "mesh_last"]


class MeshParams(C.Structure):
    """hr_mesh_params"""
    _fields_ = [("weight", C.c_int32), ("weld", C.c_int32), ("want", C.c_int32), ("reserved", C.c_int32 * 5)]


class MeshResult(C.Structure):
    """hr_mesh_result"""
    _fields_ = [("triangles", C.c_uint64), ("degenerate_triangles", C.c_uint64), ("degenerate_uv_triangles", C.c_uint64), ("weld_groups", C.c_uint64),
                ("unreferenced_vertices", C.c_uint64), ("cancelled_vertices", C.c_uint64), ("fallback_tangents", C.c_uint64), ("max_valence", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/hrcore_deform.h declares (deformable meshes: vertex updates in place, device posing, attribute read-back).
# Resolved lazily like the AOV symbols
HR_DEFORM_API_VERSION = 1
(HR_GEOM_POSITIONS, HR_GEOM_NORMALS, HR_GEOM_UVS, HR_GEOM_TANGENTS, HR_GEOM_BITANGENTS, HR_GEOM_COLORS) = range(6)
HR_DEFORM_NORMALS, HR_DEFORM_TANGENTS = 1, 2
HR_DEFORM_MAX_MORPH, HR_DEFORM_MAX_JOINTS = 8, 1024
DEFORM_SYMBOLS = ["deform_api_version", "deform_default_params", "geom_update", "geom_get_attribute", "deform_bind", "deform_pose", "deform_unbind", "deform_last"]


class DeformParams(C.Structure):
    """hr_deform_params"""
    _fields_ = [("regenerate", C.c_int32), ("weight", C.c_int32), ("weld", C.c_int32), ("reserved", C.c_int32 * 5)]


class DeformRig(C.Structure):
    """hr_deform_rig"""
    _fields_ = [("morph_positions", f32p), ("morph_normals", f32p), ("joints", u32p), ("weights", f32p), ("n_morph", C.c_int32), ("n_joints", C.c_int32),
                ("reserved", C.c_int32 * 6)]


class DeformResult(C.Structure):
    """hr_deform_result"""
    _fields_ = [("vertices", C.c_uint64), ("triangles", C.c_uint64), ("rejected_vertices", C.c_uint64), ("kept_directions", C.c_uint64),
                ("regenerated", C.c_uint32), ("posed", C.c_uint32), ("mesh", MeshResult)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "mesh"}
        d["mesh"] = self.mesh.as_dict()
        return d


# every symbol include/hrcore_query.h declares (ray queries: the caller's rays traced on the device, with surface records).
# Resolved lazily like the AOV symbols
HR_QUERY_API_VERSION = 1
HR_QUERY_ANY_HIT = 1
HR_QUERY_INVALID_RAY = -2
HR_QUERY_SF_FRONT, HR_QUERY_SF_HAS_UV, HR_QUERY_SF_NON_OCCLUDER = 1, 2, 4
QUERY_SYMBOLS = ["query_api_version", "query_trace", "query_trace_host", "query_pixels", "query_last"]


class QuerySurface(C.Structure):
    """hr_query_surface"""
    _fields_ = [("geom", C.c_int32), ("material", C.c_int32), ("prim_in_geom", C.c_int32), ("flags", C.c_uint32), ("position", C.c_float * 3),
                ("normal", C.c_float * 3), ("geometric_normal", C.c_float * 3), ("uv", C.c_float * 2), ("reserved", C.c_float)]


SURFACE_DTYPE = np.dtype([("geom", np.int32), ("material", np.int32), ("prim_in_geom", np.int32), ("flags", np.uint32), ("position", np.float32, (3,)),
                          ("normal", np.float32, (3,)), ("geometric_normal", np.float32, (3,)), ("uv", np.float32, (2,)), ("reserved", np.float32)])


class QueryDesc(C.Structure):
    """hr_query_desc"""
    _fields_ = [("n", C.c_int32), ("flags", C.c_uint32), ("origins", C.c_void_p), ("directions", C.c_void_p), ("tmax", C.c_void_p), ("skip_prim", C.c_void_p),
                ("origin_stride", C.c_int32), ("direction_stride", C.c_int32), ("tmax_stride", C.c_int32), ("skip_stride", C.c_int32), ("tmin", C.c_float),
                ("reserved", C.c_uint32 * 3), ("hits", C.c_void_p), ("surfaces", C.c_void_p)]


class QueryResult(C.Structure):
    """hr_query_result"""
    _fields_ = [("rays", C.c_uint64), ("hits", C.c_uint64), ("invalid", C.c_uint64), ("reserved", C.c_uint64 * 5)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("rays", "hits", "invalid")}


# every symbol include/hrcore_motion.h declares (motion reprojection: the history gathered where a moved or deformed surface was).
# Resolved lazily like the AOV symbols
HR_MOTION_API_VERSION = 1
MOTION_SYMBOLS = ["motion_api_version", "motion_default_params", "motion_snapshot", "motion_trace", "motion_merge", "motion_vectors", "motion_vectors_readback",
                  "motion_readback", "motion_snapshot_readback", "motion_drop", "motion_info"]


class MotionTraceResult(C.Structure):
    """hr_motion_trace_result"""
    _fields_ = [("surface_pixels", C.c_uint64), ("sky_pixels", C.c_uint64), ("unmatched_pixels", C.c_uint64), ("reserved", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k in ("surface_pixels", "sky_pixels", "unmatched_pixels")}


class MotionResult(C.Structure):
    """hr_motion_result"""
    _fields_ = [("reused_pixels", C.c_uint64), ("rejected_pixels", C.c_uint64), ("history_samples", C.c_uint64), ("history_passes", C.c_uint32),
                ("passes", C.c_uint32), ("surface_pixels", C.c_uint64), ("sky_pixels", C.c_uint64), ("unmatched_pixels", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MotionInfo(C.Structure):
    """hr_motion_info_t"""
    _fields_ = [("snapshot", C.c_int32), ("traced", C.c_int32), ("triangles", C.c_uint32), ("meshes", C.c_uint32), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {"snapshot": bool(self.snapshot), "traced": bool(self.traced), "triangles": int(self.triangles), "meshes": int(self.meshes), "bytes": int(self.bytes)}


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


class GroupInfo(C.Structure):
    _fields_ = [("n_members", C.c_int32), ("device_ids", C.c_int32 * HR_GROUP_MAX_MEMBERS), ("owned_pixels", C.c_uint64 * HR_GROUP_MAX_MEMBERS)]


class EngineError(RuntimeError):
    pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, typ=f32p):
    return a.ctypes.data_as(typ) if a is not None else typ()


def _strided(a, comps):
    """(the array as the C-ABI can read it, its stride in bytes): a float32 V x comps array whose last axis is contiguous goes as it
    is, stride included; anything else is packed tight.  None -> (None, 0)."""
    if a is None:
        return None, 0
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != comps or a.strides[1] != 4 or a.strides[0] < 4 * comps:
        a = _f32(a).reshape(-1, comps)
    return a, a.strides[0]


class Engine:
    """Thin object wrapper over one hr_ctx (or ora_ctx)."""

    def __init__(self, lib, prefix, device_id=0, rank=0, world=1, tile_size=32, stream=None, flags=0, memory_budget=0):
        self._lib = lib
        self._p = prefix
        self._ctx = C.c_void_p()
        ver = getattr(lib, prefix + "abi_version", None)
        if ver is None:
            raise EngineError(f"{prefix}abi_version missing: the library predates this binding (ABI {HR_ABI_VERSION})")
        ver.restype = C.c_uint32
        if ver() != HR_ABI_VERSION:
            raise EngineError(f"{prefix}abi_version() = {ver()}, this binding was written against {HR_ABI_VERSION}: rebuild the library")
        desc = CtxDesc(device_id, rank, world, tile_size, stream, flags, int(memory_budget))
        rc = self._fn("ctx_create")(C.byref(desc), C.byref(self._ctx))
        if rc != HR_OK:
            self._ctx = C.c_void_p()
            raise EngineError(f"{prefix}ctx_create failed with status {rc} (no usable HIP device, a bad descriptor, or a malformed HR_TUNE: see stderr)")
        self.width = self.height = 0

    # -- plumbing
    def _fn(self, name):
        fn = getattr(self._lib, self._p + name)
        fn.restype = C.c_int
        return fn

    def _call(self, name, *args):
        rc = self._fn(name)(self._ctx, *args)
        if rc != HR_OK:
            le = getattr(self._lib, self._p + "last_error")
            le.restype = C.c_char_p
            msg = le(self._ctx)
            raise EngineError(f"{self._p}{name}: status {rc}: {msg.decode() if msg else ''}")

    def _feature_call(self, feature, name, *args):
        """_call for an entry point of an optional header (FEATURES).  Its symbols are resolved lazily, on the feature's first call: a
        library without them (the CPU oracle) still makes an Engine, and the feature's calls raise EngineError."""
        # (made here, not in __init__: the context group's class has an __init__ of its own that does not chain to Engine's)
        checked = self.__dict__.setdefault("_features_checked", set())
        if feature not in checked:
            symbols, want, words = FEATURES[feature]
            missing = [s for s in symbols if not hasattr(self._lib, self._p + s)]
            if missing:
                raise EngineError(f"this library has no {words} (lacks {[self._p + s for s in missing]})")
            ver = getattr(self._lib, f"{self._p}{feature}_api_version")
            ver.restype = C.c_uint32
            if ver() != want:
                raise EngineError(f"{self._p}{feature}_api_version() = {ver()}, this binding was written against {want}: rebuild the library")
            checked.add(feature)
        self._call(name, *args)

    def close(self):
        if self._ctx:
            self._fn("ctx_destroy")(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- frame
    def resize(self, w, h):
        self._call("frame_resize", C.c_int32(w), C.c_int32(h))
        self.width, self.height = w, h

    def bind_external_frame(self, device_ptr):
        self._call("frame_bind_external", C.c_void_p(device_ptr))

    def frame_device_ptr(self):
        p = C.c_void_p()
        self._call("frame_device_ptr", C.byref(p))
        return p.value

    def set_stream(self, stream):
        self._call("ctx_set_stream", C.c_void_p(stream))

    # -- geometry
    def add_mesh(self, positions, normals, indices, uvs=None, tangents=None, bitangents=None, colors=None,
                 mode=HR_TRIANGLES, world=None, front_face_cw=None, is_occluder=True, material_id=0):
        pos, nrm = _f32(positions).reshape(-1, 3), _f32(normals).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        opt = [None if a is None else _f32(a) for a in (uvs, tangents, bitangents, colors)]
        m = np.eye(4, dtype=np.float32) if world is None else _f32(world).reshape(4, 4)
        if front_face_cw is None:  # Mesh.cpp:86-91: determinant of the full 4x4
            front_face_cw = bool(np.linalg.det(m.astype(np.float64)) < 0)
        d = MeshDesc()
        d.positions, d.normals = _ptr(pos), _ptr(nrm)
        d.uvs, d.tangents, d.bitangents, d.colors = (_ptr(a) for a in opt)
        d.n_vertices = pos.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        # numpy holds the matrix as m[row][col]; the ABI wants column-major storage
        d.world_from_entity = (C.c_float * 16)(*m.T.reshape(-1))
        d.front_face_cw, d.is_occluder, d.material_id = int(front_face_cw), int(is_occluder), material_id
        gid = C.c_int32()
        self._call("geom_add", C.byref(d), C.byref(gid))
        self.__dict__.setdefault("_mesh_vertices", {})[gid.value] = d.n_vertices  # (mesh_attribute sizes its output by it)
        return gid.value

    def add_mesh_strided(self, buf, pos_off, nrm_off, uv_off, stride_floats, indices, mode=HR_TRIANGLES, world=None, is_occluder=True,
                         material_id=0):
        """One interleaved float buffer (n, stride_floats) holding positions / normals / uvs at the given float offsets."""
        buf = np.ascontiguousarray(buf, dtype=np.float32)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        d = MeshDesc()
        base = buf.ctypes.data
        d.positions = C.cast(base + 4 * pos_off, f32p)
        d.normals = C.cast(base + 4 * nrm_off, f32p)
        if uv_off is not None:
            d.uvs = C.cast(base + 4 * uv_off, f32p)
        d.position_stride = d.normal_stride = d.uv_stride = 4 * stride_floats
        d.n_vertices = buf.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        m = np.eye(4, dtype=np.float32) if world is None else _f32(world).reshape(4, 4)
        d.world_from_entity = (C.c_float * 16)(*m.T.reshape(-1))
        d.front_face_cw, d.is_occluder, d.material_id = int(np.linalg.det(m.astype(np.float64)) < 0), int(is_occluder), material_id
        gid = C.c_int32(-1)
        self._call("geom_add", C.byref(d), C.byref(gid))
        self.__dict__.setdefault("_mesh_vertices", {})[gid.value] = d.n_vertices
        return gid.value

    def remove_mesh(self, gid):
        self._call("geom_remove", C.c_int32(gid))
        for notes in ("_mesh_vertices", "_deform_rigs"):  # (what mesh_attribute and deform_pose remember of a mesh)
            self.__dict__.setdefault(notes, {}).pop(gid, None)

    def set_transform(self, gid, world):
        m = _f32(world).reshape(4, 4)
        self._call("geom_set_transform", C.c_int32(gid), (C.c_float * 16)(*m.T.reshape(-1)))

    def clear_scene(self):
        self._call("scene_clear")
        for notes in ("_mesh_vertices", "_deform_rigs"):
            self.__dict__.setdefault(notes, {}).clear()

    def set_scene_cache(self, path):
        self._call("scene_cache", None if not path else str(path).encode())

    def commit(self):
        self._call("scene_commit")

    def scene_info(self):
        s = SceneInfo()
        self._call("scene_get_info", C.byref(s))
        return s

    def tree_info(self):
        """hr_tree_info of the last commit that built the tree (include/hrcore_tree.h)"""
        t = TreeInfo()
        self._feature_call("tree", "scene_get_tree_info", C.byref(t))
        return t

    # -- textures / materials / lights
    def create_texture(self, pixels, wrap=HR_WRAP_REPEAT, filter=HR_FILTER_LINEAR):
        a = np.ascontiguousarray(pixels)
        if a.ndim == 2:
            a = a[:, :, None]
        dtype = HR_TEX_U8 if a.dtype == np.uint8 else HR_TEX_F32
        if dtype == HR_TEX_F32:
            a = _f32(a)
        d = TextureDesc(a.shape[1], a.shape[0], a.shape[2], dtype, wrap, wrap, filter)
        tid = C.c_int32()
        self._call("texture_create", C.byref(d), a.ctypes.data_as(C.c_void_p), C.byref(tid))
        return tid.value

    def destroy_texture(self, tid):
        self._call("texture_destroy", C.c_int32(tid))

    def set_material(self, material_id, material):
        self._call("material_set", C.c_int32(material_id), C.byref(material))

    def set_lights(self, lights):
        self._call("lights_set", C.byref(lights))

    # -- sample tables
    def set_sequences(self, seq_xy, aperture_xy):
        s, a = _f32(seq_xy), _f32(aperture_xy)
        assert s.shape == a.shape and s.ndim == 3 and s.shape[2] == 2
        self._call("sequences_set", _ptr(s), _ptr(a), C.c_int32(s.shape[0]), C.c_int32(s.shape[1]))

    def set_seq_offsets(self, offsets_xy):
        o = _f32(offsets_xy).reshape(-1, 2)
        self._call("seq_offsets_set", _ptr(o), C.c_int32(o.shape[0]))

    def qmc_generate(self, mode, sequence_index, count, radial=False):
        out = np.empty((count, 2), dtype=np.float32)
        self._call("qmc_generate", C.c_int32(mode), C.c_uint32(sequence_index), C.c_uint32(count),
                   C.c_int32(int(radial)), _ptr(out))
        return out

    def aperture_generate(self, bokeh, sequence_index, count):
        """One aperture table as PassGenerator.cpp:653-676 makes it: radialSobol or randomPolygonal(5 / 6 / 8 edges, seed = sequence)."""
        out = np.empty((count, 2), dtype=np.float32)
        self._call("aperture_generate", C.c_int32(bokeh), C.c_uint32(sequence_index), C.c_uint32(count), _ptr(out))
        return out

    def generate_sequences(self, sample_mode=HR_SAMPLE_SOBOL, bokeh=HR_BOKEH_CIRCULAR, length=32):
        self._call("sequences_generate", C.c_int32(sample_mode), C.c_int32(bokeh), C.c_int32(length))

    def generate_seq_offsets(self):
        self._call("seq_offsets_generate")

    def generate_multiscatter_lut(self, want_host=True):
        out = np.empty((128, 128), dtype=np.float32) if want_host else None
        tid = C.c_int32()
        self._call("multiscatter_lut_generate", _ptr(out), C.byref(tid))
        return out, tid.value

    # -- rendering
    def clear(self):
        self._call("clear")

    def render_pass(self, params):
        self._call("render_pass", C.byref(params))

    def set_interactive_blocks(self, coords_xy):
        """coords_xy: (ny, nx, 2) integer array in texture memory order, or None for the unshuffled list."""
        if coords_xy is None:
            self._call("interactive_blocks_set", None, C.c_int32(0), C.c_int32(0))
            return
        a = np.ascontiguousarray(coords_xy, dtype=np.int32)
        self._call("interactive_blocks_set", a.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(a.shape[1]), C.c_int32(a.shape[0]))

    def pass_batch(self, max_ray_depth):
        b = C.c_int32(0)
        self._call("frame_pass_batch", C.c_int32(max_ray_depth), C.byref(b))
        return int(b.value)

    def flush(self):
        self._call("flush")

    def stats(self):
        s = PassStats()
        self._call("get_stats", C.byref(s))
        return s

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since the last clear: HIP-event times (zero unless the context was created with
        HR_CTX_TIME_KERNELS), under "trace_clock" k_trace's time by the device clock (always), under "camera_packets" whether camera
        rays are traced as packets at the moment and the union factor the selector's last probe measured."""
        t = KernelTimes()
        self._call("get_kernel_times", C.byref(t))
        d = {n: (t.ms[i], t.launches[i]) for i, n in enumerate(HR_KERNEL_NAMES)}
        d["trace_clock"] = (t.trace_clock_ms, t.trace_clock_launches)
        d["camera_packets"] = (bool(t.camera_packets), t.packet_union, t.camera_packets)  # (camera rays as packets now?, the probe's union factor, passes per packet)
        return d

    def step_log(self, capacity=4096):
        """[(start_ms, trace_ms, passes_in_flight, passes_injected, group)] of the macro steps since the last clear (newest 4096), sorted by start."""
        recs = (StepRecord * capacity)()
        n = C.c_int32()
        self._call("get_step_log", recs, C.c_int32(capacity), C.byref(n))
        return [(r.start_ms, r.trace_ms, r.passes_in_flight, r.passes_injected, r.group) for r in recs[: n.value]]

    def synchronize(self):
        self._call("synchronize")

    def readback(self, copy=True):
        p = f32p()
        w, h = C.c_int32(), C.c_int32()
        self._call("readback", C.byref(p), C.byref(w), C.byref(h))
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4))
        return a.copy() if copy else a

    def display(self, params=None, fmt=HR_DISPLAY_RGBA8, with_passes=False):
        """Display resolve of the accumulation buffer -> numpy: uint8 [H, W, 4] (RGBA8) or float32 [H, W, 4];
        with_passes: (image, number of complete passes it shows)."""
        params = params if params is not None else display_params()
        dt, ch = (np.uint8, 4) if (fmt & 0xFF) == HR_DISPLAY_RGBA8 else (np.float32, 4)
        p = C.c_void_p()
        w, h = C.c_int32(), C.c_int32()
        shown = C.c_uint32()
        self._call("display_readback", C.byref(params), C.c_int32(fmt), C.byref(p), C.byref(w), C.byref(h), C.byref(shown))
        n = w.value * h.value * ch
        buf = (C.c_uint8 * n).from_address(p.value) if dt is np.uint8 else (C.c_float * n).from_address(p.value)
        img = np.frombuffer(buf, dtype=dt).reshape(h.value, w.value, ch).copy()
        return (img, int(shown.value)) if with_passes else img

    def passes_resolved(self):
        """Passes added to the accumulation buffer since the last clear, as enqueued so far (no synchronisation)."""
        n = C.c_uint64()
        self._call("frame_passes_resolved", C.byref(n))
        return int(n.value)

    # -- tile-shard exchange (device pointers for the HIP core, host pointers for the oracle)
    def packed_slots(self, rank, world):
        n = C.c_uint64()
        self._call("frame_packed_slots", C.c_int32(rank), C.c_int32(world), C.byref(n))
        return int(n.value)

    def pack_owned(self, out_ptr, stream=None):
        self._call("frame_pack_owned", C.c_void_p(int(out_ptr)), C.c_void_p(stream or 0))

    def unpack(self, src_rank, world, packed_ptr, full_ptr, stream=None):
        self._call("frame_unpack", C.c_int32(src_rank), C.c_int32(world), C.c_void_p(int(packed_ptr)), C.c_void_p(int(full_ptr)),
                   C.c_void_p(stream or 0))

    def display_device(self, device_ptr, params=None, fmt=HR_DISPLAY_RGBA8):
        """Asynchronous display resolve into device memory (e.g. a torch tensor or a GL-interop buffer)."""
        params = params if params is not None else display_params()
        self._call("display", C.byref(params), C.c_int32(fmt), C.c_void_p(int(device_ptr)), None)

    def readback_progressive(self, copy=True):
        """(buffer, complete passes in it) without completing the passes still in the pipeline.  copy=False returns a view
        of the context's pinned buffer (valid until the next readback)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        self._call("readback_progressive", C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4))
        return (a.copy() if copy else a), int(n.value)

    # -- AOVs (include/hrcore_aov.h)
    def set_aovs(self, mask):
        """Enable the AOV planes of `mask` (HR_AOV_SURFACE | HR_AOV_MOMENTS; 0 frees them).  Completes the passes in flight; a changed
        mask starts the planes at zero, so they hold the passes requested after this call."""
        self._feature_call("aov", "aov_enable", C.c_uint32(int(mask)))

    def aov_mask(self):
        m = C.c_uint32()
        self._feature_call("aov", "aov_mask", C.byref(m))
        return int(m.value)

    def aov_plane(self, plane):
        """(H x W x 4 float32 copy of one plane, passes summed into it); completes the enqueued passes first."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint64()
        self._feature_call("aov", "aov_readback", C.c_int32(plane), C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy(), int(n.value)

    def aovs(self):
        """The raw sums of every enabled plane: {"albedo", "normal_depth", "moments": H x W x 4 float32, "passes": n}
        (include/hrcore_aov.h; heatray_amd.aov.resolve turns them into means and a variance)."""
        mask = self.aov_mask()
        out = {}
        for plane, name in enumerate(AOV_PLANE_NAMES):
            if mask & (HR_AOV_MOMENTS if plane == HR_AOV_PLANE_MOMENTS else HR_AOV_SURFACE):
                out[name], out["passes"] = self.aov_plane(plane)
        return out

    def aov_to_device(self, plane, device_ptr, stream=None):
        """Asynchronous copy of one plane (W x H float4) into device memory, e.g. a torch tensor; ordered like display_device."""
        self._feature_call("aov", "aov_copy", C.c_int32(plane), C.c_void_p(int(device_ptr)), C.c_void_p(stream or 0))

    # -- denoiser (include/hrcore_denoise.h)
    def denoise(self, params=None, with_passes=False):
        """The denoised frame (H x W x 4 float32: rgb = mean colour, a = 1) of the passes rendered so far; needs both AOV masks enabled
        before the frame's first pass.  params: a DenoiseParams (heatray_amd.denoise.default_params()), None = the defaults."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        self._feature_call("denoise", "denoise_readback", C.byref(params) if params is not None else None, C.byref(p), C.byref(w), C.byref(h), C.byref(n))
        img = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
        return (img, int(n.value)) if with_passes else img

    def denoise_to_device(self, device_ptr, params=None, stream=None):
        """Asynchronous: the denoised frame (W x H float4) into device memory, e.g. a torch tensor; ordered like aov_to_device."""
        self._feature_call("denoise", "denoise", C.byref(params) if params is not None else None, C.c_void_p(int(device_ptr)), C.c_void_p(stream or 0), None)

    def denoise_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None):
        """Asynchronous display resolve of the denoised frame into device memory (like display_device)."""
        display = display if display is not None else display_params()
        self._feature_call("denoise", "denoise_display", C.byref(params) if params is not None else None, C.byref(display), C.c_int32(fmt),
                           C.c_void_p(int(device_ptr)), None)

    # -- denoiser with the spatial variance estimate (include/hrcore_denoise_spatial.h)
    def denoise_spatial(self, params=None, spatial=None, with_result=False):
        """denoise() with a spatial variance estimate for the pixels that have fewer than spatial.below samples (one-sample pixels no
        longer pass through unfiltered).  params: a DenoiseParams, spatial: a DenoiseSpatialParams
        (heatray_amd.denoise_spatial.default_params()); None = the defaults.  with_result: (image, the DenoiseSpatialResult as a dict)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DenoiseSpatialResult()
        self._feature_call("denoise_spatial", "denoise_spatial_readback", C.byref(params) if params is not None else None, C.byref(spatial) if spatial is not None else None,
                           C.byref(p), C.byref(w), C.byref(h), C.byref(n), C.byref(r))
        img = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
        return (img, r.as_dict()) if with_result else img

    def denoise_spatial_to_device(self, device_ptr, params=None, spatial=None, stream=None):
        """Asynchronous: denoise_spatial's image (W x H float4) into device memory; ordered like denoise_to_device."""
        self._feature_call("denoise_spatial", "denoise_spatial", C.byref(params) if params is not None else None, C.byref(spatial) if spatial is not None else None,
                           C.c_void_p(int(device_ptr)), C.c_void_p(stream or 0), None, None)

    def denoise_spatial_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None, spatial=None):
        """Asynchronous display resolve of denoise_spatial's image into device memory (like denoise_display)."""
        display = display if display is not None else display_params()
        self._feature_call("denoise_spatial", "denoise_spatial_display", C.byref(params) if params is not None else None, C.byref(spatial) if spatial is not None else None,
                           C.byref(display), C.c_int32(fmt), C.c_void_p(int(device_ptr)), None)

    def denoise_spatial_variance(self, params=None, spatial=None, with_result=False):
        """The luminance variance of every pixel after the estimate, before the first iteration (H x W float32); for inspection."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        r = DenoiseSpatialResult()
        self._feature_call("denoise_spatial", "denoise_spatial_variance", C.byref(params) if params is not None else None, C.byref(spatial) if spatial is not None else None,
                           _ptr(out), C.byref(r))
        return (out, r.as_dict()) if with_result else out

    # -- adaptive sampling (include/hrcore_adaptive.h)
    def set_sample_mask(self, mask):
        """Install a sample mask (H x W, row 0 = bottom like the frame, non-zero = the pixel is sampled by the passes requested from now
        on), or remove it with None.  Completes the enqueued passes first; clear() and resize() remove the mask too."""
        if mask is None:
            self._feature_call("adaptive", "sample_mask_set", None)
            return
        m = np.asarray(mask)
        m = np.ascontiguousarray(m if m.dtype == np.uint8 else m != 0, dtype=np.uint8)  # (bytes go as they are: any non-zero value counts)
        if m.shape != (self.height, self.width):
            raise ValueError(f"sample mask of shape {m.shape} for a frame of {(self.height, self.width)}")
        self._feature_call("adaptive", "sample_mask_set", m.ctypes.data_as(C.POINTER(C.c_uint8)))

    def sample_mask(self):
        """(the mask in force as H x W uint8 of 0 / 1, whether one is installed); all ones when there is none."""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        inst = C.c_int32()
        self._feature_call("adaptive", "sample_mask_get", out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(inst))
        return out, bool(inst.value)

    def adaptive_update(self, params=None, install=True):
        """Estimate every pixel's error from the frame and the MOMENTS plane (set_aovs(HR_AOV_MOMENTS) before the first pass), build the
        sample mask from it and, with install, put it in force.  params: an AdaptiveParams (heatray_amd.adaptive.default_params()),
        None = the defaults.  Returns the AdaptiveResult."""
        r = AdaptiveResult()
        self._feature_call("adaptive", "adaptive_update", C.byref(params) if params is not None else None, C.c_int32(int(bool(install))), C.byref(r))
        return r

    def adaptive_error_to_device(self, device_ptr, stream=None):
        """Asynchronous copy of the last adaptive_update's error map (W x H floats) into device memory; ordered like aov_to_device."""
        self._feature_call("adaptive", "adaptive_error_copy", C.c_void_p(int(device_ptr)), C.c_void_p(stream or 0))

    def adaptive_error(self):
        """The error map of the last adaptive_update as H x W float32 (+inf: fewer than min_samples samples)."""
        out = np.empty((self.height, self.width), dtype=np.float32)
        self._feature_call("adaptive", "adaptive_error_readback", _ptr(out))
        return out

    # -- history reprojection (include/hrcore_history.h)
    def history_capture(self, pass_params):
        """Turn the frame and the three AOV planes (set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS) before the first pass) into the history, as
        seen by the camera of `pass_params` (view_matrix, fov_tan, aspect_ratio).  The history survives clear()."""
        self._feature_call("history", "history_capture", C.byref(pass_params))

    def history_merge(self, pass_params, params=None):
        """Add the captured history to the frame and the planes of the view being rendered with `pass_params`; once per clear().  params: a
        HistoryParams (heatray_amd.history.default_params()), None = the defaults.  Returns the HistoryResult as a dict."""
        r = HistoryResult()
        self._feature_call("history", "history_merge", C.byref(pass_params), C.byref(params) if params is not None else None, C.byref(r))
        return r.as_dict()

    def history_drop(self):
        self._feature_call("history", "history_drop")

    def history_info(self):
        """(is there a captured history, the complete passes of the frame it was captured from)"""
        have, n = C.c_int32(), C.c_uint32()
        self._feature_call("history", "history_info", C.byref(have), C.byref(n))
        return bool(have.value), int(n.value)

    def history(self):
        """The captured history as 3 x H x W x 4 float32: H0 (mean colour, samples), H1 (mean second moment, coverage), H2 (unit normal,
        mean depth; +inf: sky)."""
        out = np.empty((3, self.height, self.width, 4), dtype=np.float32)
        self._feature_call("history", "history_readback", _ptr(out))
        return out

    # -- progressive merge and preview (include/hrcore_reproject.h)
    def reproject_merge(self, pass_params, params=None):
        """history_merge's progressive form: the sampled pixels no earlier call has examined since clear() take over their history; any
        number of calls per clear().  params: a HistoryParams, None = the defaults.  Returns the ReprojectResult as a dict."""
        r = ReprojectResult()
        self._feature_call("reproject", "reproject_merge", C.byref(pass_params), C.byref(params) if params is not None else None, C.byref(r))
        return r.as_dict()

    def reproject_examined(self):
        """The examined bits as H x W bool (row 0 = bottom like the frame)."""
        out = np.empty((self.height, self.width), dtype=np.uint8)
        self._feature_call("reproject", "reproject_examined_get", out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out.astype(bool)

    def reproject_preview(self, pass_params, params=None):
        """(H x W x 4 float32, the ReprojectPreviewResult as a dict): every sampled pixel's own mean and, in the pixels without a sample,
        the history behind a neighbour's guide (alpha 1) or 0 0 0 0.  Changes nothing."""
        p = f32p()
        w, h = C.c_int32(), C.c_int32()
        r = ReprojectPreviewResult()
        self._feature_call("reproject", "reproject_preview_readback", C.byref(pass_params), C.byref(params) if params is not None else None, C.byref(p), C.byref(w), C.byref(h),
                           C.byref(r))
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy(), r.as_dict()

    def reproject_preview_to_device(self, device_ptr, pass_params, params=None, stream=None):
        """Asynchronous: the preview (W x H float4) into device memory, e.g. a torch tensor; ordered like denoise_to_device."""
        self._feature_call("reproject", "reproject_preview", C.byref(pass_params), C.byref(params) if params is not None else None, C.c_void_p(int(device_ptr)),
                           C.c_void_p(stream or 0), None)

    # -- auto-exposure (include/hrcore_exposure.h)
    def exposure_meter(self, params=None, image=None):
        """Meters the frame (completing the enqueued passes), or `image`: the device pointer of a W x H float4 image in accumulation
        format, e.g. a torch tensor that denoise_to_device filled.  params: an ExposureParams (heatray_amd.exposure.default_params()),
        None = the defaults.  Returns the ExposureResult as a dict."""
        r = ExposureResult()
        self._feature_call("exposure", "exposure_meter", C.byref(params) if params is not None else None, C.c_void_p(int(image) if image else 0), C.byref(r))
        return r.as_dict()

    def exposure_display(self, device_ptr, display=None, fmt=HR_DISPLAY_RGBA8, params=None, image=None):
        """Asynchronous: meters like exposure_meter and resolves the metered image, at the metered scale, into device memory (like
        display_device; fmt may carry HR_DISPLAY_PROGRESSIVE).  Returns the passes shown (0 for an `image`)."""
        display = display if display is not None else display_params()
        shown = C.c_uint32()
        self._feature_call("exposure", "exposure_display", C.byref(params) if params is not None else None, C.byref(display), C.c_int32(fmt),
                           C.c_void_p(int(image) if image else 0), C.c_void_p(int(device_ptr)), C.byref(shown))
        return int(shown.value)

    def exposure_last(self, with_bins=False):
        """The last metering's ExposureResult as a dict (waits for it); with_bins: (the dict, its 256 bins as uint64)."""
        r = ExposureResult()
        bins = np.zeros(HR_EXPOSURE_BINS, np.uint64)
        self._feature_call("exposure", "exposure_last", C.byref(r), bins.ctypes.data_as(C.POINTER(C.c_uint64)) if with_bins else None)
        return (r.as_dict(), bins) if with_bins else r.as_dict()

    def exposure_reset(self):
        """Forgets the adaptation state: the next metering's scale is its target."""
        self._feature_call("exposure", "exposure_reset")

    # -- the convergence metric (include/hrcore_metric.h)
    def metric_compare(self, reference, image=None, params=None):
        """The relative L2 distance of the frame (completing the enqueued passes), or of `image`, from `reference`: device pointers of
        W x H float4 images in accumulation format, e.g. a torch tensor holding a kept copy of a converged frame.  params: a MetricParams
        (heatray_amd.metric.default_params()), None = the whole image.  Waits; returns the MetricResult as a dict (`value` is the metric)."""
        r = MetricResult()
        self._feature_call("metric", "metric_compare", C.byref(params) if params is not None else None, C.c_void_p(int(image) if image else 0),
                           C.c_void_p(int(reference) if reference else 0), C.byref(r))
        return r.as_dict()

    def metric_estimate(self, params=None):
        """The relative L2 distance the frame's sample moments predict between its luminance image and its own limit (HR_AOV_MOMENTS must
        be enabled before the frame's first pass).  Waits; returns the MetricResult as a dict."""
        r = MetricResult()
        self._feature_call("metric", "metric_estimate", C.byref(params) if params is not None else None, C.byref(r))
        return r.as_dict()

    def metric_last(self, with_bins=False):
        """The last measurement's MetricResult as a dict; with_bins: (the dict, the 256 bins of num, those of den, as uint64)."""
        r = MetricResult()
        num, den = np.zeros(HR_METRIC_BINS, np.uint64), np.zeros(HR_METRIC_BINS, np.uint64)
        u64p = C.POINTER(C.c_uint64)
        self._feature_call("metric", "metric_last", C.byref(r), num.ctypes.data_as(u64p) if with_bins else None, den.ctypes.data_as(u64p) if with_bins else None)
        return (r.as_dict(), num, den) if with_bins else r.as_dict()

    # -- firefly suppression (include/hrcore_despeckle.h)
    def despeckle(self, params=None, with_moments=False, with_result=False):
        """The despeckled frame (H x W x 4 float32, accumulation format like readback()) of the passes rendered so far; needs
        HR_AOV_MOMENTS enabled before the frame's first pass.  params: a DespeckleParams (heatray_amd.despeckle.default_params()),
        None = the defaults.  with_moments: and the despeckled MOMENTS plane; with_result: and the DespeckleResult as a dict; the image
        alone, or a tuple in that order."""
        p, m = f32p(), f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle_readback", C.byref(params) if params is not None else None, C.byref(p), C.byref(m) if with_moments else None,
                           C.byref(w), C.byref(h), C.byref(n), C.byref(r))
        out = [np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()]
        if with_moments:
            out.append(np.ctypeslib.as_array(m, shape=(h.value, w.value, 4)).copy())
        if with_result:
            out.append(r.as_dict())
        return out[0] if len(out) == 1 else tuple(out)

    def despeckle_to_device(self, out_ptr, moments_out_ptr=None, params=None, frame=None, moments=None, stream=None, with_result=False):
        """Asynchronous: the despeckled frame, and with moments_out_ptr the despeckled moments, (W x H float4 each) into device memory,
        e.g. torch tensors; ordered like denoise_to_device.  frame / moments: device pointers of a caller's pair instead of the
        context's own (both or neither).  with_result: waits and returns the DespeckleResult as a dict."""
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle", C.byref(params) if params is not None else None, C.c_void_p(int(frame) if frame else 0),
                           C.c_void_p(int(moments) if moments else 0), C.c_void_p(int(out_ptr) if out_ptr else 0),
                           C.c_void_p(int(moments_out_ptr) if moments_out_ptr else 0), C.c_void_p(stream or 0), None, C.byref(r) if with_result else None)
        return r.as_dict() if with_result else None

    def despeckle_denoise(self, params=None, dparams=None, spatial=False, sparams=None, with_result=False):
        """denoise() (spatial: denoise_spatial()) run from the despeckled frame and moments instead of the raw ones.  params: a
        DespeckleParams, dparams: a DenoiseParams, sparams: a DenoiseSpatialParams; None = the defaults.  with_result: (image, the
        DespeckleResult as a dict)."""
        p = f32p()
        w, h, n = C.c_int32(), C.c_int32(), C.c_uint32()
        r = DespeckleResult()
        self._feature_call("despeckle", "despeckle_denoise_readback", C.byref(params) if params is not None else None, C.byref(dparams) if dparams is not None else None,
                           C.c_int32(int(bool(spatial))), C.byref(sparams) if sparams is not None else None, C.byref(p), C.byref(w), C.byref(h), C.byref(n), C.byref(r))
        img = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
        return (img, r.as_dict()) if with_result else img

    def despeckle_denoise_to_device(self, device_ptr, params=None, dparams=None, spatial=False, sparams=None, stream=None):
        """Asynchronous: despeckle_denoise's image (W x H float4) into device memory; ordered like denoise_to_device."""
        self._feature_call("despeckle", "despeckle_denoise", C.byref(params) if params is not None else None, C.byref(dparams) if dparams is not None else None,
                           C.c_int32(int(bool(spatial))), C.byref(sparams) if sparams is not None else None, C.c_void_p(int(device_ptr) if device_ptr else 0),
                           C.c_void_p(stream or 0), None, None)

    # -- mesh preparation (include/hrcore_mesh.h)
    def prepare_mesh(self, positions, indices, uvs=None, normals=None, mode=HR_TRIANGLES, params=None, with_result=False):
        """(normals, tangents, bitangents) of a mesh that comes without them, V x 3 float32 each, None for what params.want does not ask
        for.  positions: V x 3, indices: the index list of `mode`; uvs (V x 2) are needed for tangents, normals (V x 3) for tangents
        without normals.  Strided arrays go as they are (the last axis contiguous).  params: a MeshParams
        (heatray_amd.meshprep.default_params()), None = the defaults.  with_result: and the MeshResult as a dict.  A side call: the scene
        and the frame are left alone."""
        def strided(a, comps):
            if a is None:
                return None, 0
            a = np.asarray(a)
            if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != comps or a.strides[1] != 4 or a.strides[0] < 4 * comps:
                a = _f32(a).reshape(-1, comps)
            return a, a.strides[0]
        pos, ps = strided(positions, 3)
        uv, us = strided(uvs, 2)
        nrm, ns = strided(normals, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        want = params.want if params is not None else HR_MESH_WANT_NORMALS
        d = MeshDesc()
        d.positions, d.uvs, d.normals = _ptr(pos), _ptr(uv), _ptr(nrm)
        d.position_stride, d.uv_stride, d.normal_stride = ps, us, ns
        d.n_vertices = pos.shape[0]
        d.indices, d.n_indices, d.mode = _ptr(idx, u32p), idx.size, mode
        out = [np.empty((pos.shape[0], 3), dtype=np.float32) if want & bit else None
               for bit in (HR_MESH_WANT_NORMALS, HR_MESH_WANT_TANGENTS, HR_MESH_WANT_TANGENTS)]
        r = MeshResult()
        self._feature_call("mesh", "mesh_prepare", C.byref(d), C.byref(params) if params is not None else None, *(_ptr(a) for a in out), C.byref(r))
        return (*out, r.as_dict()) if with_result else tuple(out)

    def add_mesh_prepared(self, positions, indices, uvs=None, **add_mesh_kwargs):
        """add_mesh for a mesh without normals: prepare_mesh makes them, and with uvs the tangents and bitangents too (weight ANGLE,
        weld on); the remaining keywords are add_mesh's (mode included).  Returns the geometry id."""
        p = MeshParams(HR_MESH_WEIGHT_ANGLE, 1, HR_MESH_WANT_NORMALS | (HR_MESH_WANT_TANGENTS if uvs is not None else 0))
        n, t, b = self.prepare_mesh(positions, indices, uvs=uvs, mode=add_mesh_kwargs.get("mode", HR_TRIANGLES), params=p)
        return self.add_mesh(positions, n, indices, uvs=uvs, tangents=t, bitangents=b, **add_mesh_kwargs)

    def mesh_last(self):
        """The last successful prepare_mesh's MeshResult as a dict."""
        r = MeshResult()
        self._feature_call("mesh", "mesh_last", C.byref(r))
        return r.as_dict()

    # -- deformable meshes (include/hrcore_deform.h)
    def update_mesh(self, gid, positions, normals=None, uvs=None, tangents=None, bitangents=None, colors=None, params=None, with_result=False):
        """New vertex data for mesh `gid`, in its device block: positions (V x 3) and whichever other attributes are given; None leaves
        an attribute as it is.  Strided arrays go as they are (the last axis contiguous).  params: a DeformParams
        (heatray_amd.deform.params(regenerate=...)), None = the defaults.  The scene needs a commit afterwards: it refits.
        with_result: the DeformResult as a dict."""
        arrays = [_strided(a, comps) for a, comps in zip((positions, normals, uvs, tangents, bitangents, colors), (3, 3, 2, 3, 3, 3))]
        d = MeshDesc()
        d.positions, d.normals, d.uvs, d.tangents, d.bitangents, d.colors = (_ptr(a) for a, _ in arrays)
        d.position_stride, d.normal_stride, d.uv_stride, d.tangent_stride, d.bitangent_stride, d.color_stride = (s for _, s in arrays)
        d.n_vertices = arrays[0][0].shape[0]
        r = DeformResult()
        self._feature_call("deform", "geom_update", C.c_int32(gid), C.byref(d), C.byref(params) if params is not None else None, C.byref(r))
        self.__dict__.setdefault("_mesh_vertices", {})[gid] = d.n_vertices
        return r.as_dict() if with_result else None

    def mesh_attribute(self, gid, attribute, n_vertices=None):
        """Attribute HR_GEOM_* of mesh `gid` as the device block holds it: V x 3 float32 (V x 2 for uvs).  The C call does not say how
        many vertices the mesh has: add_mesh, add_mesh_strided and update_mesh remember it; n_vertices names it for any other mesh."""
        V = n_vertices if n_vertices is not None else self.__dict__.setdefault("_mesh_vertices", {}).get(gid)
        if V is None:
            # (an id this engine does not know: the library names the cause, if the call fails; else the count is missing)
            self._feature_call("deform", "geom_get_attribute", C.c_int32(gid), C.c_int32(attribute), f32p())
            raise ValueError(f"mesh_attribute: give n_vertices for mesh {gid}")
        out = np.empty((V, 2 if attribute == HR_GEOM_UVS else 3), dtype=np.float32)
        self._feature_call("deform", "geom_get_attribute", C.c_int32(gid), C.c_int32(attribute), _ptr(out))
        return out

    def deform_bind(self, gid, morph_positions=None, morph_normals=None, joints=None, weights=None, n_joints=None):
        """The mesh as it stands becomes the rest pose of a rig: morph_positions / morph_normals K x V x 3 deltas, joints V x 4 indices
        and weights V x 4; n_joints: the rig's joint count, None = the highest index named + 1.  A second bind replaces the first."""
        mp = None if morph_positions is None else _f32(morph_positions)
        mn = None if morph_normals is None else _f32(morph_normals)
        j = None if joints is None else np.ascontiguousarray(joints, dtype=np.uint32)
        w = None if weights is None else _f32(weights)
        rig = DeformRig()
        rig.morph_positions, rig.morph_normals, rig.joints, rig.weights = _ptr(mp), _ptr(mn), _ptr(j, u32p), _ptr(w)
        rig.n_morph = 0 if mp is None else mp.reshape(-1, *mp.shape[-2:]).shape[0]
        if n_joints is None:
            n_joints = 0 if j is None or not j.size else int(j.max()) + 1
        rig.n_joints = n_joints
        self._feature_call("deform", "deform_bind", C.c_int32(gid), C.byref(rig))
        self.__dict__.setdefault("_deform_rigs", {})[gid] = (rig.n_morph, rig.n_joints)

    def deform_pose(self, gid, morph_weights=None, joint_matrices=None, params=None, with_result=False):
        """Pose the bound mesh `gid` on the device: morph_weights K floats, joint_matrices J x 4 x 4 (numpy's m[row][col]; the ABI's
        column-major order is made here).  params as update_mesh's.  The scene needs a commit afterwards."""
        mw = None if morph_weights is None else _f32(morph_weights).reshape(-1)
        jm = None if joint_matrices is None else _f32(np.transpose(_f32(joint_matrices).reshape(-1, 4, 4), (0, 2, 1)))
        K, J = self.__dict__.setdefault("_deform_rigs", {}).get(gid, (0, 0))  # (the library reads as many as the rig has)
        if (mw is not None and mw.size < K) or (jm is not None and jm.shape[0] < J):
            raise ValueError(f"deform_pose: mesh {gid} is bound to {K} morphs and {J} joints")
        r = DeformResult()
        self._feature_call("deform", "deform_pose", C.c_int32(gid), _ptr(mw), _ptr(jm), C.byref(params) if params is not None else None, C.byref(r))
        return r.as_dict() if with_result else None

    def deform_unbind(self, gid):
        self._feature_call("deform", "deform_unbind", C.c_int32(gid))
        self.__dict__.setdefault("_deform_rigs", {}).pop(gid, None)

    def deform_last(self):
        """The last successful update_mesh's or deform_pose's DeformResult as a dict."""
        r = DeformResult()
        self._feature_call("deform", "deform_last", C.byref(r))
        return r.as_dict()

    # -- ray queries (include/hrcore_query.h)
    @staticmethod
    def _query_desc(n, origins, dirs, tmax, skip, strides, any_hit, tmin, hits, surfaces):
        d = QueryDesc()
        d.n, d.flags = int(n), HR_QUERY_ANY_HIT if any_hit else 0
        d.origins, d.directions, d.tmax, d.skip_prim = origins or None, dirs or None, tmax or None, skip or None
        d.origin_stride, d.direction_stride, d.tmax_stride, d.skip_stride = (int(v) for v in strides)
        d.tmin = -1.0 if tmin is None else float(tmin)
        d.hits, d.surfaces = hits or None, surfaces or None
        return d

    def query(self, origins, dirs, tmax=None, skip_prim=None, any_hit=False, surface=False, tmin=None):
        """Trace the caller's rays (numpy, n x 3 each) against the committed scene: the hits (HIT_DTYPE, as debug_trace reports them;
        prim = HR_QUERY_INVALID_RAY for a ray that is not finite), or (hits, surfaces) with surface=True (SURFACE_DTYPE: which mesh, which
        triangle of it, where on it).  any_hit: an occlusion query (prim 0 blocked / -1 clear).  tmin=None: the scene's ray epsilon.
        A float32 array whose rows are strided (a view into an interleaved buffer) goes to the library as it is, stride included."""
        def rows(a, comps, dtype):
            a = np.asarray(a)
            shaped = a.ndim == 2 and a.shape[1] == comps and a.strides[1] == 4 if comps > 1 else a.ndim == 1
            if a.dtype != dtype or not shaped or a.strides[0] % 4 or a.strides[0] < comps * 4:
                a = np.ascontiguousarray(a, dtype=dtype).reshape((-1, comps) if comps > 1 else (-1,))
            return a
        o, d = rows(origins, 3, np.float32), rows(dirs, 3, np.float32)
        n = o.shape[0]
        if d.shape[0] != n:
            raise ValueError(f"query: {n} origins but {d.shape[0]} directions")
        tm = None if tmax is None else rows(tmax, 1, np.float32)
        sk = None if skip_prim is None else rows(skip_prim, 1, np.int32)
        for name, a in (("tmax", tm), ("skip_prim", sk)):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"query: {n} rays but {a.shape[0]} entries of {name}")
        hits = np.empty(n, dtype=HIT_DTYPE)
        surf = np.empty(n, dtype=SURFACE_DTYPE) if surface else None
        addr = lambda a: None if a is None else a.ctypes.data
        stride = lambda a: 0 if a is None or a.shape[0] < 2 else a.strides[0]
        desc = self._query_desc(n, addr(o), addr(d), addr(tm), addr(sk), (stride(o), stride(d), stride(tm), stride(sk)), any_hit, tmin, addr(hits), addr(surf))
        nothing = C.c_float()
        if n == 0:  # (an empty array's address may be null, which the library would call "null origins"; with n = 0 nothing is read or written)
            desc.origins = desc.directions = desc.hits = C.addressof(nothing)
        self._feature_call("query", "query_trace_host", C.byref(desc))
        return (hits, surf) if surface else hits

    def query_to_device(self, n, origins_ptr, dirs_ptr, hits_ptr=None, surfaces_ptr=None, tmax_ptr=None, skip_ptr=None, strides=(0, 0, 0, 0),
                        any_hit=False, tmin=None, stream=None):
        """Asynchronous: n rays in device memory (raw device pointers, e.g. torch tensors' data_ptr(); strides in bytes for origins,
        directions, tmax, skip_prim, 0 = tight) -> n hr_hit at hits_ptr and / or n hr_query_surface at surfaces_ptr, on `stream` (None: the
        context's).  Ordered behind the last commit; the next commit waits for it (include/hrcore_query.h, ORDERING)."""
        desc = self._query_desc(n, origins_ptr, dirs_ptr, tmax_ptr, skip_ptr, strides, any_hit, tmin, hits_ptr, surfaces_ptr)
        self._feature_call("query", "query_trace", C.byref(desc), C.c_void_p(stream or 0))

    def query_pixels(self, pass_params, xy, surface=True, rays=False):
        """The camera rays through the points xy (n x 2, pixel units: the centre of pixel x, y is x + 0.5, y + 0.5, row 0 at the bottom) of
        the frame, traced with tmin = 0: hits, then surfaces with surface=True, then the rays (n x 6: o, d) with rays=True.  hits["t"] is
        the focus_distance that focuses the lens on what the pixel shows."""
        p = _f32(xy).reshape(-1, 2)
        n = p.shape[0]
        hits = np.empty(n, dtype=HIT_DTYPE)
        surf = np.empty(n, dtype=SURFACE_DTYPE) if surface else None
        ro = np.empty((n, 6), dtype=np.float32) if rays else None
        self._feature_call("query", "query_pixels", C.byref(pass_params), C.c_int32(n), _ptr(p) if n else C.pointer(C.c_float()),
                           hits.ctypes.data_as(C.c_void_p) if n else C.byref(Hit()), None if surf is None else surf.ctypes.data_as(C.c_void_p),
                           None if ro is None else _ptr(ro))
        out = (hits,) + ((surf,) if surface else ()) + ((ro,) if rays else ())
        return out if len(out) > 1 else hits

    def query_last(self):
        """{"rays", "hits", "invalid"} of the last successful query; completes the queries in flight."""
        r = QueryResult()
        self._feature_call("query", "query_last", C.byref(r))
        return r.as_dict()

    # -- motion reprojection (include/hrcore_motion.h)
    def motion_snapshot(self):
        """Remember the committed pose: every triangle's world-space (p0, e1, e2) and the table of meshes.  Survives clear(), commits
        and resize(); a second snapshot replaces it."""
        self._feature_call("motion", "motion_snapshot")

    def motion_trace(self, pass_params):
        """One pixel-centre ray per pixel of the camera of `pass_params` against the committed scene: where was each pixel's surface
        point in the snapshot's pose?  Writes the motion planes (motion_planes()); returns {"surface_pixels", "sky_pixels",
        "unmatched_pixels"}."""
        r = MotionTraceResult()
        self._feature_call("motion", "motion_trace", C.byref(pass_params), C.byref(r))
        return r.as_dict()

    def motion_merge(self, pass_params, params=None):
        """history_merge, gathering where the snapshot says each pixel's surface point was; once per clear(), instead of history_merge or
        reproject_merge.  params: a HistoryParams (heatray_amd.motion.default_params()), None = those defaults.  Returns the
        MotionResult as a dict: history_merge's keys and motion_trace's."""
        r = MotionResult()
        self._feature_call("motion", "motion_merge", C.byref(pass_params), C.byref(params) if params is not None else None, C.byref(r))
        return r.as_dict()

    def motion_planes(self):
        """The motion planes of the last trace as 2 x H x W x 4 float32: Mv0 (the surface point in the previous pose, 1 / the hit point,
        -1 / 0 0 0 0 for sky), Mv1 (the previous pose's geometric normal, depth; +inf: sky)."""
        out = np.empty((2, self.height, self.width, 4), dtype=np.float32)
        self._feature_call("motion", "motion_readback", _ptr(out))
        return out

    def motion_vectors(self, old_pass_params=None):
        """The screen-space motion of every pixel as H x W x 4 float32: (dx, dy, the point's depth in the old camera, Mv0.w), from the
        planes of the last trace.  old_pass_params None: the captured history's camera."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._feature_call("motion", "motion_vectors_readback", C.byref(old_pass_params) if old_pass_params is not None else None, _ptr(out))
        return out

    def motion_vectors_to_device(self, device_ptr, old_pass_params=None, stream=None):
        """Asynchronous: the same image into device memory (a raw pointer, 16-byte aligned) on `stream` (None: the context's)."""
        self._feature_call("motion", "motion_vectors", C.byref(old_pass_params) if old_pass_params is not None else None, C.c_void_p(device_ptr),
                           C.c_void_p(stream or 0))

    def motion_snapshot_triangles(self):
        """The snapshot as T x 12 float32 in submission order: p0.xyz e1.xyz e2.xyz 0 0 0."""
        out = np.empty((self.motion_info()["triangles"], 12), dtype=np.float32)
        self._feature_call("motion", "motion_snapshot_readback", _ptr(out) if out.size else C.pointer(C.c_float()))
        return out

    def motion_drop(self):
        self._feature_call("motion", "motion_drop")

    def motion_info(self):
        """{"snapshot", "traced", "triangles", "meshes", "bytes"}"""
        r = MotionInfo()
        self._feature_call("motion", "motion_info", C.byref(r))
        return r.as_dict()

    def debug_trace(self, origins, dirs, tmax=None, skip_prim=None, any_hit=False):
        o, d = _f32(origins).reshape(-1, 3), _f32(dirs).reshape(-1, 3)
        n = o.shape[0]
        tm = None if tmax is None else _f32(tmax).reshape(-1)
        sk = None if skip_prim is None else np.ascontiguousarray(skip_prim, dtype=np.int32).reshape(-1)
        out = np.empty(n, dtype=HIT_DTYPE)
        self._call("debug_trace", C.c_int32(n), _ptr(o), _ptr(d), _ptr(tm), _ptr(sk, i32p), C.c_int32(int(any_hit)),
                   out.ctypes.data_as(C.POINTER(Hit)))
        return out


class GroupEngine(Engine):
    """An Engine whose handle is a context group (include/hrcore_group.h): member i renders the tiles t % n == i on
    device_ids[i]; every Engine call works on it, plus the group's own two."""

    def __init__(self, lib, device_ids=None, tile_size=32, stream=None, flags=0, memory_budget=0):
        self._lib = lib
        self._p = "hr_"
        self._ctx = C.c_void_p()
        self.width = self.height = 0
        missing = [s for s in GROUP_SYMBOLS if not hasattr(lib, "hr_" + s)]
        if missing:
            raise EngineError(f"the loaded libhrcore has no context groups (lacks {missing}): rebuild it")
        for fn, want in (("abi_version", HR_ABI_VERSION), ("group_api_version", HR_GROUP_API_VERSION)):
            f = getattr(lib, "hr_" + fn)
            f.restype = C.c_uint32
            if f() != want:
                raise EngineError(f"hr_{fn}() = {f()}, this binding was written against {want}: rebuild the library")
        ids = None if device_ids is None else (C.c_int32 * max(1, len(device_ids)))(*device_ids)
        n = 0 if device_ids is None else len(device_ids)
        desc = CtxDesc(0, 0, 1, tile_size, stream, flags, int(memory_budget))
        rc = self._fn("ctx_create_group")(C.byref(desc), ids, C.c_int32(n), C.byref(self._ctx))
        if rc != HR_OK:
            self._ctx = C.c_void_p()
            raise EngineError(f"hr_ctx_create_group({list(device_ids) if device_ids is not None else 'every device'}) failed with status {rc} "
                              "(no usable HIP device, a bad device id or more than 16 members?)")

    def group_info(self):
        """{"n_members", "device_ids", "owned_pixels"} of the group."""
        g = GroupInfo()
        self._call("group_get_info", C.byref(g))
        n = g.n_members
        return {"n_members": n, "device_ids": list(g.device_ids[:n]), "owned_pixels": list(g.owned_pixels[:n])}

    def member_stats(self, member, kernel_times=False):
        """PassStats of one member (completes its passes first); with kernel_times, (stats, KernelTimes)."""
        s, t = PassStats(), KernelTimes()
        self._call("group_member_stats", C.c_int32(member), C.byref(s), C.byref(t) if kernel_times else None)
        return (s, t) if kernel_times else s
