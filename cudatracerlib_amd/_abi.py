"""ctypes mirror of include/ctl_trace.h (the C-ABI drop-in boundary).

Layouts are byte-identical to the reference structures named in the header;
``tests/test_abi.py`` checks every size against the C side.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CTL_LIB overrides the library path (the sanitizer build, tools/san_tests.sh).
LIB_PATH = os.environ.get("CTL_LIB") or os.path.join(_HERE, "_lib", "libctl_trace.so")

# CTL_ABI_VERSION of the include/ctl_trace.h these bindings mirror; load()
# refuses a library that reports another (mismatched struct layouts).
ABI_VERSION = 4
CTL_OK = 0
CTL_SCENE_HALF_HOST_QUIRK = 1
CTL_SCENE_BINARY_BVH = 2
CTL_SCENE_WIDE_QUANT = 4
CTL_DEFAULT_SPLIT_ALPHA = 0.1875   # include/ctl_trace.h
CTL_XMSH_MATERIAL_RECORD_SIZE = 148
CTL_COMM_ID_BYTES = 128
CTL_BVH_BINNED, CTL_BVH_SBVH = 0, 1
(CTL_ARRAY_TRI_DATA, CTL_ARRAY_WOOP, CTL_ARRAY_BVH_NODES, CTL_ARRAY_SCENE_BVH, CTL_ARRAY_MESH_BOXES, CTL_ARRAY_RAY_EPS,
 CTL_ARRAY_SAMPLES_1D, CTL_ARRAY_SAMPLES_2D) = range(8)
CTL_BSDF_DIFFUSE = 1
CTL_EDIFFUSE_REFLECTION = 0x2
CTL_EGLOSSY_REFLECTION = 0x8
CTL_EGLOSSY_TRANSMISSION = 0x10
CTL_BSDF_ROUGHDIELECTRIC = 5
CTL_BSDF_DIELECTRIC, CTL_BSDF_THINDIELECTRIC, CTL_BSDF_CONDUCTOR, CTL_BSDF_ROUGHCONDUCTOR, CTL_BSDF_PLASTIC = 3, 4, 6, 7, 8
CTL_ENULL, CTL_EDELTA_REFLECTION, CTL_EDELTA_TRANSMISSION = 0x1, 0x20, 0x40
CTL_EALL = 0x1ff
CTL_MEASURE_SOLID_ANGLE, CTL_MEASURE_DISCRETE = 1, 4
CTL_BSDF_OP_SAMPLE, CTL_BSDF_OP_F, CTL_BSDF_OP_PDF = 0, 1, 2
# ctl_math_eval / ctl_host_math_eval function ids
CTL_MATH_FUNCTIONS = ["sin", "cos", "tan", "acos", "atan", "atan2", "exp", "log", "log2", "pow", "erf", "erfinv", "div",
                      "sqrt", "rcp", "half_ieee", "half_quirk", "half_round_int", "u16_trunc", "normal_encode16",
                      "normal_decode16"]
CTL_MICROFACET_BECKMANN = 0
CTL_MICROFACET_GGX = 1
CTL_TEX_POINT, CTL_TEX_BILINEAR, CTL_TEX_EWA, CTL_TEX_TRILINEAR = 0, 1, 2, 3
CTL_WRAP_REPEAT, CTL_WRAP_CLAMP, CTL_WRAP_MIRROR, CTL_WRAP_BLACK = 0, 1, 2, 3
CTL_MAX_NUM_LIGHTS = 16
CTL_PT_MEGAKERNEL = 1
CTL_PT_WAVEFRONT = 2
CTL_PT_RENDER_AHEAD = 4
# ctl_scene_update dirty groups (DynamicScene streams)
CTL_DIRTY_TRI_DATA, CTL_DIRTY_WOOP, CTL_DIRTY_BVH, CTL_DIRTY_TRI_INDICES = 1, 2, 4, 8
CTL_DIRTY_MATERIALS, CTL_DIRTY_MESHES, CTL_DIRTY_NODES, CTL_DIRTY_LIGHTS = 16, 32, 64, 128
CTL_DIRTY_TEXTURES, CTL_DIRTY_ENV, CTL_DIRTY_VOLUMES, CTL_DIRTY_ALL = 256, 512, 1024, 2047
# ctl_scene_read arrays
(CTL_ARRAY_TRI_DATA, CTL_ARRAY_WOOP, CTL_ARRAY_BVH_NODES, CTL_ARRAY_SCENE_BVH, CTL_ARRAY_MESH_BOXES, CTL_ARRAY_RAY_EPS,
 CTL_ARRAY_SAMPLES_1D, CTL_ARRAY_SAMPLES_2D, CTL_ARRAY_NODE_XF, CTL_ARRAY_NODE_INV_XF, CTL_ARRAY_LIGHTS,
 CTL_ARRAY_LIGHT_TRIS, CTL_ARRAY_LIGHT_CDF, CTL_ARRAY_SCENE_BOX, CTL_ARRAY_ENV, CTL_ARRAY_WIDE_BVH,
 CTL_ARRAY_SCENE_WIDE_BVH, CTL_ARRAY_MESH_WIDE_BASE, CTL_ARRAY_CULL_BOUND, CTL_ARRAY_MESHES,
 CTL_ARRAY_TRI_INDICES) = range(21)


class BVHNode(C.Structure):          # BVHNodeData, 64 B
    _fields_ = [("v", C.c_float * 16)]


class WoopTri(C.Structure):          # TriIntersectorData, 48 B
    _fields_ = [("v", C.c_float * 12)]


class TriangleData(C.Structure):     # TriangleData (EXT_TRI), 32 B
    _fields_ = [("w", C.c_uint32 * 8)]


class KernelMesh(C.Structure):       # KernelMesh, 20 B
    _fields_ = [("triangle_offset", C.c_uint32), ("bvh_node_offset", C.c_uint32),
                ("bvh_triangle_offset", C.c_uint32), ("bvh_indices_offset", C.c_uint32),
                ("std_material_offset", C.c_uint32)]


class Node(C.Structure):             # Node, 24 B
    _fields_ = [("mesh_index", C.c_uint32), ("material_offset", C.c_uint32),
                ("instanced_material", C.c_uint32), ("lights", C.c_uint32 * 2), ("num_lights", C.c_uint32)]


class Float4x4(C.Structure):
    _fields_ = [("m", C.c_float * 16)]


class Ray(C.Structure):              # traversalRay, 32 B
    _fields_ = [("o", C.c_float * 3), ("tmin", C.c_float), ("d", C.c_float * 3), ("tmax", C.c_float)]


class Hit(C.Structure):              # traversalResult, 16 B
    _fields_ = [("dist", C.c_float), ("node_idx", C.c_int32), ("tri_idx", C.c_int32), ("bary", C.c_int32)]


class Pixel(C.Structure):            # PixelData, 28 B
    _fields_ = [("rgb", C.c_float * 3), ("rgb_splat", C.c_float * 3), ("weight_sum", C.c_float)]


class Material(C.Structure):        # 80 B
    _fields_ = [("bsdf_type", C.c_uint32), ("combined_type", C.c_uint32), ("two_sided", C.c_uint32),
                ("node_light_index", C.c_uint32), ("reflectance", C.c_float * 3), ("texture", C.c_uint32),
                ("transmittance", C.c_float * 3), ("distribution", C.c_uint32), ("eta", C.c_float),
                ("inv_eta", C.c_float), ("alpha_u", C.c_float), ("alpha_v", C.c_float),
                ("sample_visible", C.c_uint32), ("alpha_state", C.c_uint32), ("alpha_texture", C.c_uint32),
                ("alpha_threshold", C.c_float)]


class MaterialExt(C.Structure):     # ctl_material_ext, 64 B
    _fields_ = [("eta", C.c_float * 3), ("k", C.c_float * 3), ("specular", C.c_float * 3), ("fdr_int", C.c_float),
                ("inv_eta2", C.c_float), ("specular_sampling_weight", C.c_float), ("nonlinear", C.c_uint32),
                ("pad", C.c_uint32 * 3)]


class BsdfQuery(C.Structure):       # ctl_bsdf_query, 56 B
    _fields_ = [("material", C.c_uint32), ("op", C.c_uint32), ("type_mask", C.c_uint32), ("measure", C.c_uint32),
                ("wi", C.c_float * 3), ("wo", C.c_float * 3), ("sample", C.c_float * 2), ("uv", C.c_float * 2)]


class BsdfResult(C.Structure):      # ctl_bsdf_result, 32 B
    _fields_ = [("value", C.c_float * 3), ("pdf", C.c_float), ("wo", C.c_float * 3), ("sampled_type", C.c_uint32)]


class Texture(C.Structure):
    _fields_ = [("mapping", C.c_float * 6), ("set_id", C.c_uint32), ("scale", C.c_float * 3),
                ("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32), ("filter", C.c_uint32),
                ("wrap", C.c_uint32), ("offsets", C.c_uint32 * 16), ("weight_lut", C.c_float * 64)]


class LightTri(C.Structure):         # ShapeSet::triData, 64 B
    _fields_ = [("p", (C.c_float * 3) * 3), ("n", C.c_float * 3), ("area", C.c_float),
                ("i_dat", C.c_uint32), ("t_dat", C.c_uint32), ("pad", C.c_uint32)]


class Light(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("orthogonal", C.c_uint32), ("tri_first", C.c_uint32),
                ("tri_count", C.c_uint32), ("cdf_first", C.c_uint32), ("sum_area", C.c_float),
                ("node_idx", C.c_uint32), ("kind", C.c_uint32), ("pad", C.c_uint32 * 2)]


CTL_LIGHT_DIFFUSE = 0
CTL_LIGHT_INFINITE = 1
CTL_LIGHT_POINT, CTL_LIGHT_SPOT, CTL_LIGHT_DISTANT = 2, 3, 4


class LightParams(C.Structure):      # ctl_light_params: a delta light's light_tris slot, 64 B
    _fields_ = [("pos", C.c_float * 3), ("s", C.c_float * 3), ("t", C.c_float * 3), ("n", C.c_float * 3),
                ("cos_beam_width", C.c_float), ("cos_cutoff_angle", C.c_float), ("cutoff_angle", C.c_float),
                ("inv_transition_width", C.c_float)]


class LightQuery(C.Structure):       # ctl_light_query, 36 B
    _fields_ = [("light", C.c_uint32), ("ref", C.c_float * 3), ("ref_n", C.c_float * 3), ("sample", C.c_float * 2)]


class LightResult(C.Structure):      # ctl_light_result, 64 B
    _fields_ = [("value", C.c_float * 3), ("pdf", C.c_float), ("d", C.c_float * 3), ("dist", C.c_float),
                ("p", C.c_float * 3), ("measure", C.c_uint32), ("n", C.c_float * 3), ("pad", C.c_uint32)]


class EnvLight(C.Structure):          # ctl_env_light (InfiniteLight), 112 B
    _fields_ = [("texture", C.c_uint32), ("scale", C.c_float * 3), ("size", C.c_float * 2),
                ("pixel_size", C.c_float * 2), ("normalization", C.c_float), ("scene_center", C.c_float * 3),
                ("scene_radius", C.c_float), ("cdf_cols", C.c_uint32), ("cdf_rows", C.c_uint32),
                ("row_weights", C.c_uint32), ("world", (C.c_float * 3) * 3), ("pad", C.c_uint32 * 3)]


class Camera(C.Structure):
    _fields_ = [("to_world", Float4x4), ("sample_to_camera", Float4x4), ("dx", C.c_float * 3),
                ("dy", C.c_float * 3), ("inv_resolution", C.c_float * 2), ("width", C.c_uint32),
                ("height", C.c_uint32)]


class AnimVertex(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("normal", C.c_float * 3), ("bone_indices", C.c_uint64),
                ("bone_weights", C.c_uint64)]


class AnimMesh(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("vertex_first", C.c_uint32), ("vertex_count", C.c_uint32),
                ("tri_first", C.c_uint32), ("tri_count", C.c_uint32), ("max_bone", C.c_uint32)]


CTL_MAX_NUM_VOLUMES = 16
CTL_VOLUME_HOMOGENEOUS = 1
CTL_PHASE_ISOTROPIC, CTL_PHASE_HG = 0, 1
(CTL_MEDIUM_INTERSECT, CTL_MEDIUM_TRANSMITTANCE, CTL_MEDIUM_SAMPLE_DISTANCE, CTL_MEDIUM_PHASE_EVAL,
 CTL_MEDIUM_PHASE_SAMPLE) = range(5)


class Volume(C.Structure):           # ctl_volume (HomogeneousVolumeDensity + its phase function), 176 B
    _fields_ = [("kind", C.c_uint32), ("phase", C.c_uint32), ("phase_g", C.c_float), ("sig_a", C.c_float * 3),
                ("sig_s", C.c_float * 3), ("le", C.c_float * 3), ("volume_to_world", Float4x4),
                ("world_to_volume", Float4x4)]


class MediumQuery(C.Structure):      # ctl_medium_query, 56 B
    _fields_ = [("op", C.c_uint32), ("ori", C.c_float * 3), ("dir", C.c_float * 3), ("wo", C.c_float * 3),
                ("tmin", C.c_float), ("tmax", C.c_float), ("u", C.c_float * 2)]


class MediumResult(C.Structure):     # ctl_medium_result, 96 B
    _fields_ = [("hit", C.c_uint32), ("t0", C.c_float), ("t1", C.c_float), ("t", C.c_float), ("p", C.c_float * 3),
                ("transmittance", C.c_float * 3), ("sigma_a", C.c_float * 3), ("sigma_s", C.c_float * 3),
                ("pdf_success", C.c_float), ("pdf_success_rev", C.c_float), ("pdf_failure", C.c_float),
                ("value", C.c_float), ("pdf", C.c_float), ("wo_out", C.c_float * 3)]


CTL_SENSOR_SPHERICAL, CTL_SENSOR_PERSPECTIVE, CTL_SENSOR_THINLENS, CTL_SENSOR_ORTHOGRAPHIC, CTL_SENSOR_TELECENTRIC = 1, 2, 3, 4, 5


class Sensor(C.Structure):           # ctl_sensor (which of the reference's five sensors ctl_camera describes), 32 B
    _fields_ = [("type", C.c_uint32), ("aperture_radius", C.c_float), ("focus_distance", C.c_float),
                ("screen_scale", C.c_float * 2), ("pad", C.c_uint32 * 3)]


class SensorQuery(C.Structure):      # ctl_sensor_query, 20 B
    _fields_ = [("pixel_sample", C.c_float * 2), ("aperture_sample", C.c_float * 2), ("differential", C.c_uint32)]


class SensorResult(C.Structure):     # ctl_sensor_result, 80 B
    _fields_ = [("o", C.c_float * 3), ("d", C.c_float * 3), ("ox", C.c_float * 3), ("dx", C.c_float * 3),
                ("oy", C.c_float * 3), ("dy", C.c_float * 3), ("has_differentials", C.c_uint32), ("pad", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("tri_data", C.POINTER(TriangleData)), ("n_tri_data", C.c_uint64),
        ("woop_tris", C.POINTER(WoopTri)), ("n_woop_tris", C.c_uint64),
        ("bvh_nodes", C.POINTER(BVHNode)), ("n_bvh_nodes", C.c_uint64),
        ("tri_indices", C.POINTER(C.c_uint32)), ("n_tri_indices", C.c_uint64),
        ("materials", C.POINTER(Material)), ("n_materials", C.c_uint32),
        ("meshes", C.POINTER(KernelMesh)), ("n_meshes", C.c_uint32),
        ("nodes", C.POINTER(Node)), ("n_nodes", C.c_uint32),
        ("scene_bvh_nodes", C.POINTER(BVHNode)), ("n_scene_bvh_nodes", C.c_uint32),
        ("scene_start_node", C.c_int32),
        ("node_xf", C.POINTER(Float4x4)), ("node_inv_xf", C.POINTER(Float4x4)),
        ("lights", C.POINTER(Light)), ("n_lights", C.c_uint32),
        ("light_tris", C.POINTER(LightTri)), ("n_light_tris", C.c_uint32),
        ("light_tri_cdf", C.POINTER(C.c_float)), ("n_light_tri_cdf", C.c_uint32),
        ("light_cdf", C.c_float * CTL_MAX_NUM_LIGHTS),
        ("textures", C.POINTER(Texture)), ("n_textures", C.c_uint32),
        ("tex_data", C.POINTER(C.c_uint32)), ("n_tex_data", C.c_uint64),
        ("env_map_index", C.c_uint32),
        ("env", C.POINTER(EnvLight)),
        ("env_data", C.POINTER(C.c_float)), ("n_env_data", C.c_uint64),
        ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
        ("ray_eps", C.c_float),
        ("camera", Camera),
        ("flags", C.c_uint32),
        ("mesh_boxes", C.POINTER(C.c_float)),
        ("anim_vertices", C.POINTER(AnimVertex)), ("n_anim_vertices", C.c_uint32),
        ("anim_triangles", C.POINTER(C.c_uint32)), ("n_anim_triangles", C.c_uint32),
        ("anim_meshes", C.POINTER(AnimMesh)), ("n_anim_meshes", C.c_uint32),
        ("volumes", C.POINTER(Volume)), ("n_volumes", C.c_uint32),
        ("sensor", C.POINTER(Sensor)),
        ("materials_ext", C.POINTER(MaterialExt)),
    ]


class PixelVariance(C.Structure):    # PixelVarianceInfo, 44 B
    _fields_ = [("prev_I", C.c_float * 3), ("half_buffer", C.c_float * 3), ("iterations_done", C.c_int32),
                ("weight", C.c_float), ("sum_x", C.c_float), ("sum_x2", C.c_float), ("num_samples_var", C.c_int32)]


class BlockInfo(C.Structure):        # VarianceBlockSampler::TmpBlockInfo, 20 B
    _fields_ = [("block_var_i", C.c_float), ("num_pixels_var", C.c_uint32), ("block_e_i", C.c_float),
                ("block_e_i2", C.c_float), ("num_pixels_e", C.c_uint32)]


CTL_BST_UNIFORM, CTL_BST_VARIANCE = 0, 1   # ctl_block_sampler_create types

# ctl_image_filter.type (Filter.h TYPE_FUNC ids, NonLocalMeansFilter) and .flags
CTL_FILTER_BOX, CTL_FILTER_GAUSSIAN, CTL_FILTER_MITCHELL, CTL_FILTER_LANCZOS, CTL_FILTER_TRIANGLE = 1, 2, 3, 4, 5
CTL_FILTER_NLM = 16
CTL_NLM_DIRECT = 1 << 0


class ImageFilter(C.Structure):      # ctl_image_filter, 36 B
    _fields_ = [("type", C.c_uint32), ("x_width", C.c_float), ("y_width", C.c_float), ("a", C.c_float),
                ("b", C.c_float), ("k", C.c_float), ("sigma2_scale", C.c_float), ("update_periodicity", C.c_uint32),
                ("flags", C.c_uint32)]


class Tonemap(C.Structure):          # ctl_tonemap (ToneMapPostProcess), 8 B
    _fields_ = [("key", C.c_float), ("burn", C.c_float)]


class LuminanceInfo(C.Structure):    # ctl_luminance_info (Image::ComputeLuminanceInfo), 28 B
    _fields_ = [("avg_color", C.c_float * 3), ("min_lum", C.c_float), ("max_lum", C.c_float), ("avg_lum", C.c_float),
                ("avg_log_lum", C.c_float)]


class PTParams(C.Structure):
    _fields_ = [("direct", C.c_int32), ("max_path_length", C.c_int32), ("rr_start_depth", C.c_int32),
                ("shadow_any_hit", C.c_int32), ("tile_size", C.c_uint32), ("num_ranks", C.c_uint32),
                ("rank", C.c_uint32), ("flags", C.c_uint32)]


class PrimParams(C.Structure):
    _fields_ = [("draw_mode", C.c_int32), ("max_path_length", C.c_int32), ("near_depth", C.c_float),
                ("far_depth", C.c_float), ("flags", C.c_uint32)]


# PathTrace_DrawMode (PrimTracer.h:7-9)
PRIM_DRAW_MODES = ["linear_depth", "D3D_depth", "v_absdot_n_geo", "v_dot_n_geo", "v_dot_n_shade", "n_geo_colored",
                   "n_shade_colored", "uv", "bary_coords", "first_Le", "first_f", "first_f_direct",
                   "first_non_delta_Le", "first_non_delta_f", "first_non_delta_f_direct"]


CTL_WPT_SHADOW_ANY_HIT = 1 << 0   # ctl_wpt_params.flags


class WptParams(C.Structure):
    _fields_ = [("direct", C.c_int32), ("max_path_length", C.c_int32), ("rr_start_depth", C.c_int32),
                ("passes_done", C.c_uint32), ("flags", C.c_uint32)]


# Every symbol include/ctl_trace.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SYMBOLS = [
    ("ctl_abi_version", C.c_int32, []),
    ("ctl_create", _vp, [C.c_int32]),
    ("ctl_destroy", None, [_vp]),
    ("ctl_last_error", C.c_char_p, [_vp]),
    ("ctl_scene_upload", C.c_int32, [_vp, C.POINTER(SceneDesc)]),
    ("ctl_scene_update", C.c_int32, [_vp, C.POINTER(SceneDesc), C.c_uint32, _vp]),
    ("ctl_scene_set_transform", C.c_int32, [_vp, C.c_uint32, _vp, _vp]),
    ("ctl_sampler_generate", C.c_int32, [_vp, C.c_uint64, _vp]),
    ("ctl_sampler_upload", C.c_int32, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, _vp]),
    ("ctl_intersect", C.c_int32, [_vp, C.c_int64, _vp, _vp, C.c_int32, _vp]),
    ("ctl_occluded", C.c_int32, [_vp, C.c_int64, _vp, _vp, C.c_int32, _vp]),
    ("ctl_render_pass", C.c_int32, [_vp, C.POINTER(PTParams), _vp, _vp]),
    ("ctl_render_passes", C.c_int32, [_vp, C.POINTER(PTParams), C.c_uint64, C.c_uint32, _vp, _vp]),
    ("ctl_wpt_render_pass", C.c_int32, [_vp, C.POINTER(WptParams), _vp, _vp]),
    ("ctl_prim_pass", C.c_int32, [_vp, C.POINTER(PrimParams), _vp, _vp, _vp]),
    ("ctl_rays_traced", C.c_uint64, [_vp]),
    ("ctl_tail_handovers", C.c_int32, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("ctl_reset_rays", C.c_int32, [_vp, _vp]),
    ("ctl_sync", C.c_int32, [_vp, _vp]),
    ("ctl_scene_stack_bound", C.c_int32, [_vp]),
    ("ctl_host_bvh_stack_bound", C.c_int32, [_vp, C.c_uint64, C.c_int32, _vp]),
    ("ctl_host_wide_trees", C.c_int32, [C.POINTER(SceneDesc), _vp, C.c_uint64, C.POINTER(C.c_uint64), _vp, _vp,
                                        C.c_uint64, C.POINTER(C.c_uint64)]),
    ("ctl_intersect_stats", C.c_int32, [_vp, C.c_int64, _vp, _vp, C.c_int32, C.POINTER(C.c_uint64), _vp]),
    ("ctl_render_pass_stats", C.c_int32, [_vp, C.POINTER(PTParams), _vp, C.POINTER(C.c_uint64), _vp]),
    ("ctl_last_pass_ms", C.c_int32, [_vp, C.POINTER(C.c_float)]),
    ("ctl_camera_rays", C.c_int32, [_vp, C.POINTER(PTParams), _vp, C.c_int64, C.POINTER(C.c_int64), _vp]),
    ("ctl_comm_unique_id", C.c_int32, [_vp]),
    ("ctl_comm_init_rank", C.c_int32, [C.POINTER(_vp), C.c_int32, _vp, C.c_int32, C.c_int32]),
    ("ctl_comm_init_all", C.c_int32, [C.POINTER(_vp), C.c_int32, _vp]),
    ("ctl_comm_destroy", C.c_int32, [_vp]),
    ("ctl_fb_reduce", C.c_int32, [_vp, _vp, _vp, _vp, C.c_uint64, C.c_int32, _vp]),
    ("ctl_fb_reduce_all", C.c_int32, [_vp, _vp, _vp, _vp, C.c_int32, C.c_uint64, C.c_int32, _vp]),
    ("ctl_image_resolve", C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, _vp, _vp]),
    ("ctl_variance_add_pass", C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, _vp, _vp, _vp]),
    ("ctl_variance_stats", C.c_int32, [_vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp]),
    ("ctl_woop_set", None, [_vp, _vp, _vp, C.POINTER(WoopTri)]),
    ("ctl_host_sampler_tables", C.c_int32, [C.c_uint64, C.c_uint32, C.c_uint32, _vp, _vp]),
    ("ctl_host_scene_create", _vp, []),
    ("ctl_host_scene_destroy", None, [_vp]),
    ("ctl_host_scene_add_mesh", C.c_int32, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp,
                                            C.POINTER(Material), C.c_uint32]),
    ("ctl_host_scene_set_mesh_material_ext", C.c_int32, [_vp, C.c_uint32, C.POINTER(MaterialExt), C.c_uint32]),
    ("ctl_host_bsdf_eval", C.c_int32, [C.POINTER(SceneDesc), C.c_uint64, _vp, _vp]),
    ("ctl_bsdf_eval", C.c_int32, [_vp, C.c_uint64, _vp, _vp, _vp]),
    ("ctl_host_math_eval", C.c_int32, [C.c_uint32, C.c_uint64, _vp, _vp, _vp]),
    ("ctl_math_eval", C.c_int32, [_vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp]),
    ("ctl_host_scene_add_texture", C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    ("ctl_host_scene_add_node", C.c_int32, [_vp, C.c_uint32, _vp]),
    ("ctl_host_scene_add_area_light", C.c_int32, [_vp, C.c_uint32, C.c_uint32, _vp]),
    ("ctl_host_scene_add_point_light", C.c_int32, [_vp, _vp, _vp]),
    ("ctl_host_scene_add_spot_light", C.c_int32, [_vp, _vp, _vp, _vp, C.c_float, C.c_float]),
    ("ctl_host_scene_add_distant_light", C.c_int32, [_vp, _vp, _vp, C.c_float]),
    ("ctl_host_light_eval", C.c_int32, [C.POINTER(SceneDesc), _vp, C.c_int64, _vp]),
    ("ctl_host_scene_add_homogeneous_volume", C.c_int32, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, C.c_float]),
    ("ctl_host_medium_eval", C.c_int32, [C.POINTER(SceneDesc), _vp, C.c_int64, _vp]),
    ("ctl_medium_eval", C.c_int32, [_vp, _vp, C.c_int64, _vp, _vp]),
    ("ctl_light_eval", C.c_int32, [_vp, _vp, C.c_int64, _vp, _vp]),
    ("ctl_host_scene_set_sensor", C.c_int32, [_vp, C.c_uint32, C.c_float, C.c_float, _vp]),
    ("ctl_host_scene_sensor_state", C.c_int32, [_vp, C.POINTER(Camera), C.POINTER(Sensor)]),
    ("ctl_sensor_eval", C.c_int32, [_vp, _vp, C.c_int64, _vp, _vp]),
    ("ctl_host_sensor_eval", C.c_int32, [C.POINTER(SceneDesc), _vp, C.c_int64, _vp]),
    ("ctl_host_scene_set_camera", C.c_int32, [_vp, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float,
                                              C.c_uint32, C.c_uint32]),
    ("ctl_host_scene_set_flags", C.c_int32, [_vp, C.c_uint32]),
    ("ctl_host_scene_set_environment", C.c_int32, [_vp, C.c_uint32, _vp]),
    ("ctl_host_scene_set_environment_transform", C.c_int32, [_vp, _vp]),
    ("ctl_host_scene_set_bvh_params", C.c_int32, [_vp, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("ctl_host_scene_set_bvh_builder", C.c_int32, [_vp, C.c_uint32, C.c_float]),
    ("ctl_host_scene_compile", C.c_int32, [_vp, C.c_uint32, C.POINTER(SceneDesc)]),
    ("ctl_host_scene_add_animated_mesh", C.c_int32, [_vp, C.POINTER(AnimVertex), C.c_uint32, _vp, C.c_uint32, _vp,
                                                     _vp, C.POINTER(Material), C.c_uint32]),
    ("ctl_scene_animate", C.c_int32, [_vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_float, _vp]),
    ("ctl_scene_read", C.c_int32, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, _vp]),
    ("ctl_scene_array_size", C.c_int32, [_vp, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("ctl_scene_rebuild_mesh", C.c_int32, [_vp, C.c_uint32, _vp, C.c_uint32, _vp]),
    ("ctl_last_rebuild_ms", C.c_int32, [_vp, C.POINTER(C.c_float * 2)]),
    ("ctl_host_scene_add_xmsh", C.c_int32, [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint32]),
    ("ctl_host_scene_write_xmsh", C.c_int32, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("ctl_host_scene_write_animated_xmsh", C.c_int32, [_vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("ctl_host_scene_set_animated_bvh", C.c_int32, [_vp, C.c_uint32]),
    ("ctl_host_scene_add_animation", C.c_int32, [_vp, C.c_uint32, C.c_char_p, C.c_uint32, _vp, C.c_uint32,
                                                 C.c_uint32]),
    ("ctl_host_scene_animation_count", C.c_int32, [_vp, C.c_uint32]),
    ("ctl_host_scene_animation_info", C.c_int32, [_vp, C.c_uint32, C.c_uint32, _vp, C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("ctl_host_scene_animation_frames", C.c_int32, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64]),
    ("ctl_animation_frame_index", C.c_int32, [C.c_uint32, C.c_uint32, C.c_float, C.POINTER(C.c_uint32),
                                              C.POINTER(C.c_float)]),
    ("ctl_scene_set_animation", C.c_int32, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint32]),
    ("ctl_scene_animate_frame", C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _vp]),
    ("ctl_scene_animate_time", C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _vp]),
    ("ctl_host_last_error", C.c_char_p, []),
    ("ctl_host_scene_generate", C.c_int32, [_vp, C.c_int32, C.c_double, C.c_uint32, C.c_uint32]),
    ("ctl_render_pass_blocks", C.c_int32, [_vp, C.POINTER(PTParams), _vp, C.c_uint32, _vp, _vp]),
    ("ctl_block_stats", C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]),
    ("ctl_block_sampler_create", _vp, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("ctl_block_sampler_destroy", None, [_vp]),
    ("ctl_block_sampler_start_new_rendering", C.c_int32, [_vp]),
    ("ctl_block_sampler_set_fractions", C.c_int32, [_vp, C.c_uint32, C.c_uint32]),
    ("ctl_block_sampler_set_user_weight", C.c_int32, [_vp, C.c_uint32, C.c_uint32, C.c_float]),
    ("ctl_block_sampler_blocks", C.c_int32, [_vp, _vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("ctl_block_sampler_tile_samples", C.c_int32, [_vp, _vp]),
    ("ctl_block_sampler_add_pass", C.c_int32, [_vp, _vp, C.c_uint32]),
    ("ctl_block_sampler_weights", C.c_int32, [_vp, _vp]),
    ("ctl_block_sampler_passes_done", C.c_int32, [_vp, _vp]),
    ("ctl_image_pipeline", C.c_int32, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32,
                                       C.POINTER(ImageFilter), C.POINTER(Tonemap), _vp, _vp, _vp]),
    ("ctl_image_luminance", C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.POINTER(LuminanceInfo), _vp]),
    ("ctl_filter_evaluate", C.c_int32, [C.POINTER(ImageFilter), C.c_float, C.c_float, C.POINTER(C.c_float)]),
    ("ctl_rgbe_encode", C.c_int32, [C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
    ("ctl_rgbe_decode", C.c_int32, [C.c_uint32, C.POINTER(C.c_float)]),
    ("ctl_tonemap_constants", C.c_int32, [C.POINTER(Tonemap), C.c_float, C.c_float, C.POINTER(C.c_float),
                                          C.POINTER(C.c_float)]),
]

# Added within CTL_ABI_VERSION 4: a library built from an earlier commit (a CTL_LIB base of the
# tools/ab_*.sh comparisons) loads without them, and calling one there raises AttributeError.
OPTIONAL = {"ctl_tail_handovers"}

_lib = None


def load(path=LIB_PATH):
    """Load libctl_trace.so and bind every declared symbol.  Raises loudly if
    the HIP extension was not built: there is no fallback path."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libctl_trace.so not built ({path}); run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if name in OPTIONAL:
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    v = lib.ctl_abi_version()
    if v != ABI_VERSION:
        raise RuntimeError(f"{path} reports CTL_ABI_VERSION {v}, these bindings are for {ABI_VERSION}: rebuild it")
    if path == LIB_PATH:
        _lib = lib
    return lib
