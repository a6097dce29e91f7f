"""ctypes mirrors of the POD structs declared in include/yuki_hip.h.

The same layouts are accepted by the parity oracle (oracle/oracle_api.h), so the
tests build one description of a scene / camera / sampler and hand it to both.
"""
import ctypes as C

import numpy as np

f32p = C.POINTER(C.c_float)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)


class MeshDesc(C.Structure):
    _fields_ = [("has_normals", C.c_uint8), ("has_uvs", C.c_uint8), ("swaps_handedness", C.c_uint8), ("pad", C.c_uint8)]


class SphereDesc(C.Structure):
    _fields_ = [
        ("object_to_world", C.c_float * 16),
        ("world_to_object", C.c_float * 16),
        ("radius", C.c_float),
        ("material", C.c_int32),
    ]


class MaterialDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("a", C.c_float * 3), ("b", C.c_float * 3), ("c", C.c_float), ("flags", C.c_uint32), ("a_texture", C.c_uint32)]


class TextureDesc(C.Structure):
    """textures/image_texture.rs:49-56: row-major RGB f32, row 0 = top row of the file."""

    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("rgb", C.POINTER(C.c_float))]


class LightDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32),
        ("p", C.c_float * 3),
        ("i", C.c_float * 3),
        ("cos_total_width", C.c_float),
        ("cos_falloff_start", C.c_float),
        ("world_to_light", C.c_float * 16),
        ("sample_to_world", C.c_float * 16),
        ("sample_to_world_inv", C.c_float * 16),
        ("area", C.c_float),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_uint32),
        ("points", f32p),
        ("normals", f32p),
        ("uvs", f32p),
        ("n_triangles", C.c_uint32),
        ("indices", u32p),
        ("tri_mesh", u32p),
        ("tri_material", i32p),
        ("tri_area_light", i32p),
        ("n_meshes", C.c_uint32),
        ("meshes", C.POINTER(MeshDesc)),
        ("n_spheres", C.c_uint32),
        ("spheres", C.POINTER(SphereDesc)),
        ("n_materials", C.c_uint32),
        ("materials", C.POINTER(MaterialDesc)),
        ("n_lights", C.c_uint32),
        ("lights", C.POINTER(LightDesc)),
        ("background", C.c_float * 3),
        ("split_method", C.c_uint32),
        ("max_shapes_in_node", C.c_uint32),
        ("shape_order", u32p),
        ("n_textures", C.c_uint32),
        ("textures", C.POINTER(TextureDesc)),
    ]


class CameraMatrices(C.Structure):
    """`Camera` of camera.rs:19-22: two Transforms (matrix + inverse each)."""

    _fields_ = [
        ("camera_to_world", C.c_float * 16),
        ("camera_to_world_inv", C.c_float * 16),
        ("raster_to_camera", C.c_float * 16),
        ("raster_to_camera_inv", C.c_float * 16),
    ]


class CameraParams(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("target", C.c_float * 3),
        ("up", C.c_float * 3),
        ("fov_axis", C.c_uint32),
        ("fov_degrees", C.c_float),
        ("res_x", C.c_uint16),
        ("res_y", C.c_uint16),
    ]


class SamplerDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("jitter", C.c_uint32), ("seed", C.c_uint64)]


class IntegratorDesc(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("max_depth", C.c_uint32), ("has_clamp", C.c_uint32), ("indirect_clamp", C.c_float)]


class ToneMapDesc(C.Structure):
    """yk_tone_map_desc: ToneMapType (app/renderpasses/tonemap.rs:40-44) with its params."""

    _fields_ = [("kind", C.c_uint32), ("exposure", C.c_float), ("channel", C.c_uint32), ("has_bounds", C.c_uint32), ("bounds", C.c_float * 2)]


class ExposureDesc(C.Structure):
    """yk_exposure_desc: the meter's cuts (units of 1/65536), bias, clamp, adaptation rates and window (csrc/yk_exposure.h)."""

    _fields_ = [
        ("low_cut", C.c_uint32),
        ("high_cut", C.c_uint32),
        ("ev_bias", C.c_float),
        ("min_ev", C.c_float),
        ("max_ev", C.c_float),
        ("adapt_up", C.c_float),
        ("adapt_down", C.c_float),
        ("window", C.c_uint16 * 4),
    ]


class ExposureState(C.Structure):
    """yk_exposure_state: the meter's 32-byte record."""

    _fields_ = [
        ("exposure", C.c_float),
        ("log2_adapted", C.c_float),
        ("log2_metered", C.c_float),
        ("frames", C.c_uint32),
        ("counted", C.c_uint32),
        ("skipped", C.c_uint32),
        ("below", C.c_uint32),
        ("above", C.c_uint32),
    ]


class PresentDesc(C.Structure):
    """yk_present_desc: the window, the encode (yk_present_encode) and the frame format (yk_present_format)."""

    _fields_ = [("window_x", C.c_uint16), ("window_y", C.c_uint16), ("encode", C.c_uint32), ("format", C.c_uint32)]


class PresentRect(C.Structure):
    """yk_present_rect: the target rectangle of ScaleOutput::draw in top-down window coordinates."""

    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32)]


class DenoiseDesc(C.Structure):
    """yk_denoise_desc: the à-trous iterations and the three stops (csrc/yk_denoise.h)."""

    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float)]


class UpsampleDesc(C.Structure):
    """yk_upsample_desc: the factor and the normal and plane stops of the guided upsample (csrc/yk_upsample.h)."""

    _fields_ = [("s", C.c_uint32), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float)]


class TemporalDesc(C.Structure):
    """yk_temporal_desc: the plane and normal tests of reproject and blend's history clamp (csrc/yk_temporal.h)."""

    _fields_ = [("plane_tolerance", C.c_float), ("normal_cos_min", C.c_float), ("max_history", C.c_float)]


class VarianceDesc(C.Structure):
    """yk_variance_desc: the à-trous iterations, the variance-scaled colour stop and the two geometric stops
    (csrc/yk_variance.h)."""

    _fields_ = [("iterations", C.c_uint32), ("sigma_variance", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("epsilon", C.c_float), ("spatial_scale", C.c_float)]


class RectifyDesc(C.Structure):
    """yk_rectify_desc: the window and the box of the history rectification (csrc/yk_rectify.h)."""

    _fields_ = [("radius", C.c_uint32), ("gamma", C.c_float)]


DESPECKLE_REPAIR = 1  # yk_despeckle_desc::flags
DESPECKLE_UNTOUCHED, DESPECKLE_CLAMPED, DESPECKLE_REPAIRED = 0, 1, 2  # the values of yk_despeckle's mask


class DespeckleDesc(C.Structure):
    """yk_despeckle_desc: the window, the rank and the gain of the despeckle pass (csrc/yk_despeckle.h)."""

    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("min_taps", C.c_uint32), ("flags", C.c_uint32), ("gain", C.c_float), ("floor", C.c_float)]


class AdaptiveDesc(C.Structure):
    """yk_adaptive_desc: the adaptive sampler's rule (csrc/yk_adaptive.h)."""

    _fields_ = [("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("round_passes", C.c_uint32), ("max_rounds", C.c_uint32), ("dilate", C.c_uint32), ("threshold", C.c_float), ("epsilon", C.c_float)]


class AdaptiveInfo(C.Structure):
    """yk_adaptive_info: what yk_render_adaptive_device did."""

    _fields_ = [("rounds", C.c_uint32), ("converged", C.c_uint32), ("first_pixels", C.c_uint32), ("last_pixels", C.c_uint32), ("samples", C.c_uint64), ("rays", C.c_uint64), ("shadow_rays", C.c_uint64)]


class IntegratorRay(C.Structure):
    """yk_integrator_ray: IntegratorRay (integrators/mod.rs:76-80), the ray and its yk_ray_type."""

    _fields_ = [("o", C.c_float * 3), ("d", C.c_float * 3), ("t_max", C.c_float), ("ray_type", C.c_uint32)]


class Tile(C.Structure):
    _fields_ = [("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16), ("y1", C.c_uint16)]


class BvhNode(C.Structure):
    _fields_ = [
        ("bmin", C.c_float * 3),
        ("bmax", C.c_float * 3),
        ("a", C.c_uint32),
        ("count", C.c_uint16),
        ("axis", C.c_uint8),
        ("is_leaf", C.c_uint8),
    ]


class SceneLayoutInfo(C.Structure):
    """yk_scene_layout_info: who laid a scene's traversal records out ("scene_layout"), and what the kernels get with them."""

    _fields_ = [
        ("layout", C.c_uint32),
        ("reason", C.c_uint32),
        ("seconds_upload", C.c_double),
        ("seconds_layout", C.c_double),
        ("tree_fetched", C.c_uint32),
        ("root_ref", C.c_uint32),
        ("n_top", C.c_uint32),
        ("n_top_any", C.c_uint32),
        ("wide", C.c_uint32),
        ("wide_auto", C.c_uint32),
    ]


class SceneUpdateInfo(C.Structure):
    """yk_scene_update_info: how a scene's last update in place ran (yk_scene_update / yk_scene_update_device)."""

    _fields_ = [
        ("n_updates", C.c_uint32),
        ("route", C.c_uint32),
        ("reason", C.c_uint32),
        ("n_levels", C.c_uint32),
        ("plan_bytes", C.c_uint64),
        ("seconds_check", C.c_double),
        ("seconds_boxes", C.c_double),
        ("seconds_records", C.c_double),
        ("seconds_total", C.c_double),
    ]


class TraceStats(C.Structure):
    _fields_ = [
        ("closest_rays", C.c_uint64),
        ("closest_node_tests", C.c_uint64),
        ("closest_shape_tests", C.c_uint64),
        ("shadow_rays", C.c_uint64),
        ("shadow_node_tests", C.c_uint64),
        ("shadow_shape_tests", C.c_uint64),
    ]


BVH_NODE_DTYPE = np.dtype(
    [("bmin", "<f4", 3), ("bmax", "<f4", 3), ("a", "<u4"), ("count", "<u2"), ("axis", "u1"), ("is_leaf", "u1")]
)
TILE_DTYPE = np.dtype([("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")])
INTEGRATOR_RAY_DTYPE = np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("t_max", "<f4"), ("ray_type", "<u4")])
OVERLAY_LINE_DTYPE = np.dtype([("p0", "<f4", 3), ("p1", "<f4", 3), ("rgb", "<f4", 3)])  # yk_overlay_line, 36 bytes
class SceneEdit(C.Structure):
    """yk_scene_edit: the tables of an edit in place (yk_scene_apply_edit); a NULL table keeps what the scene has."""

    _fields_ = [("spheres", C.POINTER(SphereDesc)), ("lights", C.POINTER(LightDesc)), ("materials", C.POINTER(MaterialDesc)), ("background", f32p)]


class SceneEditInfo(C.Structure):
    """yk_scene_edit_info: how a scene's last edit in place ran and what it rewrote (EDIT_* bits)."""

    _fields_ = [
        ("n_edits", C.c_uint32),
        ("route", C.c_uint32),
        ("reason", C.c_uint32),
        ("rewrote", C.c_uint32),
        ("seconds_check", C.c_double),
        ("seconds_tables", C.c_double),
        ("seconds_boxes", C.c_double),
        ("seconds_records", C.c_double),
        ("seconds_total", C.c_double),
    ]


class SceneTransformInfo(C.Structure):
    """yk_scene_transform_info: how a scene's last transform in place ran, what it keeps of the rest pose and the tree's cost."""

    _fields_ = [
        ("n_transforms", C.c_uint32),
        ("route", C.c_uint32),
        ("reason", C.c_uint32),
        ("n_moved_meshes", C.c_uint32),
        ("n_flipped_meshes", C.c_uint32),
        ("reserved", C.c_uint32),
        ("rest_bytes", C.c_uint64),
        ("tree_cost", C.c_double),
        ("tree_cost_rest", C.c_double),
        ("seconds_check", C.c_double),
        ("seconds_points", C.c_double),
        ("seconds_boxes", C.c_double),
        ("seconds_records", C.c_double),
        ("seconds_total", C.c_double),
    ]


SPHERE_DTYPE = np.dtype([("object_to_world", "<f4", 16), ("world_to_object", "<f4", 16), ("radius", "<f4"), ("material", "<i4")])  # yk_sphere_desc, 136 bytes
MESH_TRANSFORM_DTYPE = np.dtype([("rest_to_world", "<f4", 16), ("world_to_rest", "<f4", 16)])  # yk_mesh_transform, 128 bytes
GUIDE_DTYPE = np.dtype([("ns", "<f4", 3), ("hit", "<f4"), ("p", "<f4", 3), ("t", "<f4")])  # yk_guide, 32 bytes
HISTORY_DTYPE = np.dtype([("rgb", "<f4", 3), ("n", "<f4")])  # yk_history, 16 bytes
SURFACE_NONE = 0xFFFFFFFF  # YK_SURFACE_NONE
GUIDES_THROUGH_MAX = 8  # YK_GUIDES_THROUGH_MAX
SURFACE_ID_DTYPE = np.dtype([("shape", "<u4"), ("b", "<f4", 3)])  # yk_surface_id, 16 bytes
SURFACE_FLOATS = 28  # YK_SURFACE_FLOATS: one record of yk_surface
SURFACE_FIELDS = dict(hit=0, t=1, p=slice(2, 5), n=slice(5, 8), ns=slice(8, 11), dpdus=slice(11, 14), wo=slice(14, 17), u=17, v=18, material=19, area_light=20, shape=21, b=slice(22, 25), origin=slice(25, 28))
MOTION_DTYPE = np.dtype([("p_prev", "<f4", 3), ("known", "<f4")])  # yk_motion, 16 bytes
ALBEDO_DTYPE = np.dtype([("a", "<f4", 3), ("known", "<f4")])  # yk_albedo, 16 bytes
ALBEDO_FLOOR = 0.015625  # YK_ALBEDO_FLOOR, 2^-6
ALBEDO_MEAN_MAX_S = 8  # YK_ALBEDO_MEAN_MAX_S: the largest sub-sample grid of yk_albedo_mean
UPSAMPLE_MAX_S = 8  # YK_UPSAMPLE_MAX_S: the largest factor of yk_upsample
MOMENTS_DTYPE = np.dtype([("m1", "<f4"), ("m2", "<f4"), ("frames", "<f4"), ("n", "<f4")])  # yk_moments, 16 bytes: yk_history's layout
PIXEL_STATS_DTYPE = np.dtype([("mean", "<f4"), ("m2", "<f4"), ("n", "<u4"), ("drawn", "<u4")])  # yk_pixel_stats, 16 bytes

# enums (include/yuki_hip.h)
SPLIT_SAH, SPLIT_MIDDLE, SPLIT_EQUAL_COUNTS = 0, 1, 2
MAT_MATTE, MAT_GLASS, MAT_METAL, MAT_GLOSSY = 0, 1, 2, 3
LIGHT_POINT, LIGHT_SPOT, LIGHT_DISTANT, LIGHT_RECT = 0, 1, 2, 3
SAMPLER_UNIFORM, SAMPLER_STRATIFIED = 0, 1
INTEGRATOR_WHITTED, INTEGRATOR_PATH, INTEGRATOR_BVH_INTERSECTIONS, INTEGRATOR_GEOMETRY_NORMALS, INTEGRATOR_SHADING_NORMALS, INTEGRATOR_SHADING_UVS = 0, 1, 2, 3, 4, 5
RAY_DIRECT, RAY_REFLECTION, RAY_REFRACTION, RAY_NORMAL, RAY_SHADOW = 0, 1, 2, 3, 4
FOV_X, FOV_Y = 0, 1
TONE_MAP_RAW, TONE_MAP_FILMIC, TONE_MAP_HEATMAP = 0, 1, 2
HEATMAP_RED, HEATMAP_GREEN, HEATMAP_BLUE, HEATMAP_LUMINANCE = 0, 1, 2, 3
PRESENT_ENCODE_NONE, PRESENT_ENCODE_SHADER, PRESENT_ENCODE_SRGB = 0, 1, 2
PRESENT_RGBA8, PRESENT_RGB32F = 0, 1
LAYOUT_HOST, LAYOUT_DEVICE = 0, 1
UPDATE_ROUTE_HOST, UPDATE_ROUTE_DEVICE = 0, 1
EDIT_LIGHTS, EDIT_MATERIALS, EDIT_SPHERES, EDIT_BOXES, EDIT_RECORDS, EDIT_BACKGROUND = 1, 2, 4, 8, 16, 32  # yk_scene_edit_info.rewrote
LAYOUT_REASON_NONE, LAYOUT_REASON_OUT_OF_MEMORY, LAYOUT_REASON_DEVICE_ERROR, LAYOUT_REASON_MULTI = 0, 1, 2, 3
RECORDS_NODES, RECORDS_NODES4, RECORDS_TOP, RECORDS_TOP_ANY, RECORDS_TRIS, RECORDS_PRIM_SHADE, RECORDS_PRIM_ATTR = range(7)
RECORD_NAMES = ("nodes", "nodes4", "top", "top_any", "tris", "prim_shade", "prim_attr")


def pack_spheres(spheres):
    """A list of SceneData spheres (dicts of o2w, w2o, radius, material) -> (n,) SPHERE_DTYPE records, the array
    yk_scene_desc.spheres and yk_scene_edit.spheres point at."""
    out = np.zeros(len(spheres), dtype=SPHERE_DTYPE)
    if len(spheres):
        out["object_to_world"] = np.asarray([np.asarray(s["o2w"], dtype=np.float32).reshape(16) for s in spheres], dtype=np.float32)
        out["world_to_object"] = np.asarray([np.asarray(s["w2o"], dtype=np.float32).reshape(16) for s in spheres], dtype=np.float32)
        out["radius"] = np.asarray([s["radius"] for s in spheres], dtype=np.float64).astype(np.float32)
        out["material"] = np.asarray([int(s["material"]) for s in spheres], dtype=np.int32)
    return out


def pack_mesh_transforms(matrices):
    """One 4 x 4 matrix a mesh (row-major; an (n, 4, 4) array, or a list whose entries may be None for the identity) ->
    (n,) MESH_TRANSFORM_DTYPE records for Scene.transform.  rest_to_world is the matrix rounded to float32; world_to_rest
    is numpy.linalg.inv of the GIVEN matrix in float64, rounded once to float32 (the library does not invert: a caller
    that has a better inverse fills the records itself).  An identity entry gets the identity pair."""
    out = np.zeros(len(matrices), dtype=MESH_TRANSFORM_DTYPE)
    eye = np.eye(4, dtype=np.float32).reshape(16)
    for k, m in enumerate(matrices):
        if m is None:
            out["rest_to_world"][k] = out["world_to_rest"][k] = eye
            continue
        m = np.asarray(m, dtype=np.float64).reshape(4, 4)
        out["rest_to_world"][k] = m.astype(np.float32).reshape(16)
        out["world_to_rest"][k] = eye if np.array_equal(out["rest_to_world"][k], eye) else np.linalg.inv(m).astype(np.float32).reshape(16)
    return out


def ptr(a, ty):
    """Pointer into a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return C.cast(None, ty)
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ty)


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def f16(m):
    return (C.c_float * 16)(*[float(x) for x in np.asarray(m, dtype=np.float32).reshape(16)])
