//! Raw bindings for `include/yuki_hip.h` (ABI version 1).  Field order and types follow the
//! header line by line; see the header for the reference file:line each item replaces.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const YK_ABI_VERSION: u32 = 1;

pub type yk_status = c_int;
pub const YK_OK: yk_status = 0;
pub const YK_ERR_INVALID_ARGUMENT: yk_status = 1;
pub const YK_ERR_NO_DEVICE: yk_status = 2;
pub const YK_ERR_DEVICE: yk_status = 3;
pub const YK_ERR_OUT_OF_MEMORY: yk_status = 4;
pub const YK_ERR_UNSUPPORTED: yk_status = 5;
pub const YK_ERR_BVH_BUILD: yk_status = 6;
pub const YK_ERR_CANCELLED: yk_status = 7;
pub const YK_ERR_STACK_OVERFLOW: yk_status = 8;

pub const YK_MAT_MATTE: u32 = 0;
pub const YK_MAT_GLASS: u32 = 1;
pub const YK_MAT_METAL: u32 = 2;
pub const YK_MAT_GLOSSY: u32 = 3;
pub const YK_MAT_FLAG_REMAP: u32 = 1;
pub const YK_MAT_FLAG_TEXTURED_A: u32 = 2;
pub const YK_LIGHT_POINT: u32 = 0;
pub const YK_LIGHT_SPOT: u32 = 1;
pub const YK_LIGHT_DISTANT: u32 = 2;
pub const YK_LIGHT_RECT: u32 = 3;
pub const YK_SPLIT_SAH: u32 = 0;
pub const YK_SPLIT_MIDDLE: u32 = 1;
pub const YK_SPLIT_EQUAL_COUNTS: u32 = 2;
pub const YK_SAMPLER_UNIFORM: u32 = 0;
pub const YK_SAMPLER_STRATIFIED: u32 = 1;
pub const YK_INTEGRATOR_WHITTED: u32 = 0;
pub const YK_INTEGRATOR_PATH: u32 = 1;
pub const YK_INTEGRATOR_BVH_INTERSECTIONS: u32 = 2;
pub const YK_INTEGRATOR_GEOMETRY_NORMALS: u32 = 3;
pub const YK_INTEGRATOR_SHADING_NORMALS: u32 = 4;
pub const YK_INTEGRATOR_SHADING_UVS: u32 = 5;
pub const YK_RAY_DIRECT: u32 = 0;
pub const YK_RAY_REFLECTION: u32 = 1;
pub const YK_RAY_REFRACTION: u32 = 2;
pub const YK_RAY_NORMAL: u32 = 3;
pub const YK_RAY_SHADOW: u32 = 4;
pub const YK_LI_DEBUG_MAX_RECORDS: u32 = 1 << 24;
pub const YK_TONE_MAP_RAW: u32 = 0;
pub const YK_TONE_MAP_FILMIC: u32 = 1;
pub const YK_TONE_MAP_HEATMAP: u32 = 2;
pub const YK_HEATMAP_RED: u32 = 0;
pub const YK_HEATMAP_GREEN: u32 = 1;
pub const YK_HEATMAP_BLUE: u32 = 2;
pub const YK_HEATMAP_LUMINANCE: u32 = 3;
pub const YK_PRESENT_ENCODE_NONE: u32 = 0;
pub const YK_PRESENT_ENCODE_SHADER: u32 = 1;
pub const YK_PRESENT_ENCODE_SRGB: u32 = 2;
pub const YK_PRESENT_RGBA8: u32 = 0;
pub const YK_PRESENT_RGB32F: u32 = 1;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_mesh_desc {
    pub has_normals: u8,
    pub has_uvs: u8,
    pub swaps_handedness: u8,
    pub pad: u8,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_sphere_desc {
    pub object_to_world: [f32; 16],
    pub world_to_object: [f32; 16],
    pub radius: f32,
    pub material: i32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_material_desc {
    pub kind: u32,
    pub a: [f32; 3],
    pub b: [f32; 3],
    pub c: f32,
    pub flags: u32,
    pub a_texture: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_texture_desc {
    pub width: u32,
    pub height: u32,
    pub rgb: *const f32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_light_desc {
    pub kind: u32,
    pub p: [f32; 3],
    pub i: [f32; 3],
    pub cos_total_width: f32,
    pub cos_falloff_start: f32,
    pub world_to_light: [f32; 16],
    pub sample_to_world: [f32; 16],
    pub sample_to_world_inv: [f32; 16],
    pub area: f32,
}

#[repr(C)]
pub struct yk_scene_desc {
    pub n_vertices: u32,
    pub points: *const f32,
    pub normals: *const f32,
    pub uvs: *const f32,
    pub n_triangles: u32,
    pub indices: *const u32,
    pub tri_mesh: *const u32,
    pub tri_material: *const i32,
    pub tri_area_light: *const i32,
    pub n_meshes: u32,
    pub meshes: *const yk_mesh_desc,
    pub n_spheres: u32,
    pub spheres: *const yk_sphere_desc,
    pub n_materials: u32,
    pub materials: *const yk_material_desc,
    pub n_lights: u32,
    pub lights: *const yk_light_desc,
    pub background: [f32; 3],
    pub split_method: u32,
    pub max_shapes_in_node: u32,
    pub shape_order: *const u32,
    pub n_textures: u32,
    pub textures: *const yk_texture_desc,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_camera {
    pub camera_to_world: [f32; 16],
    pub camera_to_world_inv: [f32; 16],
    pub raster_to_camera: [f32; 16],
    pub raster_to_camera_inv: [f32; 16],
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_camera_params {
    pub position: [f32; 3],
    pub target: [f32; 3],
    pub up: [f32; 3],
    pub fov_axis: u32,
    pub fov_degrees: f32,
    pub res_x: u16,
    pub res_y: u16,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_sampler_desc {
    pub kind: u32,
    pub nx: u32,
    pub ny: u32,
    pub jitter: u32,
    pub seed: u64,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_integrator_desc {
    pub kind: u32,
    pub max_depth: u32,
    pub has_clamp: u32,
    pub indirect_clamp: f32,
}

/// ToneMapType (app/renderpasses/tonemap.rs:40-44) with its params
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_tone_map_desc {
    pub kind: u32,
    pub exposure: f32,
    pub channel: u32,
    pub has_bounds: u32,
    pub bounds: [f32; 2],
}

/// The exposure meter's rule (yk_exposure.h): cuts in units of 1/65536, bias, clamp, rates and window
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_exposure_desc {
    pub low_cut: u32,
    pub high_cut: u32,
    pub ev_bias: f32,
    pub min_ev: f32,
    pub max_ev: f32,
    pub adapt_up: f32,
    pub adapt_down: f32,
    pub window: [u16; 4],
}

/// The exposure meter's 32-byte record
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_exposure_state {
    pub exposure: f32,
    pub log2_adapted: f32,
    pub log2_metered: f32,
    pub frames: u32,
    pub counted: u32,
    pub skipped: u32,
    pub below: u32,
    pub above: u32,
}

/// ScaleOutput::draw (app/renderpasses/scale_output.rs): the window, the encode and the frame format
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_present_desc {
    pub window_x: u16,
    pub window_y: u16,
    pub encode: u32,
    pub format: u32,
}

/// First-hit geometry of the ray through a pixel centre: what the denoiser's stops read (yuki_amd/csrc/yk_denoise.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_guide {
    pub ns: [f32; 3],
    pub hit: f32,
    pub p: [f32; 3],
    pub t: f32,
}

/// The à-trous iterations (0 ..= 8) and the colour, normal and plane-distance stops; +inf switches a stop off
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_denoise_desc {
    pub iterations: u32,
    pub sigma_color: f32,
    pub sigma_normal: f32,
    pub sigma_plane: f32,
}

/// A pixel's history across camera moves: the mean radiance and the effective number of samples behind it (0 = none);
/// 16-byte aligned on the device (yuki_amd/csrc/yk_temporal.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_history {
    pub rgb: [f32; 3],
    pub n: f32,
}

/// The plane test (scene units, > 0, +inf = off) and the normal test ([-1, 1]) of reproject, and blend's history clamp (>= 1)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_temporal_desc {
    pub plane_tolerance: f32,
    pub normal_cos_min: f32,
    pub max_history: f32,
}

/// A pixel's luminance moments beside its history: the layout of `yk_history`, so a moments buffer goes through
/// `yk_history_reproject[_moved][_device]` cast to it (yuki_amd/csrc/yk_variance.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_moments {
    pub m1: f32,
    pub m2: f32,
    pub frames: f32,
    pub n: f32,
}

/// A pixel's adaptive-sampling statistics beside its film sum: running mean and sum of squared deviations of the
/// luminance of the samples taken, their number, and the pixel's next sample index (yuki_amd/csrc/yk_adaptive.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_pixel_stats {
    pub mean: f32,
    pub m2: f32,
    pub n: u32,
    pub drawn: u32,
}

/// The adaptive sampler's rule: min_samples >= 2, max_samples in min_samples..=2^24, round_passes 1..=0xFFFF,
/// max_rounds 0 = until nothing is selected, dilate 0 | 1, threshold > 0, epsilon >= 0
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_adaptive_desc {
    pub min_samples: u32,
    pub max_samples: u32,
    pub round_passes: u32,
    pub max_rounds: u32,
    pub dilate: u32,
    pub threshold: f32,
    pub epsilon: f32,
}

/// What `yk_render_adaptive_device` did
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_adaptive_info {
    pub rounds: u32,
    pub converged: u32,
    pub first_pixels: u32,
    pub last_pixels: u32,
    pub samples: u64,
    pub rays: u64,
    pub shadow_rays: u64,
}

/// The variance-guided a-trous filter: iterations 0..=8, the variance-scaled colour stop, the normal and plane stops (each
/// > 0, +inf = off), epsilon under the colour stop and the factor on the spatial variance estimate (both >= 0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_variance_desc {
    pub iterations: u32,
    pub sigma_variance: f32,
    pub sigma_normal: f32,
    pub sigma_plane: f32,
    pub epsilon: f32,
    pub spatial_scale: f32,
}

/// `yk_surface_id::shape` on a miss
pub const YK_SURFACE_NONE: u32 = 0xffff_ffff;
/// the most glass interfaces `yk_render_guides_through` follows
pub const YK_GUIDES_THROUGH_MAX: u32 = 8;

/// The identity of a pixel's first hit beside its guide: the source shape (a sphere is n_triangles + k) and the hit's
/// barycentrics; 16-byte aligned on the device (yuki_amd/csrc/yk_motion.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_surface_id {
    pub shape: u32,
    pub b: [f32; 3],
}

/// Where a pixel's surface point stood under the previous vertex array; known = 0: nowhere (then p_prev is 0)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_motion {
    pub p_prev: [f32; 3],
    pub known: f32,
}

/// The floor under the divisor of `yk_denoise_albedo`, 2^-6
pub const YK_ALBEDO_FLOOR: f32 = 0.015625;
pub const YK_ALBEDO_MEAN_MAX_S: u32 = 8;

/// The diffuse albedo of a pixel's first hit; known = 0: nothing to demodulate by (then a is all ones); 16-byte aligned on
/// the device (yuki_amd/csrc/yk_albedo.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_albedo {
    pub a: [f32; 3],
    pub known: f32,
}

/// The largest factor of `yk_upsample` (= YK_ALBEDO_MEAN_MAX_S)
pub const YK_UPSAMPLE_MAX_S: u32 = 8;

/// The factor (1 ..= 8) and the normal and plane-distance stops of the guided upsample; +inf switches a stop off
/// (yuki_amd/csrc/yk_upsample.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_upsample_desc {
    pub s: u32,
    pub sigma_normal: f32,
    pub sigma_plane: f32,
}

/// The window and the box of the history rectification: the (2 radius + 1)^2 pixels of the current film around a pixel
/// (radius 1 .. 3) and the half-width of the box in standard deviations (>= 0, +inf = every pixel passes through)
/// (yuki_amd/csrc/yk_rectify.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_rectify_desc {
    pub radius: u32,
    pub gamma: f32,
}

/// yk_despeckle_desc::flags: a pixel that is not finite becomes the mean of its taken taps
pub const YK_DESPECKLE_REPAIR: u32 = 1;

/// The window, the rank and the gain of the despeckle pass: a film pixel brighter than `gain` x the rank-th largest
/// luminance among the other pixels of its (2 radius + 1)^2 window (radius 1 .. 2, rank 1 .. 4) is scaled down to that
/// bound; fewer than max(min_taps, rank) usable taps, or a luminance below `floor`, and it passes through
/// (yuki_amd/csrc/yk_despeckle.h)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_despeckle_desc {
    pub radius: u32,
    pub rank: u32,
    pub min_taps: u32,
    pub flags: u32,
    pub gain: f32,
    pub floor: f32,
}

/// The target rectangle of ScaleOutput::draw in top-down window coordinates
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_present_rect {
    pub x0: i32,
    pub y0: i32,
    pub width: u32,
    pub height: u32,
}

/// IntegratorRay (integrators/mod.rs:76-80): the ray and its yk_ray_type
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_integrator_ray {
    pub o: [f32; 3],
    pub d: [f32; 3],
    pub t_max: f32,
    pub ray_type: u32,
}

/// A world-space segment and its colour (RayVisualization's two vertices of a line)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_overlay_line {
    pub p0: [f32; 3],
    pub p1: [f32; 3],
    pub rgb: [f32; 3],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_tile {
    pub x0: u16,
    pub y0: u16,
    pub x1: u16,
    pub y1: u16,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_bvh_node {
    pub bmin: [f32; 3],
    pub bmax: [f32; 3],
    pub a: u32,
    pub count: u16,
    pub axis: u8,
    pub is_leaf: u8,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_scene_info {
    pub n_nodes: u64,
    pub n_interior: u64,
    pub n_shapes: u64,
    pub bounds_min: [f32; 3],
    pub bounds_max: [f32; 3],
    pub build_seconds: f64,
    pub upload_seconds: f64,
    pub device_bytes: u64,
    pub max_leaf_shapes: u32,
    pub tree_depth: u32,
}

pub const YK_BVH_BUILDER_HOST: u32 = 0;
pub const YK_BVH_BUILDER_DEVICE: u32 = 1;
pub const YK_BVH_BUILDER_HOST_LEVELS: u32 = 2;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_bvh_build_info {
    pub builder: u32,
    pub reason: u32,
    pub levels: u32,
    pub small_range: u32,
    pub small_ranges: u64,
    pub seconds_upload: f64,
    pub seconds_levels: f64,
    pub seconds_small: f64,
    pub seconds_layout: f64,
    pub seconds_copy_back: f64,
}

pub const YK_LAYOUT_HOST: u32 = 0;
pub const YK_LAYOUT_DEVICE: u32 = 1;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_scene_layout_info {
    pub layout: u32,
    pub reason: u32,
    pub seconds_upload: f64,
    pub seconds_layout: f64,
    pub tree_fetched: u32,
    pub root_ref: u32,
    pub n_top: u32,
    pub n_top_any: u32,
    pub wide: u32,
    pub wide_auto: u32,
}

pub const YK_UPDATE_ROUTE_HOST: u32 = 0;
pub const YK_UPDATE_ROUTE_DEVICE: u32 = 1;

/// the tables of an edit in place (yk_scene_apply_edit); a null table keeps what the scene has
#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_scene_edit {
    pub spheres: *const yk_sphere_desc,
    pub lights: *const yk_light_desc,
    pub materials: *const yk_material_desc,
    pub background: *const f32,
}

pub const YK_EDIT_LIGHTS: u32 = 1;
pub const YK_EDIT_MATERIALS: u32 = 2;
pub const YK_EDIT_SPHERES: u32 = 4;
pub const YK_EDIT_BOXES: u32 = 8;
pub const YK_EDIT_RECORDS: u32 = 16;
pub const YK_EDIT_BACKGROUND: u32 = 32;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_scene_edit_info {
    pub n_edits: u32,
    pub route: u32,
    pub reason: u32,
    pub rewrote: u32,
    pub seconds_check: f64,
    pub seconds_tables: f64,
    pub seconds_boxes: f64,
    pub seconds_records: f64,
    pub seconds_total: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_scene_update_info {
    pub n_updates: u32,
    pub route: u32,
    pub reason: u32,
    pub n_levels: u32,
    pub plan_bytes: u64,
    pub seconds_check: f64,
    pub seconds_boxes: f64,
    pub seconds_records: f64,
    pub seconds_total: f64,
}

/// one record a mesh of yk_scene_transform: the mesh's place relative to its rest pose, row-major; the pair is the caller's
#[repr(C)]
#[derive(Clone, Copy)]
pub struct yk_mesh_transform {
    pub rest_to_world: [f32; 16],
    pub world_to_rest: [f32; 16],
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_scene_transform_info {
    pub n_transforms: u32,
    pub route: u32,
    pub reason: u32,
    pub n_moved_meshes: u32,
    pub n_flipped_meshes: u32,
    pub reserved: u32,
    pub rest_bytes: u64,
    pub tree_cost: f64,
    pub tree_cost_rest: f64,
    pub seconds_check: f64,
    pub seconds_points: f64,
    pub seconds_boxes: f64,
    pub seconds_records: f64,
    pub seconds_total: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_combiner_info {
    pub submissions: u64,
    pub tiles: u64,
    pub requeued: u64,
    pub largest_submission: u32,
    pub lanes: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct yk_render_stats {
    pub rays: u64,
    pub shadow_rays: u64,
    pub samples: u64,
    pub seconds_total: f64,
    pub seconds_trace: f64,
    pub seconds_shadow: f64,
    pub seconds_shade: f64,
    pub trace_launches: u32,
    pub batches: u32,
    pub shadow_launches: u32,
    pub reserved: u32,
}

pub enum yk_context {}
pub enum yk_scene {}
pub enum yk_loaded_scene {}
pub enum yk_tile_list {}
pub enum yk_pixel_list {}
pub const YK_MULTI_SHARED_DEVICES: u32 = 1;
pub const YK_MULTI_PEER_COPY: u32 = 2;
pub enum yk_multi {}
pub enum yk_multi_scene {}
pub enum yk_multi_film {}
pub enum yk_dist {}
pub enum yk_combiner {}
pub type yk_cancel_fn = Option<unsafe extern "C" fn(user: *mut c_void) -> c_int>;

extern "C" {
    pub fn yk_abi_version() -> u32;
    pub fn yk_status_string(s: yk_status) -> *const c_char;
    pub fn yk_context_create(device: c_int, out: *mut *mut yk_context) -> yk_status;
    pub fn yk_context_destroy(ctx: *mut yk_context);
    pub fn yk_last_error(ctx: *const yk_context, buf: *mut c_char, cap: usize) -> yk_status;
    pub fn yk_context_stream(ctx: *const yk_context) -> *mut c_void;
    pub fn yk_context_set_option(ctx: *mut yk_context, key: *const c_char, value: i64) -> yk_status;
    pub fn yk_camera_init(params: *const yk_camera_params, out: *mut yk_camera) -> yk_status;
    pub fn yk_film_tiles(res_x: u16, res_y: u16, tile_dim: u16, out: *mut yk_tile, cap: usize) -> usize;
    pub fn yk_make_rect_light(light_to_world: *const f32, light_to_world_inv: *const f32, radiance: *const f32, size: *const f32, out: *mut yk_light_desc) -> yk_status;
    pub fn yk_make_spot_light(light_to_world: *const f32, light_to_world_inv: *const f32, intensity: *const f32, total_width_degrees: f32, falloff_start_degrees: f32, out: *mut yk_light_desc) -> yk_status;
    pub fn yk_make_point_light(light_to_world: *const f32, intensity: *const f32, out: *mut yk_light_desc) -> yk_status;
    pub fn yk_film_update_tiles(tiles: *const yk_tile, n_tiles: usize, tile_rgb: *const f32, res_x: u16, res_y: u16, film_rgb: *mut f32) -> yk_status;
    pub fn yk_scene_create(ctx: *mut yk_context, desc: *const yk_scene_desc, out: *mut *mut yk_scene) -> yk_status;
    /// `desc`'s large arrays are device pointers on `ctx`'s device; `stream` is the hipStream_t that produced them (or null).
    pub fn yk_scene_create_device(ctx: *mut yk_context, desc: *const yk_scene_desc, stream: *mut c_void, out: *mut *mut yk_scene) -> yk_status;
    pub fn yk_scene_destroy(scene: *mut yk_scene);
    pub fn yk_scene_get_info(scene: *const yk_scene, out: *mut yk_scene_info) -> yk_status;
    pub fn yk_scene_update(ctx: *mut yk_context, scene: *mut yk_scene, points: *const f32, normals: *const f32) -> yk_status;
    pub fn yk_scene_update_device(ctx: *mut yk_context, scene: *mut yk_scene, d_points: *const f32, d_normals: *const f32, stream: *mut c_void) -> yk_status;
    pub fn yk_scene_get_update_info(scene: *const yk_scene, out: *mut yk_scene_update_info) -> yk_status;
    pub fn yk_scene_apply_edit(ctx: *mut yk_context, scene: *mut yk_scene, edit: *const yk_scene_edit) -> yk_status;
    pub fn yk_scene_apply_edit_device(ctx: *mut yk_context, scene: *mut yk_scene, edit: *const yk_scene_edit, d_spheres: *const c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_scene_get_edit_info(scene: *const yk_scene, out: *mut yk_scene_edit_info) -> yk_status;
    pub fn yk_scene_transform(ctx: *mut yk_context, scene: *mut yk_scene, transforms: *const yk_mesh_transform) -> yk_status;
    pub fn yk_scene_transform_device(ctx: *mut yk_context, scene: *mut yk_scene, d_transforms: *const c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_scene_get_transform_info(scene: *const yk_scene, out: *mut yk_scene_transform_info) -> yk_status;
    pub fn yk_bvh_refit(nodes: *mut yk_bvh_node, n_nodes: usize, shape_order: *const u32, n_shapes: usize, shape_bounds: *const f32) -> yk_status;
    pub fn yk_scene_export_bvh(scene: *const yk_scene, nodes: *mut yk_bvh_node, shape_order: *mut u32) -> yk_status;
    pub fn yk_scene_get_build_info(scene: *const yk_scene, out: *mut yk_bvh_build_info) -> yk_status;
    pub fn yk_scene_get_layout_info(scene: *const yk_scene, out: *mut yk_scene_layout_info) -> yk_status;
    pub fn yk_render_tiles(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tiles: *const yk_tile, n_tiles: usize, out_rgb: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_render_tiles_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tiles: *const yk_tile, n_tiles: usize, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_render_tiles_accumulating(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tiles: *const yk_tile, tile_samples: *const u16, n_tiles: usize, out_rgb: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_render_tiles_accumulating_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tiles: *const yk_tile, tile_samples: *const u16, n_tiles: usize, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_film_accumulate_tiles(tiles: *const yk_tile, n_tiles: usize, tile_rgb: *const f32, res_x: u16, res_y: u16, film_rgb: *mut f32, tile_sample_counts: *mut u32) -> yk_status;
    pub fn yk_film_accumulate_tiles_device(ctx: *mut yk_context, tiles: *const yk_tile, n_tiles: usize, d_tile_rgb: *const c_void, res_x: u16, res_y: u16, d_film_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_tile_list_create(ctx: *mut yk_context, tiles: *const yk_tile, tile_samples: *const u16, n_tiles: usize, out: *mut *mut yk_tile_list) -> yk_status;
    pub fn yk_tile_list_destroy(list: *mut yk_tile_list);
    pub fn yk_render_tile_list_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, list: *const yk_tile_list, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_film_update_tile_list_device(ctx: *mut yk_context, list: *const yk_tile_list, d_tile_rgb: *const c_void, res_x: u16, res_y: u16, d_film_rgb: *mut c_void, stream: *mut c_void, accumulate: c_int) -> yk_status;
    pub fn yk_render_tiles_accumulating_passes(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tiles: *const yk_tile, tile_samples: *const u16, n_tiles: usize, n_passes: u32, out_rgb: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_render_tile_list_samples_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, list: *const yk_tile_list, first_sample: u32, n_passes: u32, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_context_interrupt(ctx: *mut yk_context) -> yk_status;
    pub fn yk_combiner_create(contexts: *const *mut yk_context, n_contexts: u32, max_tiles: u32, linger_us: u32, out: *mut *mut yk_combiner) -> yk_status;
    pub fn yk_combiner_destroy(combiner: *mut yk_combiner);
    pub fn yk_combiner_render_tile(combiner: *mut yk_combiner, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tile: *const yk_tile, accumulating_sample: i32, tile_pixels: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_combiner_get_info(combiner: *const yk_combiner, out: *mut yk_combiner_info) -> yk_status;
    pub fn yk_combiner_last_error(combiner: *const yk_combiner, buf: *mut c_char, cap: usize) -> yk_status;
    pub fn yk_render_tile_list_passes_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, list: *const yk_tile_list, n_passes: u32, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_film_accumulate_tile_list_passes_device(ctx: *mut yk_context, list: *const yk_tile_list, d_passes_rgb: *const c_void, n_passes: u32, res_x: u16, res_y: u16, d_film_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_write_exr(path: *const c_char, width: u32, height: u32, rgb: *const f32) -> yk_status;
    pub fn yk_write_pfm(path: *const c_char, width: u32, height: u32, rgb: *const f32) -> yk_status;
    pub fn yk_tone_map(ctx: *mut yk_context, desc: *const yk_tone_map_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_rgb: *mut f32, used_bounds: *mut f32) -> yk_status;
    pub fn yk_tone_map_device(ctx: *mut yk_context, desc: *const yk_tone_map_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_film_min_max(ctx: *mut yk_context, film_rgb: *const f32, res_x: u16, res_y: u16, channel: u32, out_min_max: *mut f32) -> yk_status;
    pub fn yk_film_histogram(ctx: *mut yk_context, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, window: *const u16, out_bins: *mut u32, out_skipped_below_above: *mut u32) -> yk_status;
    pub fn yk_exposure_meter(ctx: *mut yk_context, desc: *const yk_exposure_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, prev: *const yk_exposure_state, out: *mut yk_exposure_state) -> yk_status;
    pub fn yk_exposure_meter_device(ctx: *mut yk_context, desc: *const yk_exposure_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_prev: *const c_void, d_out_state: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_tone_map_metered_device(ctx: *mut yk_context, desc: *const yk_tone_map_desc, d_state: *const c_void, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_scene_node_bounds(scene: *const yk_scene, target_level: i32, out_bounds: *mut f32, cap: usize) -> usize;
    pub fn yk_overlay_world_to_clip(params: *const yk_camera_params, scene_bounds: *const f32, out: *mut f32) -> yk_status;
    pub fn yk_overlay_ray_lines(rays: *const yk_integrator_ray, n: usize, out: *mut yk_overlay_line) -> yk_status;
    pub fn yk_overlay_draw(ctx: *mut yk_context, world_to_clip: *const f32, lines: *const yk_overlay_line, n_lines: usize, boxes: *const f32, n_boxes: usize, film_rgb: *mut f32, res_x: u16, res_y: u16) -> yk_status;
    pub fn yk_overlay_draw_device(ctx: *mut yk_context, world_to_clip: *const f32, d_lines: *const c_void, n_lines: usize, d_boxes: *const c_void, n_boxes: usize, d_film_rgb: *mut c_void, res_x: u16, res_y: u16, stream: *mut c_void) -> yk_status;
    pub fn yk_present_target_rect(res_x: u16, res_y: u16, window_x: u16, window_y: u16, out: *mut yk_present_rect) -> yk_status;
    pub fn yk_present(ctx: *mut yk_context, desc: *const yk_present_desc, film_rgb: *const f32, res_x: u16, res_y: u16, out: *mut c_void) -> yk_status;
    pub fn yk_present_device(ctx: *mut yk_context, desc: *const yk_present_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_render_guides(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, out: *mut yk_guide) -> yk_status;
    pub fn yk_render_guides_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, d_guides: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_denoise(ctx: *mut yk_context, desc: *const yk_denoise_desc, film_rgb: *const f32, guides: *const yk_guide, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_rgb: *mut f32) -> yk_status;
    pub fn yk_denoise_device(ctx: *mut yk_context, desc: *const yk_denoise_desc, d_film_rgb: *const c_void, d_guides: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_history_reproject(ctx: *mut yk_context, desc: *const yk_temporal_desc, prev_history: *const yk_history, prev_guides: *const yk_guide, prev_camera: *const yk_camera, guides: *const yk_guide, res_x: u16, res_y: u16, out_history: *mut yk_history) -> yk_status;
    pub fn yk_history_reproject_device(ctx: *mut yk_context, desc: *const yk_temporal_desc, d_prev_history: *const c_void, d_prev_guides: *const c_void, prev_camera: *const yk_camera, d_guides: *const c_void, res_x: u16, res_y: u16, d_out_history: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_history_blend(ctx: *mut yk_context, desc: *const yk_temporal_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, history: *const yk_history, out_history: *mut yk_history, out_rgb: *mut f32) -> yk_status;
    pub fn yk_history_blend_device(ctx: *mut yk_context, desc: *const yk_temporal_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_history: *const c_void, d_out_history: *mut c_void, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_render_guides_ids(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, out_guides: *mut yk_guide, out_ids: *mut yk_surface_id) -> yk_status;
    pub fn yk_render_guides_ids_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, d_guides: *mut c_void, d_ids: *mut c_void, stream: *mut c_void) -> yk_status;
    /// guides through glass (yuki_amd/csrc/yk_guides_through.h): the same records at the first hit that is not glass
    pub fn yk_render_guides_through(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, max_through: u32, out_guides: *mut yk_guide, out_ids: *mut yk_surface_id, out_through: *mut u32) -> yk_status;
    pub fn yk_render_guides_through_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, res_x: u16, res_y: u16, max_through: u32, d_guides: *mut c_void, d_ids: *mut c_void, d_through: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_surface_motion(ctx: *mut yk_context, scene: *const yk_scene, ids: *const yk_surface_id, guides: *const yk_guide, prev_points: *const f32, res_x: u16, res_y: u16, out: *mut yk_motion) -> yk_status;
    pub fn yk_surface_motion_device(ctx: *mut yk_context, scene: *const yk_scene, d_ids: *const c_void, d_guides: *const c_void, d_prev_points: *const f32, res_x: u16, res_y: u16, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_surface_motion_spheres(ctx: *mut yk_context, scene: *const yk_scene, ids: *const yk_surface_id, guides: *const yk_guide, prev_points: *const f32, prev_spheres: *const yk_sphere_desc, res_x: u16, res_y: u16, out: *mut yk_motion) -> yk_status;
    pub fn yk_surface_motion_spheres_device(ctx: *mut yk_context, scene: *const yk_scene, d_ids: *const c_void, d_guides: *const c_void, d_prev_points: *const f32, d_prev_spheres: *const c_void, res_x: u16, res_y: u16, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_surface_motion_transforms(ctx: *mut yk_context, scene: *const yk_scene, ids: *const yk_surface_id, guides: *const yk_guide, prev_transforms: *const yk_mesh_transform, prev_spheres: *const yk_sphere_desc, res_x: u16, res_y: u16, out: *mut yk_motion) -> yk_status;
    pub fn yk_surface_motion_transforms_device(ctx: *mut yk_context, scene: *const yk_scene, d_ids: *const c_void, d_guides: *const c_void, d_prev_transforms: *const c_void, d_prev_spheres: *const c_void, res_x: u16, res_y: u16, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_history_reproject_moved(ctx: *mut yk_context, desc: *const yk_temporal_desc, prev_history: *const yk_history, prev_guides: *const yk_guide, prev_camera: *const yk_camera, guides: *const yk_guide, motion: *const yk_motion, res_x: u16, res_y: u16, out_history: *mut yk_history) -> yk_status;
    pub fn yk_history_reproject_moved_device(ctx: *mut yk_context, desc: *const yk_temporal_desc, d_prev_history: *const c_void, d_prev_guides: *const c_void, prev_camera: *const yk_camera, d_guides: *const c_void, d_motion: *const c_void, res_x: u16, res_y: u16, d_out_history: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_surface_albedo(ctx: *mut yk_context, scene: *const yk_scene, ids: *const yk_surface_id, res_x: u16, res_y: u16, out: *mut yk_albedo) -> yk_status;
    pub fn yk_surface_albedo_device(ctx: *mut yk_context, scene: *const yk_scene, d_ids: *const c_void, res_x: u16, res_y: u16, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_albedo_mean(ctx: *mut yk_context, scene: *const yk_scene, ids_ss: *const yk_surface_id, res_x: u16, res_y: u16, s: u32, out: *mut yk_albedo) -> yk_status;
    pub fn yk_albedo_mean_device(ctx: *mut yk_context, scene: *const yk_scene, d_ids_ss: *const c_void, res_x: u16, res_y: u16, s: u32, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_render_albedo_mean(ctx: *mut yk_context, scene: *const yk_scene, camera_ss: *const yk_camera, res_x: u16, res_y: u16, s: u32, out: *mut yk_albedo) -> yk_status;
    pub fn yk_render_albedo_mean_device(ctx: *mut yk_context, scene: *const yk_scene, camera_ss: *const yk_camera, res_x: u16, res_y: u16, s: u32, d_out: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_denoise_albedo(ctx: *mut yk_context, desc: *const yk_denoise_desc, film_rgb: *const f32, guides: *const yk_guide, albedo: *const yk_albedo, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_rgb: *mut f32) -> yk_status;
    pub fn yk_denoise_albedo_device(ctx: *mut yk_context, desc: *const yk_denoise_desc, d_film_rgb: *const c_void, d_guides: *const c_void, d_albedo: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_upsample(ctx: *mut yk_context, desc: *const yk_upsample_desc, low_rgb: *const f32, low_guides: *const yk_guide, low_albedo: *const yk_albedo, low_res_x: u16, low_res_y: u16, tile_dim: u16, samples: *const u32, guides: *const yk_guide, albedo: *const yk_albedo, out_rgb: *mut f32, out_weight: *mut f32) -> yk_status;
    pub fn yk_upsample_device(ctx: *mut yk_context, desc: *const yk_upsample_desc, d_low_rgb: *const c_void, d_low_guides: *const c_void, d_low_albedo: *const c_void, low_res_x: u16, low_res_y: u16, tile_dim: u16, samples: *const u32, d_guides: *const c_void, d_albedo: *const c_void, d_out_rgb: *mut c_void, d_out_weight: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_moments_blend(ctx: *mut yk_context, desc: *const yk_temporal_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, moments: *const yk_moments, out_moments: *mut yk_moments) -> yk_status;
    pub fn yk_moments_blend_device(ctx: *mut yk_context, desc: *const yk_temporal_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_moments: *const c_void, d_out_moments: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_variance(ctx: *mut yk_context, desc: *const yk_variance_desc, moments: *const yk_moments, film_rgb: *const f32, guides: *const yk_guide, albedo: *const yk_albedo, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_variance: *mut f32) -> yk_status;
    pub fn yk_variance_device(ctx: *mut yk_context, desc: *const yk_variance_desc, d_moments: *const c_void, d_film_rgb: *const c_void, d_guides: *const c_void, d_albedo: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_variance: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_denoise_variance(ctx: *mut yk_context, desc: *const yk_variance_desc, film_rgb: *const f32, guides: *const yk_guide, variance: *const f32, albedo: *const yk_albedo, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_rgb: *mut f32) -> yk_status;
    pub fn yk_denoise_variance_device(ctx: *mut yk_context, desc: *const yk_variance_desc, d_film_rgb: *const c_void, d_guides: *const c_void, d_variance: *const c_void, d_albedo: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_history_rectify(ctx: *mut yk_context, desc: *const yk_rectify_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, history: *const yk_history, moments: *const yk_moments, out_history: *mut yk_history, out_moments: *mut yk_moments) -> yk_status;
    pub fn yk_history_rectify_device(ctx: *mut yk_context, desc: *const yk_rectify_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_history: *const c_void, d_moments: *const c_void, d_out_history: *mut c_void, d_out_moments: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_despeckle(ctx: *mut yk_context, desc: *const yk_despeckle_desc, film_rgb: *const f32, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, out_rgb: *mut f32, out_mask: *mut u8, out_counts: *mut u32) -> yk_status;
    pub fn yk_despeckle_device(ctx: *mut yk_context, desc: *const yk_despeckle_desc, d_film_rgb: *const c_void, res_x: u16, res_y: u16, tile_dim: u16, samples: *const u32, d_out_rgb: *mut c_void, d_out_mask: *mut c_void, d_out_counts: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_pixel_list_create(ctx: *mut yk_context, res_x: u16, res_y: u16, out: *mut *mut yk_pixel_list) -> yk_status;
    pub fn yk_pixel_list_destroy(list: *mut yk_pixel_list);
    pub fn yk_pixel_list_set(list: *mut yk_pixel_list, xy: *const u32, sample: *const u32, n: u32, passes: u32) -> yk_status;
    pub fn yk_pixel_list_read(list: *const yk_pixel_list, out_xy: *mut u32, out_sample: *mut u32, cap: u32, out_n: *mut u32) -> yk_status;
    pub fn yk_adaptive_select(ctx: *mut yk_context, desc: *const yk_adaptive_desc, stats: *const yk_pixel_stats, res_x: u16, res_y: u16, out_xy: *mut u32, out_sample: *mut u32, out_n: *mut u32) -> yk_status;
    pub fn yk_adaptive_select_device(ctx: *mut yk_context, desc: *const yk_adaptive_desc, d_stats: *const c_void, res_x: u16, res_y: u16, list: *mut yk_pixel_list, out_n: *mut u32, stream: *mut c_void) -> yk_status;
    pub fn yk_adaptive_accumulate(ctx: *mut yk_context, xy: *const u32, n: u32, passes_rgb: *const f32, n_passes: u32, res_x: u16, res_y: u16, film_sum: *mut f32, stats: *mut yk_pixel_stats) -> yk_status;
    pub fn yk_adaptive_accumulate_device(ctx: *mut yk_context, list: *const yk_pixel_list, d_passes_rgb: *const c_void, n_passes: u32, res_x: u16, res_y: u16, d_film_sum: *mut c_void, d_stats: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_adaptive_resolve(ctx: *mut yk_context, film_sum: *const f32, stats: *const yk_pixel_stats, res_x: u16, res_y: u16, out_rgb: *mut f32, out_variance: *mut f32) -> yk_status;
    pub fn yk_adaptive_resolve_device(ctx: *mut yk_context, d_film_sum: *const c_void, d_stats: *const c_void, res_x: u16, res_y: u16, d_out_rgb: *mut c_void, d_out_variance: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_render_pixel_list_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, list: *const yk_pixel_list, n_passes: u32, d_out_rgb: *mut c_void, stream: *mut c_void, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_render_adaptive_device(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, desc: *const yk_adaptive_desc, res_x: u16, res_y: u16, d_film_sum: *mut c_void, d_stats: *mut c_void, stream: *mut c_void, info: *mut yk_adaptive_info, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_write_png(path: *const c_char, width: u32, height: u32, channels: u32, pixels: *const u8) -> yk_status;
    pub fn yk_render_tile(ctx: *mut yk_context, scene: *const yk_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, tile: *const yk_tile, tile_pixels: *mut f32, out_rays: *mut u64) -> yk_status;
    pub fn yk_film_update_tiles_device(ctx: *mut yk_context, tiles: *const yk_tile, n_tiles: usize, d_tile_rgb: *const c_void, res_x: u16, res_y: u16, d_film_rgb: *mut c_void, stream: *mut c_void) -> yk_status;
    pub fn yk_li(ctx: *mut yk_context, scene: *const yk_scene, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, n: usize, ray_o: *const f32, ray_d: *const f32, pixel_xy: *const u16, sample_index: *const u32, dimension: u32, out_li: *mut f32, out_ray_counts: *mut u32) -> yk_status;
    pub fn yk_li_debug(ctx: *mut yk_context, scene: *const yk_scene, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, n: usize, ray_o: *const f32, ray_d: *const f32, pixel_xy: *const u16, sample_index: *const u32, dimension: u32, ray_cap: u32, out_li: *mut f32, out_ray_counts: *mut u32, out_rays: *mut yk_integrator_ray, out_n_rays: *mut u32) -> yk_status;
    pub fn yk_image_texture_load(path: *const c_char, out: *mut yk_texture_desc) -> yk_status;
    pub fn yk_image_texture_free(tex: *mut yk_texture_desc);
    pub fn yk_load_ply(path: *const c_char, split_method: u32, max_shapes_in_node: u32, out: *mut *mut yk_loaded_scene) -> yk_status;
    pub fn yk_load_pbrt(path: *const c_char, split_method: u32, max_shapes_in_node: u32, out: *mut *mut yk_loaded_scene) -> yk_status;
    pub fn yk_load_mitsuba(path: *const c_char, split_method: u32, max_shapes_in_node: u32, out: *mut *mut yk_loaded_scene) -> yk_status;
    pub fn yk_load_scene(path: *const c_char, split_method: u32, max_shapes_in_node: u32, out: *mut *mut yk_loaded_scene) -> yk_status;
    pub fn yk_loaded_scene_get(loaded: *const yk_loaded_scene, desc: *mut yk_scene_desc, camera: *mut yk_camera_params, tile_dim: *mut u16) -> yk_status;
    pub fn yk_loaded_scene_destroy(loaded: *mut yk_loaded_scene);
    pub fn yk_loader_last_error() -> *const c_char;
    // several GPUs of one process (RenderManager's role for GPU workers) and one process per GPU
    pub fn yk_multi_create(devices: *const c_int, n_devices: u32, out: *mut *mut yk_multi) -> yk_status;
    pub fn yk_multi_create_ex(devices: *const c_int, n_devices: u32, flags: u32, out: *mut *mut yk_multi) -> yk_status;
    pub fn yk_multi_deal(res_x: u16, res_y: u16, tile_dim: u16, n_ranks: u32, rank: u32, out: *mut yk_tile, cap: usize, out_pixels: *mut u64) -> usize;
    pub fn yk_multi_destroy(m: *mut yk_multi);
    pub fn yk_multi_device_count(m: *const yk_multi) -> u32;
    pub fn yk_multi_context(m: *mut yk_multi, rank: u32) -> *mut yk_context;
    pub fn yk_multi_set_option(m: *mut yk_multi, key: *const c_char, value: i64) -> yk_status;
    pub fn yk_multi_last_error(m: *const yk_multi, buf: *mut c_char, cap: usize) -> yk_status;
    pub fn yk_multi_scene_create(m: *mut yk_multi, desc: *const yk_scene_desc, out: *mut *mut yk_multi_scene) -> yk_status;
    pub fn yk_multi_scene_destroy(scene: *mut yk_multi_scene);
    pub fn yk_multi_scene_get_info(scene: *const yk_multi_scene, out: *mut yk_scene_info) -> yk_status;
    pub fn yk_multi_film_create(m: *mut yk_multi, res_x: u16, res_y: u16, tile_dim: u16, out: *mut *mut yk_multi_film) -> yk_status;
    pub fn yk_multi_film_destroy(film: *mut yk_multi_film);
    pub fn yk_multi_film_device_ptr(film: *const yk_multi_film) -> *mut c_void;
    pub fn yk_multi_render_film(m: *mut yk_multi, scene: *const yk_multi_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, film: *mut yk_multi_film, film_rgb: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_multi_accumulate_film(m: *mut yk_multi, scene: *const yk_multi_scene, camera: *const yk_camera, sampler: *const yk_sampler_desc, integrator: *const yk_integrator_desc, film: *mut yk_multi_film, first_sample: u32, n_passes: u32, film_rgb: *mut f32, stats: *mut yk_render_stats, cancel: yk_cancel_fn, user: *mut c_void) -> yk_status;
    pub fn yk_multi_film_clear(m: *mut yk_multi, film: *mut yk_multi_film) -> yk_status;
    pub fn yk_multi_interrupt(m: *mut yk_multi) -> yk_status;
    pub fn yk_multi_sync(m: *mut yk_multi) -> yk_status;
    pub fn yk_dist_unique_id(id: *mut u8) -> yk_status;
    pub fn yk_dist_create(ctx: *mut yk_context, id: *const u8, rank: u32, world: u32, out: *mut *mut yk_dist) -> yk_status;
    pub fn yk_dist_destroy(dist: *mut yk_dist);
    pub fn yk_dist_gather(dist: *mut yk_dist, d_send: *const c_void, d_recv: *mut c_void, count: usize, stream: *mut c_void) -> yk_status;
}

/// `yk_last_error` as a `String` (empty when none).
pub fn combiner_last_error(combiner: *const yk_combiner) -> String {
    let mut buf = vec![0u8; 512];
    unsafe { yk_combiner_last_error(combiner, buf.as_mut_ptr() as *mut c_char, buf.len()) };
    let n = buf.iter().position(|&b| b == 0).unwrap_or(buf.len());
    String::from_utf8_lossy(&buf[..n]).into_owned()
}

pub fn last_error(ctx: *const yk_context) -> String {
    let mut buf = vec![0u8; 512];
    unsafe { yk_last_error(ctx, buf.as_mut_ptr() as *mut c_char, buf.len()) };
    let n = buf.iter().position(|&b| b == 0).unwrap_or(buf.len());
    String::from_utf8_lossy(&buf[..n]).into_owned()
}
