/* yuki_hip.h — C ABI of the MI355X-native wavefront Path integrator.
 *
 * Drop-in boundary for the hot path of sndels/yuki: the private Rust trait
 *
 *     trait Integrator { fn li(..); fn render(&self, scratch, scene, camera,
 *         sampler, accumulating, tile, tile_pixels, early_termination_predicate)
 *         -> usize }                    (yuki/src/integrators/mod.rs:92-186)
 *
 * and the data its sibling traits describe (Sampler sampling/mod.rs:46-57,
 * Material materials/mod.rs:20-27, Shape shapes/mod.rs:26-39, Light
 * lights/mod.rs:29-37).  A Rust shim `impl Integrator for HipPath` binds exactly
 * these entry points; our own host code (C++ wrapper
 * yuki_hip.hpp, Python mirror yuki_amd/) and the parity tests call the same ones.
 *
 * Conventions
 *   - plain C, caller-owned buffers, no hidden allocation handed back;
 *   - every call returns a yk_status (the reference panics/asserts instead:
 *     integrators/mod.rs:131,141 -> YK_ERR_INVALID_ARGUMENT);
 *   - matrices are row-major float[16] (math/matrix.rs:16);
 *   - radiance buffers are tightly packed RGB float triples (Spectrum<f32>,
 *     math/spectrum.rs:45-55), tile-major, each tile row-major — the layout of
 *     `tile_pixels[ty*tile_width+tx]` (integrators/mod.rs:177-182);
 *   - the sampler seed is explicit (the reference draws it from thread_rng(),
 *     sampling/uniform.rs:37 — quirk 20 of SURVEY.md).
 */
#ifndef YUKI_HIP_H
#define YUKI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YK_ABI_VERSION 1

typedef enum yk_status {
    YK_OK = 0,
    YK_ERR_INVALID_ARGUMENT = 1, /* contract violation (reference: assert!/panic) */
    YK_ERR_NO_DEVICE = 2,        /* HIP runtime / device unavailable */
    YK_ERR_DEVICE = 3,           /* a HIP call failed; see yk_last_error */
    YK_ERR_OUT_OF_MEMORY = 4,
    YK_ERR_UNSUPPORTED = 5,      /* e.g. Whitted deeper than 16, yk_li with a debug integrator, unsupported file content */
    YK_ERR_BVH_BUILD = 6,        /* reference: assert_ne!(mid,start) bvh.rs:368 */
    YK_ERR_CANCELLED = 7,        /* early_termination_predicate returned true */
    YK_ERR_STACK_OVERFLOW = 8    /* traversal stack > 64, reference: assert bvh.rs:174 */
} yk_status;

/* ---- scene description: flattened, world space, caller owned, read only ---- */

/* shapes/mesh.rs:7-43 — per `Mesh` flags (normals / uvs presence is per mesh) */
typedef struct yk_mesh_desc {
    uint8_t has_normals, has_uvs, swaps_handedness, pad;
} yk_mesh_desc;

/* shapes/sphere.rs:14-35 */
typedef struct yk_sphere_desc {
    float object_to_world[16];
    float world_to_object[16];
    float radius;
    int32_t material;
} yk_sphere_desc;

/* materials/{matte,glass,metal,glossy}.rs with ConstantTexture inputs
 * (textures/constant.rs) folded in */
typedef enum yk_material_kind { YK_MAT_MATTE = 0, YK_MAT_GLASS = 1, YK_MAT_METAL = 2, YK_MAT_GLOSSY = 3 } yk_material_kind;
typedef struct yk_material_desc {
    uint32_t kind;
    float a[3];     /* matte Kd | glass R | metal eta | glossy Rs */
    float b[3];     /*          | glass T | metal k   |           */
    float c;        /* matte sigma (radians) | glass eta | metal/glossy roughness */
    uint32_t flags; /* bit0: remap_roughness ; bit1: matte Kd comes from textures[a_texture] */
    uint32_t a_texture; /* ImageTexture index when bit1 is set (scene/pbrt/mod.rs:887-902) */
} yk_material_desc;
#define YK_MAT_FLAG_REMAP 1u
#define YK_MAT_FLAG_TEXTURED_A 2u

/* textures/image_texture.rs:49-56 `ImageTexture<Spectrum<f32>>`: row-major RGB, row 0 = top
 * row of the image file; evaluated point-sampled, repeat, v flipped (:81-111) */
typedef struct yk_texture_desc {
    uint32_t width, height;
    const float* rgb; /* 3 * width * height */
} yk_texture_desc;

/* lights/{point,spot,distant,rectangular}_light.rs — build with yk_make_*_light */
typedef enum yk_light_kind { YK_LIGHT_POINT = 0, YK_LIGHT_SPOT = 1, YK_LIGHT_DISTANT = 2, YK_LIGHT_RECT = 3 } yk_light_kind;
typedef struct yk_light_desc {
    uint32_t kind;
    float p[3]; /* point/spot position ; distant: direction w */
    float i[3]; /* intensity (point/spot) | radiance (distant/rect) */
    float cos_total_width, cos_falloff_start;
    float world_to_light[16];      /* spot */
    float sample_to_world[16];     /* rect */
    float sample_to_world_inv[16]; /* rect */
    float area;                    /* rect */
} yk_light_desc;

typedef enum yk_split_method { YK_SPLIT_SAH = 0, YK_SPLIT_MIDDLE = 1, YK_SPLIT_EQUAL_COUNTS = 2 } yk_split_method;

/* scene/mod.rs:41-49 `Scene` + SceneLoadSettings (:25-39) */
typedef struct yk_scene_desc {
    uint32_t n_vertices;
    const float* points;  /* 3*n_vertices, world space (Mesh::new pre-transforms, mesh.rs:27-33) */
    const float* normals; /* 3*n_vertices or NULL */
    const float* uvs;     /* 2*n_vertices or NULL */
    uint32_t n_triangles;
    const uint32_t* indices;       /* 3*n_triangles */
    const uint32_t* tri_mesh;      /* n_triangles -> meshes[] */
    const int32_t* tri_material;   /* n_triangles -> materials[] */
    const int32_t* tri_area_light; /* n_triangles -> lights[] or -1 (Triangle.area_light, triangle.rs:22) */
    uint32_t n_meshes;
    const yk_mesh_desc* meshes;
    uint32_t n_spheres; /* shape ids: triangles first, then spheres (see shape_order) */
    const yk_sphere_desc* spheres;
    uint32_t n_materials;
    const yk_material_desc* materials;
    uint32_t n_lights;
    const yk_light_desc* lights;
    float background[3];
    uint32_t split_method;       /* yk_split_method */
    uint32_t max_shapes_in_node; /* scene/mod.rs:36 default 1 */
    /* Order in which the shapes enter BoundingVolumeHierarchy::new (Scene.shapes, which the
     * pbrt loader fills in file order): n_triangles + n_spheres entries, entry < n_triangles
     * = that triangle, otherwise sphere (entry - n_triangles).  NULL = triangles, then spheres. */
    const uint32_t* shape_order;
    uint32_t n_textures;
    const yk_texture_desc* textures;
} yk_scene_desc;

/* camera.rs:19-22 `Camera` = two Transforms */
typedef struct yk_camera {
    float camera_to_world[16], camera_to_world_inv[16];
    float raster_to_camera[16], raster_to_camera_inv[16];
} yk_camera;

/* camera.rs:24-30 `CameraParameters` + the film resolution Camera::new reads */
typedef struct yk_camera_params {
    float position[3], target[3], up[3];
    uint32_t fov_axis; /* 0 = FoV::X, 1 = FoV::Y */
    float fov_degrees;
    uint16_t res_x, res_y;
} yk_camera_params;

/* sampling/mod.rs:16-19 `SamplerType` */
typedef enum yk_sampler_kind { YK_SAMPLER_UNIFORM = 0, YK_SAMPLER_STRATIFIED = 1 } yk_sampler_kind;
typedef struct yk_sampler_desc {
    uint32_t kind;
    uint32_t nx, ny; /* uniform: nx = pixel_samples ; stratified: pixel_samples.{x,y} */
    uint32_t jitter; /* stratified jitter_samples */
    uint64_t seed;   /* rng_seed */
} yk_sampler_desc;

/* integrators/mod.rs:33-40 `IntegratorType` */
typedef enum yk_integrator_kind {
    YK_INTEGRATOR_WHITTED = 0, /* whitted.rs:39-181; max_depth <= 16 on the device */
    YK_INTEGRATOR_PATH = 1,
    YK_INTEGRATOR_BVH_INTERSECTIONS = 2,
    YK_INTEGRATOR_GEOMETRY_NORMALS = 3,
    YK_INTEGRATOR_SHADING_NORMALS = 4,
    YK_INTEGRATOR_SHADING_UVS = 5 /* shading_uvs.rs: (uv.x, uv.y, 0) on a hit, black on a miss */
} yk_integrator_kind;
typedef struct yk_integrator_desc {
    uint32_t kind;
    uint32_t max_depth;   /* path.rs:20-23 Params */
    uint32_t has_clamp;   /* indirect_clamp.is_some() */
    float indirect_clamp;
} yk_integrator_desc;

/* film.rs:43-65 `FilmTile.bb` (Bounds2<u16>, max exclusive) */
typedef struct yk_tile {
    uint16_t x0, y0, x1, y1;
} yk_tile;

/* bvh.rs:536-556 — the reference's 32-byte node, exported for inspection/tests */
typedef struct yk_bvh_node {
    float bmin[3], bmax[3];
    uint32_t a;     /* interior: second_child_index ; leaf: first_shape_index */
    uint16_t count; /* leaf: shape_count */
    uint8_t axis, is_leaf;
} yk_bvh_node;

typedef struct yk_scene_info {
    uint64_t n_nodes, n_interior, n_shapes;
    float bounds_min[3], bounds_max[3];
    double build_seconds, upload_seconds;
    uint64_t device_bytes;
    uint32_t max_leaf_shapes, tree_depth;
} yk_scene_info;

/* How a scene's tree was built (yk_scene_get_build_info). */
enum {
    YK_BVH_BUILDER_HOST = 0,        /* the host recursion (the reference's, node for node) */
    YK_BVH_BUILDER_DEVICE = 1,      /* the level-synchronous builder on the device: the same tree */
    YK_BVH_BUILDER_HOST_LEVELS = 2  /* the host instance of the level algorithm (environment YK_BVH_BUILDER=levels) */
};
enum {                                /* why a build that was asked for the level builder ran the host recursion */
    YK_BVH_REASON_NONE = 0,
    YK_BVH_REASON_SPLIT_METHOD = 1,   /* YK_SPLIT_EQUAL_COUNTS: its select_nth over the whole array is sequential */
    YK_BVH_REASON_NON_FINITE = 2,     /* a shape bound or centroid is not finite */
    YK_BVH_REASON_SELECT_NTH = 3,     /* a range longer than max(bvh_small_range, 2) needed the equal-counts fallback */
    YK_BVH_REASON_TOO_MANY_NODES = 4, /* more than 2^28 nodes or shapes */
    YK_BVH_REASON_OUT_OF_MEMORY = 5,  /* the builder could not get its device memory */
    YK_BVH_REASON_DEVICE_ERROR = 6    /* a HIP call of the builder failed */
};
typedef struct yk_bvh_build_info {
    uint32_t builder;      /* YK_BVH_BUILDER_* : who produced the tree */
    uint32_t reason;       /* YK_BVH_REASON_* : non-zero when the level builder was asked for and not used */
    uint32_t levels;       /* levels the level phase ran */
    uint32_t small_range;  /* the small-range limit S in effect */
    uint64_t small_ranges; /* ranges finished by the small-range path */
    double seconds_upload;    /* shape bounds to the device, primitive array */
    double seconds_levels;    /* level phase */
    double seconds_small;     /* small-range phase */
    double seconds_layout;    /* depth-first numbering, interior boxes */
    double seconds_copy_back; /* nodes and shape order to the host */
} yk_bvh_build_info;

typedef struct yk_render_stats {
    uint64_t rays;          /* closest-hit rays == the reference's ray_count (path.rs:87) */
    uint64_t shadow_rays;   /* any-hit rays, not part of the metric */
    uint64_t samples;       /* camera samples rendered */
    double seconds_total;   /* first launch -> film resolved (device time, HIP events) */
    double seconds_trace;   /* summed duration of the closest-hit traversal launches */
    double seconds_shadow;  /* summed duration of the any-hit traversal launches */
    double seconds_shade;   /* summed duration of the shade (BSDF+NEE) launches */
    uint32_t trace_launches, batches;
    uint32_t shadow_launches, reserved; /* any-hit traversal launches (two on bounces whose shadow rays are split) */
} yk_render_stats;

typedef struct yk_context yk_context;
typedef struct yk_scene yk_scene;

/* early_termination_predicate (integrators/mod.rs:129,153: the reference polls it once per pixel
 * sample; render_worker.rs:240-255 relies on that for "low latency kills").  Returning non-zero
 * aborts the render with YK_ERR_CANCELLED (tile contents undefined, as in render_worker.rs:252-255).
 * When is it polled:
 *   - before every batch is enqueued (all calls);
 *   - in a SYNCHRONOUS call — one that returns pixels to the host or is given `stats` — about every
 *     100 us while the GPU works.  On a non-zero answer a word in pinned host memory is set; one
 *     wave of every running traversal launch reads it whenever it claims work, raises a word in
 *     device memory and poisons the launch's queue head, so no wave claims again; every kernel (every
 *     block of the grid-stride ones) reads the device word when it starts and finds its queue
 *     empty; a job of many batches is enqueued two batches at a time.  The call returns after the
 *     drain (3-5 ms into a 1.5-s job; ~10 ms for a context's first interruption).  The next render on the context is unaffected.
 *   - an ASYNCHRONOUS submission (device output, stats == NULL) has returned before the GPU
 *     started: the caller interrupts it with yk_context_interrupt from any thread.
 * The predicate is called from the thread that made the call, never concurrently. */
typedef int (*yk_cancel_fn)(void* user);

/* ---- library / context ---------------------------------------------------- */
uint32_t yk_abi_version(void);
const char* yk_status_string(yk_status s);
yk_status yk_context_create(int device, yk_context** out);
void yk_context_destroy(yk_context* ctx);
/* ctx NULL: the message of the calling thread's last failed call that took no context (a host-only scene); reading clears it. */
yk_status yk_last_error(const yk_context* ctx, char* buf, size_t cap);
/* The hipStream_t every entry point of this context runs on when it is given no stream of the
 * caller's (a render also uses a side stream that joins it again before the call's last launch).
 * Lets a caller order its own device work — a collective, a film read-back — after a render
 * without a second stream: wrap the handle (torch.cuda.ExternalStream, hipStreamWaitEvent ...).
 * Owned by the context; NULL for a NULL context. */
void* yk_context_stream(const yk_context* ctx);
/* Stop what the context has enqueued (see yk_cancel_fn): callable from any thread while another one is
 * inside a render call on the same context.  Kernels stop at their next look at the word; the context's next
 * submission first waits for the interrupted one to drain. */
yk_status yk_context_interrupt(yk_context* ctx);
/* tuning knobs (none changes any result): "batch_paths" (camera samples per batch, 64 .. 2^29),
 * "streams" (1|2 work sets), "sample_buf_cap" (bytes), "time_kernels" (0 | 1: per-kernel
 * seconds in yk_render_stats for jobs of at least 2^20 samples | 2: always),
 * "packet_bounces" / "packet_shadow_bounces" (leading bounces traced by the wave-packet
 * kernels), "overlap_shadow" (0|1), "shade_reorder" (0|1: paths of a shade block dealt to
 * lanes by material kind), "nee_skip" (a bit mask, 0 | 2, default 2: bit 2 — a shadow ray whose contribution
 * is +-0 in every component is counted in shadow_rays but not traced; 0 traces every ray), "top_nodes" (tree-top nodes the traversal kernels keep
 * in LDS, 0..1023; the kernels hold at most what they were built for), "wide_bvh" (0: binary nodes only | 1: traverse the 4-wide collapse of the
 * BVH | 2, default: keep both, jobs of up to 6 M paths use the 4-wide one), "bvh_builder" (0, default: the
 * tree is built by the host recursion | 1: by the level-synchronous builder on the device where the input
 * qualifies — YK_SPLIT_SAH or YK_SPLIT_MIDDLE, finite bounds, no long range that needs select_nth — and by
 * the host recursion otherwise; the tree is the same either way, yk_scene_get_build_info says which ran)
 * and "bvh_small_range" (0 .. 2^20, default 32: ranges of at most this many shapes are finished by one
 * lane each), "scene_layout" (0, default: the traversal records are laid out from the tree on the host and uploaded |
 * 1: on the device, from the builder's tree in place or from an uploaded host-built one — the same bytes either way,
 * yk_scene_get_layout_info says which ran; a device-built, device-laid scene copies its 32-byte nodes back only when
 * yk_scene_export_bvh, yk_scene_node_bounds or a "trace_stage_kernel" stage call asks for them) — the last five apply
 * to scenes created afterwards; "overlay_coop_min" (1 .. 65536, default 32: box
 * edges of at least this many pixels are drawn by a whole wave in yk_overlay_draw[_device], shorter ones by one lane);
 * "denoise_lds_max_step" (0 | 1 | 2, default 2: the a-trous iterations of yk_denoise[_device] with a step up to this
 * stage their taps in LDS, the others read global memory); "update_top_block" (0 | 1, default 1: the device route of
 * yk_scene_update finishes the tree's top levels of at most 256 nodes each with one block instead of a launch per level);
 * "albedo_mean_band_rows" (0 .. 65535, default 0: the output rows yk_render_albedo_mean[_device] traces and reduces at a
 * time; 0 = as many as fit its 64 MiB scratch); "exposure_wave_combine" (0 | 1, default 1: in the exposure meter's
 * histogram pass a wave whose lanes all hit one bin adds to it once instead of once a lane; the counts are the same).  Test hook: "trace_stage_kernel" (0, default: yk_trace_closest /
 * yk_trace_any run the generic kernels as documented | 1: the generic kernels in the render loop's
 * flavour | 2: the wave-packet kernels; modes 1 and 2 report shape ids and verdicts only, and
 * refuse out_t, out_bary, counters, a closest-hit t_max and, in mode 2, a tree deeper than 64
 * with YK_ERR_INVALID_ARGUMENT). */
yk_status yk_context_set_option(yk_context* ctx, const char* key, int64_t value);

/* ---- host-side restatements (no GPU needed) -------------------------------- */
/* Camera::new, camera.rs:52-102 */
yk_status yk_camera_init(const yk_camera_params* params, yk_camera* out);
/* film_tiles / generate_tiles / outward_spiral, film.rs:299-376,409-475.
 * Returns the number of tiles; writes min(cap, n) of them in spiral order. */
size_t yk_film_tiles(uint16_t res_x, uint16_t res_y, uint16_t tile_dim, yk_tile* out, size_t cap);
/* RectangularLight::new rectangular_light.rs:31-42, SpotLight::new spot_light.rs:20-36,
 * PointLight::new point_light.rs:18-24 */
yk_status yk_make_rect_light(const float light_to_world[16], const float light_to_world_inv[16], const float radiance[3],
                             const float size[2], yk_light_desc* out);
yk_status yk_make_spot_light(const float light_to_world[16], const float light_to_world_inv[16], const float intensity[3],
                             float total_width_degrees, float falloff_start_degrees, yk_light_desc* out);
yk_status yk_make_point_light(const float light_to_world[16], const float intensity[3], yk_light_desc* out);
/* Film::update_tile (film.rs:210-282), host buffers: tile-major -> row-major film */
yk_status yk_film_update_tiles(const yk_tile* tiles, size_t n_tiles, const float* tile_rgb, uint16_t res_x, uint16_t res_y,
                               float* film_rgb);

/* ---- scene ------------------------------------------------------------------ */
/* BoundingVolumeHierarchy::new (bvh.rs:39-115) on the host, then upload.
 * ctx may be NULL: host-only scene (BVH build/export without a GPU).
 * A scene (and a yk_tile_list) is read-only after creation and belongs to the DEVICE of `ctx`:
 * any context on that device may render it, also concurrently from several threads — two
 * contexts with their own streams keep two renders in flight, so the latency tail of one
 * overlaps the bulk of the next.  Destroy it only after every render that uses
 * it has completed (the library does not reference-count scenes). */
yk_status yk_scene_create(yk_context* ctx, const yk_scene_desc* desc, yk_scene** out);
/* The same scene from geometry that is in device memory already: a tensor of the caller's, the output of its own kernel,
 * the next frame of an animation.  `desc` is read as by yk_scene_create, except that its large arrays — points, normals,
 * uvs, indices, tri_mesh, tri_material, tri_area_light, shape_order — are DEVICE pointers on ctx's device (the same ones
 * may be NULL); meshes, spheres, materials, lights and textures with their texels stay host pointers.  `stream` is the
 * hipStream_t on which the caller produced the arrays (NULL: nothing to wait for): the context's stream waits for an event
 * recorded there and all work runs on the context's stream.  The call is synchronous; on return the caller may free or
 * overwrite its arrays — the scene owns device-to-device copies — and the scene is an ordinary one for every entry point.
 * Nothing of O(n) runs on the host and no geometry crosses the host link: the per-triangle checks, the permutation test
 * of shape_order and the shape bounds are kernels (their first error, in the order and with the message of
 * yk_scene_create, is read back before any kernel follows an index), and the device builder and the device layout run
 * whatever "bvh_builder" and "scene_layout" say ("bvh_small_range", "top_nodes" and "wide_bvh" apply).  Where the builder
 * or the layout refuses (yk_scene_get_build_info / yk_scene_get_layout_info say who ran and why), the geometry is copied
 * to the host once and yk_scene_create's path builds the same scene.  A triangle coordinate that is NaN or infinite counts
 * as YK_BVH_REASON_NON_FINITE here, also where the fold of the bound would drop the NaN.  The host copies of the tree and of the per-shape
 * material kinds are fetched on the first call that reads them.  YK_ERR_INVALID_ARGUMENT: ctx NULL; a large array that
 * is not device memory of this context's device (checked with hipPointerGetAttributes before anything is launched) or
 * whose allocation ends before its count does; whatever yk_scene_create refuses. */
yk_status yk_scene_create_device(yk_context* ctx, const yk_scene_desc* desc, void* stream, yk_scene** out);
/* Update in place: the scene's vertices move, its tree is refitted and its records are rewritten ("Update in
 * place").  `points` holds 3 floats for each of the scene's n_vertices (the count of its description); `normals` is the
 * same size, or NULL to keep the normals the scene has — non-NULL for a scene created without normals is
 * YK_ERR_INVALID_ARGUMENT.  Indices and uvs do not change (spheres, lights and materials change through
 * yk_scene_apply_edit, below), and neither does the tree's
 * topology: every node keeps its children, split axis, leaf flag, first slot and count, and the leaf order stays.  A leaf's
 * box is folded from its shapes in leaf order (a triangle's bound from the new points, a sphere's as the scene has it), an
 * interior node's from its two children in child order, and all seven record buffers, yk_scene_info.bounds_min/max and the
 * layout info's scalars follow.  A scene updated with its own points is byte for byte what it was.  A rectangular light's
 * record is not moved: vertices of triangles that carry an area light are the caller's business.  The tree's depth stays
 * too: rays that overflow the 64-entry traversal stack of a tree deeper than that (YK_ERR_STACK_OVERFLOW) still do.
 *   yk_scene_update        host arrays.  It follows the scene's layout (yk_scene_get_layout_info): a device-laid scene
 *                          uploads the arrays and takes the device route, a host-laid one refits on the host
 *                          (yk_bvh_refit), lays the records out there and uploads them.  ctx may be NULL for a host-only
 *                          scene: its tree is refitted.
 *   yk_scene_update_device DEVICE pointers on ctx's device, produced on `stream` (a hipStream_t, NULL: nothing to wait for),
 *                          checked as yk_scene_create_device checks its arrays, with the same messages.  It always takes
 *                          the device route: leaf boxes, one launch per tree level bottom-up and the layout's own kernels.
 *                          Where an allocation or a HIP call fails there, the arrays are copied to the host once and the
 *                          host route runs; yk_scene_get_update_info says so.  Both routes write the same bytes.
 * All or nothing: the arguments are tested before anything of the scene is written, and a refused update leaves every
 * buffer of the scene untouched.  Every coordinate of `points` must be finite ("points: coordinate not finite",
 * YK_ERR_INVALID_ARGUMENT) — deliberately stricter than creation, which hands such geometry to the host builder.
 * Ordering: the call holds the context's lock, waits for `stream` as yk_scene_create_device does and for everything this
 * context has enqueued — renders of this scene enqueued on it before the call finish on the old geometry — and returns when
 * the records are complete.  Renders of the scene from ANOTHER context or a combiner are the caller's to order: none may be
 * in flight during the call.  After a device-route update the host copy of the tree is stale: yk_scene_export_bvh,
 * yk_scene_node_bounds and the "trace_stage_kernel" stage calls fetch the refitted one on their next call.  Scenes of a
 * yk_multi cannot be updated (no entry point takes one). */
yk_status yk_scene_update(yk_context* ctx, yk_scene* scene, const float* points, const float* normals);
yk_status yk_scene_update_device(yk_context* ctx, yk_scene* scene, const float* d_points, const float* d_normals, void* stream);
enum { YK_UPDATE_ROUTE_HOST = 0, YK_UPDATE_ROUTE_DEVICE = 1 };
typedef struct yk_scene_update_info {
    uint32_t n_updates;    /* updates that were carried out (refused ones do not count) */
    uint32_t route;        /* YK_UPDATE_ROUTE_* of the last update */
    uint32_t reason;       /* YK_LAYOUT_REASON_* : non-zero when the last update asked for the device route and ran on the host */
    uint32_t n_levels;     /* device route: launches of the level pass (the depth of the deepest interior node) */
    uint64_t plan_bytes;   /* device memory the update state keeps (tree, depths, level lists, small tables); built on the
                            * first device-route update and added to yk_scene_info.device_bytes */
    double seconds_check, seconds_boxes, seconds_records, seconds_total; /* last update: the finite test (with the copy of
                            * the arrays into the scene), leaf and interior boxes, the seven record buffers, the whole call */
} yk_scene_update_info;
yk_status yk_scene_get_update_info(const yk_scene* scene, yk_scene_update_info* out);
/* Edit in place: the scene's spheres, lights, materials and background change; its triangles stay ("Edit in
 * place").  Every table of `edit` is either NULL (keep what the scene has) or holds as many records as the scene was
 * created with: counts never change.  Neither does a light's kind (tri_area_light binds triangles to rectangular lights
 * and the count of delta lights sizes the work buffers).  A material's kind may change and so may a sphere's material.
 * What is rewritten follows from what changed:
 *   lights, or materials whose device BSDF kinds all stay   that device table only: no refit, no record pass;
 *   a material's device BSDF kind changed                   also the scene's kind tables and its record buffers, by the
 *                                                            layout's own code (the tree stays);
 *   spheres                                                 also the device sphere table, the spheres' world bounds
 *                                                            (Sphere::world_bound), the refit of yk_scene_update with
 *                                                            those bounds, and the records;
 *   background                                              the scene's constant.
 * After an edit of lights, materials or background the scene is byte for byte the scene yk_scene_create makes of the
 * edited description with the same options; after a sphere edit it is the refitted one (the tree's topology stays, as
 * after yk_scene_update).  An edit with the scene's own tables changes no byte of it.
 * All or nothing, checked before anything of the scene is written, YK_ERR_INVALID_ARGUMENT each: "null edit"; "spheres
 * given as a host table and as a device table"; "lights: a light's kind cannot change"; "sphere material out of range" and
 * "material texture index out of range" (yk_scene_create's checks); "spheres: matrix entry or radius not finite".
 * Triangles that carry a rectangular light are not moved by an edit of that light: to move one consistently, call
 * yk_scene_update with the moved vertices of its two triangles and yk_scene_apply_edit with the moved light record (either
 * order, nothing rendered in between).
 *   yk_scene_apply_edit         host tables.  It follows the scene's layout as yk_scene_update does: a device-laid scene
 *                               refits and lays out on the device, a host-laid one on the host.  ctx may be NULL for a
 *                               host-only scene.
 *   yk_scene_apply_edit_device  the same with the sphere table in DEVICE memory: n_spheres yk_sphere_desc records at a
 *                               4-byte aligned address on ctx's device, produced on `stream`; edit->spheres must be NULL.
 *                               One kernel checks the records (a flag word, read back before anything is written) and
 *                               writes the device sphere table, the bounds and the material column.  It takes the device
 *                               route and falls back to the host route with a recorded reason, as yk_scene_update_device.
 * Ordering and staleness are yk_scene_update's: the call drains the context's streams first, so renders enqueued before it
 * finish on the old scene; after a device-route sphere edit the host copy of the tree is stale until something reads it.
 * Still out of reach of an edit: counts, light kinds, indices, the vertices of rectangular-light triangles, and scenes of a
 * yk_multi (no entry point takes one). */
typedef struct yk_scene_edit {
    const yk_sphere_desc* spheres;      /* the scene's n_spheres records, or NULL: keep */
    const yk_light_desc* lights;        /* the scene's n_lights records, or NULL: keep */
    const yk_material_desc* materials;  /* the scene's n_materials records, or NULL: keep */
    const float* background;            /* 3 floats, or NULL: keep */
} yk_scene_edit;
enum { YK_EDIT_LIGHTS = 1, YK_EDIT_MATERIALS = 2, YK_EDIT_SPHERES = 4, YK_EDIT_BOXES = 8, YK_EDIT_RECORDS = 16, YK_EDIT_BACKGROUND = 32 };
typedef struct yk_scene_edit_info {
    uint32_t n_edits;  /* edits that were carried out (refused ones do not count) */
    uint32_t route;    /* YK_UPDATE_ROUTE_* of the last edit */
    uint32_t reason;   /* YK_LAYOUT_REASON_* : non-zero when the last edit asked for the device route and ran on the host */
    uint32_t rewrote;  /* YK_EDIT_* bits: what the last edit rewrote */
    double seconds_check, seconds_tables, seconds_boxes, seconds_records, seconds_total; /* last edit: the checks, the small
                        * tables, leaf and interior boxes, the seven record buffers, the whole call */
} yk_scene_edit_info;
yk_status yk_scene_apply_edit(yk_context* ctx, yk_scene* scene, const yk_scene_edit* edit);
yk_status yk_scene_apply_edit_device(yk_context* ctx, yk_scene* scene, const yk_scene_edit* edit, const void* d_spheres, void* stream);
yk_status yk_scene_get_edit_info(const yk_scene* scene, yk_scene_edit_info* out);
/* Transform in place: every mesh of the scene is placed by a matrix, relative to its REST POSE ("Transform in
 * place"; the rule: yuki_amd/csrc/yk_scene_transform.h).  `transforms` holds one yk_mesh_transform for each of the scene's
 * n_meshes (the count of its description), row-major.  The pair is the caller's, as a sphere's pair is: the library does not
 * invert.  The rest pose is the points and normals the scene had after its last yk_scene_create* or yk_scene_update*; the
 * first transform after either keeps a copy of them (and the table vertex -> mesh, built from indices and tri_mesh).
 * Transforms are ABSOLUTE, not cumulative: A then B is B, and the identity afterwards restores the rest pose's bytes.
 * Per vertex, by the record of the one mesh whose triangles index it (a vertex no triangle indexes keeps its rest bits):
 *   rest_to_world == identity, entry by entry (-0 counts as 0)   the rest pose's BITS; world_to_rest is not read;
 *   otherwise                                                    p' = Transform * Point3 of rest_to_world (with its w == 1
 *                                                                test and division), n' = Transform * Normal through
 *                                                                world_to_rest — not renormalised, as Mesh::new does not;
 *                                                                normals only where the scene has a normals array.
 * A non-identity record whose rest_to_world swaps handedness (the sign of its upper 3 x 3 determinant) flips the mesh's
 * swaps_handedness flag relative to creation's: the records are what a scene created with the mirrored mesh would get.
 * After the points are written the call is yk_scene_update's: the refit (topology and leaf order stay), the seven record
 * buffers, bounds_min / bounds_max.  yk_scene_update* afterwards resets the flags to creation's and drops the rest copy.
 * All or nothing, checked before a byte of the scene is written, YK_ERR_INVALID_ARGUMENT each; where two hold at once the
 * message is the first of this list (the precedence is fixed, on both routes):
 *   NULL arguments; a scene that is not this context's;
 *   "transforms: matrix entry not finite"                     either matrix of a non-identity record, or rest_to_world of any;
 *   "transforms: a mesh that carries an area light cannot move"  a non-identity record for a mesh with a triangle whose
 *                                                             tri_area_light >= 0: the rectangular light's record is not
 *                                                             moved by this call (the limit of yk_scene_update stays);
 *   "transforms: vertex shared by two meshes"                 a vertex indexed by triangles of two different meshes;
 *   "points: coordinate not finite"                           a RESULT is not finite (a scale of 1e38 overflows).  Normals
 *                                                             are never tested, as yk_scene_update does not test them.
 *   yk_scene_transform         a host table.  It follows the scene's layout as yk_scene_update does; ctx may be NULL for a
 *                              host-only scene (its tree is refitted; it keeps no normals).
 *   yk_scene_transform_device  the table in DEVICE memory of ctx's device, 4-byte aligned, produced on `stream`, checked as
 *                              yk_scene_create_device checks its arrays.  It always takes the device route: one kernel per
 *                              mesh table, a check pass that computes every result and sets only a flag word (read back
 *                              once), a write pass that computes again and writes points, normals and mesh flags — the
 *                              arithmetic is deterministic, so no third copy of the geometry is staged — then
 *                              yk_scene_update's refit and records.  It falls back to the host route with a recorded
 *                              reason, as yk_scene_update_device.  Both routes write the same bytes.
 * tree_cost: a refit keeps the topology, so a mesh moved across the scene leaves a worse tree.  After the refit the call
 * computes, in binary64, ( sum over interior nodes of A(n) + sum over leaves of A(n) * count(n) ) / A(root), A = 2 (dx dy +
 * dy dz + dz dx) of the node's float box converted to double; 0 when A(root) is not > 0.  tree_cost_rest is the same number
 * for the tree as it stood when the rest pose was kept (a sphere edit between transforms changes the tree and not this
 * number: it is refreshed only by the first transform after yk_scene_create* or yk_scene_update*).  Both are relative to
 * their own root's area: a move that grows the root can lower tree_cost while the tree gets worse; to compare across such
 * moves multiply by the area of yk_scene_info.bounds_min/max.  A scene in device memory keeps its rest copy there on either
 * route (the motion pass reads it); a copy that does not fit fails the call, YK_ERR_OUT_OF_MEMORY.  The device sums in
 * blocks and the host in node order; the terms are equal bit for bit, so the two differ by at most n_nodes * 2^-51 relative.
 * Ordering, locking and the staleness of the host tree after a device-route call are yk_scene_update's.  Limits: meshes
 * that carry a rectangular light do not move; the tree's topology is not rebuilt; no instancing (one record per mesh, every
 * vertex in one mesh); counts and indices stay; scenes of a yk_multi cannot be transformed (no entry point takes one). */
typedef struct yk_mesh_transform {
    float rest_to_world[16];
    float world_to_rest[16];
} yk_mesh_transform;   /* 128 bytes */
typedef struct yk_scene_transform_info {
    uint32_t n_transforms;     /* transforms that were carried out (refused ones do not count) */
    uint32_t route;            /* YK_UPDATE_ROUTE_* of the last transform */
    uint32_t reason;           /* YK_LAYOUT_REASON_* : non-zero when the last transform asked for the device route and ran on the host */
    uint32_t n_moved_meshes;   /* non-identity records of the last transform */
    uint32_t n_flipped_meshes; /* of those, records that swap handedness */
    uint32_t reserved;
    uint64_t rest_bytes;       /* the rest copy (points, normals), the table vertex -> mesh and the small per-mesh and cost
                                * words; for a scene in device memory they live there, on either route, and are counted in
                                * yk_scene_info.device_bytes, once; for a host-only scene they are host bytes */
    double tree_cost, tree_cost_rest;
    double seconds_check, seconds_points, seconds_boxes, seconds_records, seconds_total; /* last transform: the rest copy (first
                                * call) and the check pass, the write pass, leaf and interior boxes, the records, the whole call */
} yk_scene_transform_info;
yk_status yk_scene_transform(yk_context* ctx, yk_scene* scene, const yk_mesh_transform* transforms);
yk_status yk_scene_transform_device(yk_context* ctx, yk_scene* scene, const void* d_transforms, void* stream);
yk_status yk_scene_get_transform_info(const yk_scene* scene, yk_scene_transform_info* out);
/* The refit rule on the host, over an exported tree (yk_scene_export_bvh): the boxes of `nodes` are recomputed in place
 * from shape_bounds — six floats (min.xyz, max.xyz) per SOURCE shape, n_shapes of them — leaves folded from the default
 * bounds in leaf order through shape_order, interior nodes from their children in descending array index.  Nothing else
 * of a node is written.  YK_ERR_INVALID_ARGUMENT: a NULL array, or a link, slot or shape index out of range. */
yk_status yk_bvh_refit(yk_bvh_node* nodes, size_t n_nodes, const uint32_t* shape_order, size_t n_shapes, const float* shape_bounds);
void yk_scene_destroy(yk_scene* scene);
yk_status yk_scene_get_info(const yk_scene* scene, yk_scene_info* out);
/* nodes: n_nodes entries in the reference's depth-first layout; shape_order:
 * n_shapes source indices in leaf order (bvh.rs:96).  Either may be NULL. */
yk_status yk_scene_export_bvh(const yk_scene* scene, yk_bvh_node* nodes, uint32_t* shape_order);
/* Which builder produced the scene's tree, why the device builder was not used when "bvh_builder" asked
 * for it, and the seconds of its phases (zero for the host recursion; yk_scene_info.build_seconds is the
 * whole build whichever builder ran).  A fallback is silent for the result and visible here only.
 * Scenes of a yk_multi (yk_multi_scene_create) are always built by the host recursion. */
yk_status yk_scene_get_build_info(const yk_scene* scene, yk_bvh_build_info* out);
/* Where a scene's traversal records (the 64-byte nodes, the two LDS tree tops, the 4-wide collapse, the leaf-order
 * tris / prim_shade / prim_attr) were laid out — "scene_layout" of yk_context_set_option — and what the traversal
 * kernels are handed with them.  A device layout that fails falls back to the host layout: the scene is valid and
 * `reason` says why.  Scenes of a yk_multi are always laid out on the host. */
enum { YK_LAYOUT_HOST = 0, YK_LAYOUT_DEVICE = 1 };
enum {
    YK_LAYOUT_REASON_NONE = 0,
    YK_LAYOUT_REASON_OUT_OF_MEMORY = 1, /* the layout could not get its device memory */
    YK_LAYOUT_REASON_DEVICE_ERROR = 2,  /* a HIP call of the layout failed */
    YK_LAYOUT_REASON_MULTI = 3          /* a scene of a yk_multi */
};
typedef struct yk_scene_layout_info {
    uint32_t layout;       /* YK_LAYOUT_* : who laid the records out */
    uint32_t reason;       /* YK_LAYOUT_REASON_* : non-zero when the device layout was asked for and not used */
    double seconds_upload; /* device layout: the tree (when the host built it) and the small tables to the device */
    double seconds_layout; /* device layout: the layout kernels */
    uint32_t tree_fetched; /* 1 once the host copy of the 32-byte nodes and the shape order exists (always 1 for a host-built tree;
                            * a device-built, device-laid scene copies them back on the first call that reads them) */
    uint32_t root_ref, n_top, n_top_any, wide, wide_auto; /* DevScene's root reference and tree-top sizes; whether the 4-wide
                                                           * nodes exist and whether they serve small jobs only ("wide_bvh" = 2) */
} yk_scene_layout_info;
yk_status yk_scene_get_layout_info(const yk_scene* scene, yk_scene_layout_info* out);
/* Test hook: one of the scene's device record buffers copied back, however it was laid out.  *n_bytes receives the
 * buffer's size; with out == NULL that is all, otherwise cap_bytes must be at least that (YK_ERR_INVALID_ARGUMENT). */
enum { YK_RECORDS_NODES = 0, YK_RECORDS_NODES4 = 1, YK_RECORDS_TOP = 2, YK_RECORDS_TOP_ANY = 3, YK_RECORDS_TRIS = 4, YK_RECORDS_PRIM_SHADE = 5, YK_RECORDS_PRIM_ATTR = 6 };
yk_status yk_scene_read_records(const yk_scene* scene, uint32_t which, void* out, size_t cap_bytes, size_t* n_bytes);
/* Test hooks: the host instance of the two order rules of the device layout (yuki_amd/csrc/yk_scene_layout.h) over an
 * exported tree of n nodes.  yk_layout_top_order: the reference node indices of the tree top of at most `cap` nodes,
 * breadth first; returns their number (out_order: cap entries).  yk_layout_wide_slots: the DevNode4 index of every
 * reference node the 4-wide collapse keeps, 0xffffffff for the others; returns the number of DevNode4 (0: leaf root). */
size_t yk_layout_top_order(const yk_bvh_node* nodes, size_t n, uint32_t cap, uint32_t* out_order);
size_t yk_layout_wide_slots(const yk_bvh_node* nodes, size_t n, uint32_t* out_slot_per_node);
/* Test hook: the partition step of the level builder on its own.  pass[i] says whether the element at
 * position i passes the predicate; `order` (n words, in and out) is rearranged exactly as the two-ended
 * swap partition of the host recursion (itertools::partition) would.  Returns the number passing. */
size_t yk_bvh_partition_plan(const uint8_t* pass, size_t n, uint32_t* order);

/* ---- the hot path -------------------------------------------------------------- */
/* Integrator::render for a batch of tiles (integrators/mod.rs:120-185, non-accumulating
 * film).  out_rgb: host buffer, tile-major, 3 floats per pixel. */
yk_status yk_render_tiles(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                          const yk_integrator_desc* integrator, const yk_tile* tiles, size_t n_tiles, float* out_rgb,
                          yk_render_stats* stats, yk_cancel_fn cancel, void* user);
/* Same, radiance left in device memory (d_out_rgb: device pointer, same layout)
 * on `stream` (a hipStream_t, NULL = the context's stream).  Asynchronous unless
 * stats != NULL. */
yk_status yk_render_tiles_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera,
                                 const yk_sampler_desc* sampler, const yk_integrator_desc* integrator, const yk_tile* tiles,
                                 size_t n_tiles, void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel,
                                 void* user);
/* Integrator::render(accumulating = true) (integrators/mod.rs:146-161; the tile queue of
 * render_manager.rs:135-143): ONE sample per pixel whose global sample index is the tile's
 * FilmTile.sample (tile_samples[t], u16 like film.rs:52, which must be below the sampler's
 * samples per pixel as in render_manager.rs:135-143 — YK_ERR_INVALID_ARGUMENT otherwise); the
 * raw radiance is stored (divided by 1).  Fold the result into the film with yk_film_accumulate_tiles[_device]; the displayed
 * image is film / samples (tonemap.rs:240-241), which yk_tone_map computes. */
yk_status yk_render_tiles_accumulating(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                       const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles,
                                       float* out_rgb, yk_render_stats* stats, yk_cancel_fn cancel, void* user);
yk_status yk_render_tiles_accumulating_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                              const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples,
                                              size_t n_tiles, void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel,
                                              void* user);
/* Film::update_tile with `samples` present (film.rs:260-272): film += tile pixels and
 * tile_sample_counts[t] += 1 (position t in `tiles` plays FilmTile.index; may be NULL). */
yk_status yk_film_accumulate_tiles(const yk_tile* tiles, size_t n_tiles, const float* tile_rgb, uint16_t res_x, uint16_t res_y, float* film_rgb,
                                   uint32_t* tile_sample_counts);
yk_status yk_film_accumulate_tiles_device(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, const void* d_tile_rgb, uint16_t res_x,
                                          uint16_t res_y, void* d_film_rgb, void* stream);
/* A tile list prepared once and reused every frame — what a GPU worker does with the film's
 * tile queue (render_manager.rs:125-143).  The list keeps a device-resident pixel table, so
 * yk_render_tile_list_device (with stats == NULL) and yk_film_update_tile_list_device enqueue
 * their work on `stream` and return without any host synchronisation; results are identical
 * to the yk_tile-array entry points.  tile_samples != NULL makes it an accumulating-film list
 * (FilmTile.sample per tile). */
typedef struct yk_tile_list yk_tile_list;
yk_status yk_tile_list_create(yk_context* ctx, const yk_tile* tiles, const uint16_t* tile_samples, size_t n_tiles, yk_tile_list** out);
void yk_tile_list_destroy(yk_tile_list* list);
yk_status yk_render_tile_list_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                     const yk_integrator_desc* integrator, const yk_tile_list* list, void* d_out_rgb, void* stream,
                                     yk_render_stats* stats, yk_cancel_fn cancel, void* user);
yk_status yk_film_update_tile_list_device(yk_context* ctx, const yk_tile_list* list, const void* d_tile_rgb, uint16_t res_x, uint16_t res_y,
                                          void* d_film_rgb, void* stream, int accumulate);
/* Several passes of the accumulating film in ONE submission: passes FilmTile.sample,
 * FilmTile.sample + 1, ... + n_passes - 1 of every tile (what render_manager.rs:125-143 does by
 * re-queueing the tiles n_passes times).  A single 1080p pass is 2 M camera rays — every launch
 * of it lasts as long as its longest ray — so an interactive GPU worker renders a handful of
 * passes per submission (8 passes: 2.6x the rays per second of pass-by-pass).
 * out: n_passes x (pixels of the list) x RGB, pass-major; each pass is bit for bit what the
 * one-pass call with that sample index returns.  yk_film_accumulate_tile_list_passes_device
 * adds them to the film pass after pass (film.rs:260-272), so the film equals the one n_passes
 * single submissions would have produced. */
yk_status yk_render_tiles_accumulating_passes(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                              const yk_integrator_desc* integrator, const yk_tile* tiles, const uint16_t* tile_samples,
                                              size_t n_tiles, uint32_t n_passes, float* out_rgb, yk_render_stats* stats, yk_cancel_fn cancel,
                                              void* user);
yk_status yk_render_tile_list_passes_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                            const yk_integrator_desc* integrator, const yk_tile_list* list, uint32_t n_passes, void* d_out_rgb,
                                            void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user);
/* The same for a PLAIN tile list (tile_samples == NULL) whose tiles all stand at the same sample: passes first_sample ..
 * first_sample + n_passes - 1 of every tile — the worker's accumulate loop (render_manager.rs:125-143 re-queues all
 * tiles with the next sample index) without a new list per pass. */
yk_status yk_render_tile_list_samples_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                             const yk_integrator_desc* integrator, const yk_tile_list* list, uint32_t first_sample,
                                             uint32_t n_passes, void* d_out_rgb, void* stream, yk_render_stats* stats, yk_cancel_fn cancel,
                                             void* user);
yk_status yk_film_accumulate_tile_list_passes_device(yk_context* ctx, const yk_tile_list* list, const void* d_passes_rgb, uint32_t n_passes,
                                                     uint16_t res_x, uint16_t res_y, void* d_film_rgb, void* stream);

/* Film output (app/util.rs:90-111 write_exr -> exr::prelude::write_rgb_file): an OpenEXR 2
 * scan-line file with three FLOAT channels B, G, R, uncompressed, increasing Y — readable by
 * the tools the reference targets (readme.md:46-47); and a little-endian PFM ("PF") writer.
 * pixels: row-major RGB, row 0 = top. */
yk_status yk_write_exr(const char* path, uint32_t width, uint32_t height, const float* rgb);
yk_status yk_write_pfm(const char* path, uint32_t width, uint32_t height, const float* rgb);

/* ---- tone map (app/renderpasses/tonemap.rs; what `yuki --out` writes, app/headless.rs:62-84) ----------
 * The film the reference writes to its EXR is, unless the settings say Raw, the tone-mapped one (ToneMapType,
 * default Filmic { exposure: 1.0 }, tonemap.rs:40-51).  The shader arithmetic is fixed to one evaluation order
 * (binary32, every operation separate and left to right, no FMA, correctly rounded divisions); the rules are
 * stated next to the tonemap.rs lines they come from in yuki_amd/csrc/yk_tonemap.h.  In short:
 *   Filmic (FILMIC_FS_CODE :318-385): divide by (float)samples[flat] when > 0, where flat = (y / tile_dim) *
 *     (res_x / tile_dim, FLOOR) + x / tile_dim indexes a table laid out over the CEIL grid (FilmTile.index) — the
 *     reference's own mismatch when res_x % tile_dim != 0, reproduced; then * exposure, ACESInputMat, RRTAndODTFit,
 *     ACESOutputMat, saturate(x) = x > 0 ? (x < 1 ? x : 1) : 0 (NaN -> 0).
 *   Heatmap (HEATMAP_FS_CODE :387-422): maps texel[channel] for Green / Blue and LUMINANCE for Red and Luminance
 *     (the shader's `channel > 0 && channel < 3`), while yk_film_min_max reads red for Red (find_min_max :447-472) —
 *     reproduced.  Bounds not given: find_min_max over the film first (headless.rs:135-145).
 *   Raw: the film unchanged (:163). */
typedef enum yk_tone_map_kind { YK_TONE_MAP_RAW = 0, YK_TONE_MAP_FILMIC = 1, YK_TONE_MAP_HEATMAP = 2 } yk_tone_map_kind;
typedef enum yk_heatmap_channel { YK_HEATMAP_RED = 0, YK_HEATMAP_GREEN = 1, YK_HEATMAP_BLUE = 2, YK_HEATMAP_LUMINANCE = 3 } yk_heatmap_channel;
typedef struct yk_tone_map_desc {
    uint32_t kind;       /* yk_tone_map_kind */
    float exposure;      /* Filmic */
    uint32_t channel;    /* Heatmap: yk_heatmap_channel */
    uint32_t has_bounds; /* Heatmap: 0 = find_min_max over the film */
    float bounds[2];     /* Heatmap (min, max) when has_bounds */
} yk_tone_map_desc;
/* Host buffers, row-major RGB (h, w, 3).  ctx NULL = the host instance on the CPU (like yk_scene_create), else on
 * ctx's device (synchronous).  tile_dim: Film::tile_dim() (film.rs:143-150) — the width of the first tile of the
 * film's spiral queue, 16 without tiles (tonemap.rs:238).  samples: Film.samples, ceil(res_x/tile_dim) *
 * ceil(res_y/tile_dim) u32 in FilmTile.index order (film.rs:299-331), or NULL for a film that does not accumulate
 * (no division).  used_bounds: the Heatmap bounds applied, may be NULL.  out_rgb may equal film_rgb.
 * YK_ERR_INVALID_ARGUMENT: unknown kind or channel, tile_dim 0, a zero resolution, NULL film or out. */
yk_status yk_tone_map(yk_context* ctx, const yk_tone_map_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y,
                      uint16_t tile_dim, const uint32_t* samples, float* out_rgb, float* used_bounds);
/* The same on device buffers (e.g. yk_multi_film_device_ptr, a film updated with yk_film_update_tile_list_device),
 * enqueued on `stream` (NULL = the context's) without waiting for the device: a Heatmap without bounds finds them on
 * the device and the map reads them there.  `samples` is a HOST table, copied before the call returns (through the
 * context's pinned staging: a call that brings a table waits for the previous call's upload of one, if that has not
 * run yet).  d_out_rgb may equal d_film_rgb.  The tone map's work buffers belong to the context: calls on one context
 * are ordered only when they share a stream.  Allocates on first use only. */
yk_status yk_tone_map_device(yk_context* ctx, const yk_tone_map_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                             uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream);
/* find_min_max (tonemap.rs:447-472) over a host film: the fold from (FLT_MAX, -FLT_MAX) that skips NaN pixels; red,
 * green, blue or luminance ((0.2126*r + 0.7152*g) + 0.0722*b).  ctx NULL = CPU.  The sign of a zero bound is not
 * specified. */
yk_status yk_film_min_max(yk_context* ctx, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint32_t channel, float out_min_max[2]);

/* ---- exposure meter (the project's own; the reference's exposure is a slider, tonemap.rs:12-22) ----------
 * A 256-bin integer histogram of the film's luminances chooses the Filmic exposure; the rule is stated in full in
 * yuki_amd/csrc/yk_exposure.h and is integer arithmetic up to one division, so the host and the device instance agree bit
 * for bit whatever the order of the device's additions.  In short:
 *   pixel: r, g, b divided by (float)samples[flat] when > 0 (the tone map's step 1, same lookup), Y = (0.2126*r +
 *     0.7152*g) + 0.0722*b.  Y not finite or <= 0: counted in `skipped` only.
 *   bin = clamp((bits(Y) >> 20) - 888, 0, 255): eight bins to a stop over 2^-16 <= Y < 2^16; values below go to bin 0 and
 *     `below`, values above to bin 255 and `above`.  A bin's value in Q16 stops is ((bin >> 3) - 16) * 65536 + Q[bin & 7],
 *     Q = {5732, 16248, 25711, 34312, 42196, 49472, 56229, 62534}: at most 0.0875 stop from any luminance in the bin.
 *   window {x0, y0, x1, y1}, half open: pixels outside are neither counted nor skipped.
 *   cut: of the N counted samples in bin order, the lowest (N * low_cut) >> 16 and the highest (N * high_cut) >> 16 are
 *     dropped (cuts in units of 1/65536); log2_metered = (float)((double)S / ((double)K * 65536.0)) over the K kept ones.
 *   adapt: log2_adapted = prev.log2_adapted + (log2_metered - prev.log2_adapted) * (adapt_up when the difference is > 0,
 *     else adapt_down); without a previous state, or with prev.frames == 0, log2_adapted = log2_metered.  N == 0 carries
 *     the previous state, or gives log2_adapted = ev_bias and frames = 0 without one.
 *   exposure = 2^clamp(ev_bias - log2_adapted, min_ev, max_ev) by a fixed polynomial (relative error below 1e-5).
 *     ev_bias is log2 of the key (0.18) plus any compensation. */
typedef struct yk_exposure_desc {
    uint32_t low_cut, high_cut; /* units of 1/65536; low_cut + high_cut < 65536 */
    float ev_bias, min_ev, max_ev, adapt_up, adapt_down; /* -24 <= min_ev <= max_ev <= 24; rates in [0, 1] */
    uint16_t window[4]; /* x0, y0, x1, y1: x0 < x1 <= res_x, y0 < y1 <= res_y */
} yk_exposure_desc;
typedef struct yk_exposure_state {
    float exposure, log2_adapted, log2_metered;
    uint32_t frames, counted, skipped, below, above;
} yk_exposure_state;
/* The histogram alone, host film (as yk_tone_map's: ctx NULL = the host instance, samples may be NULL).  window NULL =
 * the whole film.  out_bins and out_skipped_below_above may each be NULL, not both.
 * YK_ERR_INVALID_ARGUMENT: NULL film, a zero resolution, tile_dim 0, an empty window or one outside the film. */
yk_status yk_film_histogram(yk_context* ctx, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                            const uint16_t window[4], uint32_t out_bins[256], uint32_t out_skipped_below_above[3]);
/* Meter a host film: *out from the film and *prev (NULL: no history; may equal out).  ctx NULL = the host instance.
 * YK_ERR_INVALID_ARGUMENT also for a descriptor outside the ranges above. */
yk_status yk_exposure_meter(yk_context* ctx, const yk_exposure_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                            const uint32_t* samples, const yk_exposure_state* prev, yk_exposure_state* out);
/* The same on a device film, enqueued on `stream` (NULL = the context's) without waiting: d_prev (NULL: no history) and
 * d_out_state are yk_exposure_state records in device memory, 4-byte aligned, and may be the same record, so a chain of
 * frames never touches the host.  `samples` is a HOST table as for yk_tone_map_device.  Allocates on first use only. */
yk_status yk_exposure_meter_device(yk_context* ctx, const yk_exposure_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                                   uint16_t tile_dim, const uint32_t* samples, const void* d_prev, void* d_out_state, void* stream);
/* yk_tone_map_device for Filmic with the exposure desc->exposure * d_state->exposure (one binary32 multiply), the
 * record read on the device when the kernel runs.  YK_ERR_INVALID_ARGUMENT: any kind but Filmic, a NULL or misaligned
 * d_state, and what yk_tone_map_device refuses. */
yk_status yk_tone_map_metered_device(yk_context* ctx, const yk_tone_map_desc* desc, const void* d_state, const void* d_film_rgb, uint16_t res_x,
                                     uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream);

/* Exactly the trait method: one tile, returns the ray count through *out_rays. */
yk_status yk_render_tile(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                         const yk_integrator_desc* integrator, const yk_tile* tile, float* tile_pixels, uint64_t* out_rays);
/* Film::update_tile on the device: scatter tile-major radiance into a row-major
 * film (both device pointers).  Used on rank 0 after the RCCL gather. */
yk_status yk_film_update_tiles_device(yk_context* ctx, const yk_tile* tiles, size_t n_tiles, const void* d_tile_rgb,
                                      uint16_t res_x, uint16_t res_y, void* d_film_rgb, void* stream);
/* Integrator::li (integrators/mod.rs:94-101) for n caller-supplied rays; the
 * sampler is started at (pixel, sample_index) and advanced by `dimension`
 * draws already consumed by the caller (2 for a camera ray).  out_ray_counts (may be NULL): the closest-hit rays of every
 * sample (RadianceResult::ray_scene_intersections) for Whitted; zeros for Path, whose wavefront keeps no per-sample
 * count (yk_li_debug reports it). */
yk_status yk_li(yk_context* ctx, const yk_scene* scene, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator,
                size_t n, const float* ray_o, const float* ray_d, const uint16_t* pixel_xy, const uint32_t* sample_index,
                uint32_t dimension, float* out_li, uint32_t* out_ray_counts);

/* Integrator::li_debug (integrators/mod.rs:103-115): the rays of a sample, each with its type (mod.rs:83-90) */
typedef enum yk_ray_type { YK_RAY_DIRECT = 0, YK_RAY_REFLECTION = 1, YK_RAY_REFRACTION = 2, YK_RAY_NORMAL = 3, YK_RAY_SHADOW = 4 } yk_ray_type;
typedef struct yk_integrator_ray {
    float o[3];
    float d[3];
    float t_max;
    uint32_t ray_type; /* yk_ray_type (IntegratorRay::ray_type; `type` is a Rust keyword) */
} yk_integrator_ray;   /* 32 bytes */
#define YK_LI_DEBUG_MAX_RECORDS (1u << 24) /* largest n * ray_cap yk_li_debug accepts */
/* Integrator::li_debug for n caller-supplied rays; the sampler is started as in yk_li.  Path only (other kinds:
 * YK_ERR_UNSUPPORTED, as the reference's Whitted and debug integrators keep the trait default).  Returns li, the
 * closest-hit ray count of every sample (ray_scene_intersections; may be NULL) and its records in Path::li_internal's
 * push order (path.rs:71-149): every traced segment (Direct, then Reflection or Refraction by the sampled lobe; t_max =
 * the hit t, else the camera ray's own t_max or the exit through the BVH root box), a Normal record (si.p, si.n) after
 * each hit, and a Shadow record (VisibilityTester::ray) for every light whose li is non-black and that has a visibility
 * tester.  Normal records and segments that miss the root box have t_max = min_debug_ray_length (path.rs:58-62).
 * out_rays: n * ray_cap records, sample-major (unused slots zero; may be NULL when ray_cap == 0); out_n_rays[i] is the
 * number of records sample i produced and may exceed ray_cap (then only ray_cap were written).
 * ray_cap = max_depth * (2 + n_lights) always suffices; n * ray_cap must not exceed YK_LI_DEBUG_MAX_RECORDS. */
yk_status yk_li_debug(yk_context* ctx, const yk_scene* scene, const yk_sampler_desc* sampler, const yk_integrator_desc* integrator,
                      size_t n, const float* ray_o, const float* ray_d, const uint16_t* pixel_xy, const uint32_t* sample_index,
                      uint32_t dimension, uint32_t ray_cap, float* out_li, uint32_t* out_ray_counts,
                      yk_integrator_ray* out_rays, uint32_t* out_n_rays);

/* ---- the overlays of draw_visualizations (app/window.rs:1033-1063) ------------
 * RayVisualization (app/renderpasses/ray_visualization.rs) and BvhVisualization (bvh_visualization.rs) draw GL lines into
 * the tone-mapped film, rays first, then boxes.  GL fixes no bit-level result for a line; the rule fixed here is stated
 * in yuki_amd/csrc/yk_overlay.h (binary32, no FMA: clip coordinates, clipping to the view volume, one pixel per major-axis
 * pixel centre, the last primitive in list order wins a pixel), and the host and the device instance agree bit for bit. */
/* BoundingVolumeHierarchy::node_bounds (bvh.rs:121-157): the root box first when target_level <= 0, then the breadth-first
 * walk from (node 0, level 1) that pushes both children's boxes of every interior node at target_level (at every level when
 * target_level < 0): -1 gives n_nodes boxes, 0 the root alone.  Six floats a box (p_min, p_max).  Returns the number of
 * boxes and writes min(cap, n) of them; out_bounds may be NULL.  A host function: works on a scene made without a device. */
size_t yk_scene_node_bounds(const yk_scene* scene, int32_t target_level, float* out_bounds, size_t cap);
/* The `world_to_clip` both passes build (ray_visualization.rs:80-150, bvh_visualization.rs:101-171), row-major:
 * flip_y * (camera_to_clip * look_at), with zf the largest distance from the camera to a corner of scene_bounds (p_min,
 * p_max of scene.bvh.bounds(), the root box) and zn = zf * 1e-5.  params->res_x / res_y: FilmSettings.res.  A host function.
 * YK_ERR_INVALID_ARGUMENT: a non-finite bound, zf == 0, a degenerate look_at, a non-finite matrix entry. */
yk_status yk_overlay_world_to_clip(const yk_camera_params* params, const float scene_bounds[6], float out[16]);
typedef struct yk_overlay_line {
    float p0[3], p1[3], rgb[3];
} yk_overlay_line; /* 36 bytes: a world-space segment and its colour */
/* RayVisualization::set_rays (:28-56): p0 = o, p1 = o + d * t_max per component, the colour by type (Direct white,
 * Reflection red, Refraction green, Normal blue, Shadow yellow).  The reference indexes its vertices with u16, so
 * more than 32,768 rays (or an unknown type) is YK_ERR_INVALID_ARGUMENT.  A host function. */
yk_status yk_overlay_ray_lines(const yk_integrator_ray* rays, size_t n, yk_overlay_line* out);
/* Draws the lines, then the boxes (six floats each, as yk_scene_node_bounds writes them: expanded into the reference's 8
 * corners and 12 edges, red for an even array index, green for an odd one) into a row-major RGB film (h, w, 3) on the
 * host.  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).  Pixels no primitive covers keep
 * their bits.  YK_ERR_INVALID_ARGUMENT: NULL matrix or film, a zero resolution, a NULL list with a non-zero count,
 * n_lines + 12 * n_boxes above 2^32 - 2. */
yk_status yk_overlay_draw(yk_context* ctx, const float world_to_clip[16], const yk_overlay_line* lines, size_t n_lines, const float* boxes,
                          size_t n_boxes, float* film_rgb, uint16_t res_x, uint16_t res_y);
/* The same on device buffers, in place in d_film_rgb (4-byte alignment suffices), enqueued on `stream` (NULL = the
 * context's) without waiting for the device.  The id buffer the passes share belongs to the context and is allocated on
 * first use (and when a larger film comes): calls on one context are ordered only when they share a stream. */
yk_status yk_overlay_draw_device(yk_context* ctx, const float world_to_clip[16], const void* d_lines, size_t n_lines, const void* d_boxes,
                                 size_t n_boxes, void* d_film_rgb, uint16_t res_x, uint16_t res_y, void* stream);

/* ---- present: ScaleOutput::draw (app/renderpasses/scale_output.rs), the last pass of a frame (app/window.rs:246-270) ----
 * The tone-mapped film stretched into the window with bilinear filtering, the aspect ratio kept inside a letterbox,
 * sRGB-encoded, as an 8-bit frame.  GL fixes no bit-level result for a textured quad; the rule fixed here is stated next
 * to the scale_output.rs lines it comes from in yuki_amd/csrc/yk_present.h, and the host and the device instance agree
 * bit for bit.  In short (binary32, every operation separate, no FMA):
 *   Rectangle (:64-84, the reference's u32 arithmetic): frame_aspect < texture_aspect: scaled_height = (W*h)/w, full
 *     width, centred vertically with the larger margin ABOVE when the difference is odd; otherwise scaled_width =
 *     (H*w)/h, full height, centred with the larger margin on the right.  Film row 0 is the top row.  Coverage is
 *     exactly that integer rectangle; it may be empty.
 *   Texture coordinate, exact: n = (2*(i - x0) + 1)*w - width, d = 2*width, first tap floor(n / d), neighbour's weight
 *     (float)(n mod d) / (float)d; rows alike.  Identity and integer magnification have exact taps.
 *   Filter (:58-62): Linear both ways, 2 x 2 taps, no mip levels; BorderClamp with GL's border (0, 0, 0), so a magnified
 *     film has a dark half-texel fringe (reproduced).  mix(x, y, a) = a == 0 ? x : x*(1 - a) + y*a, horizontal mixes
 *     first; a tap of weight zero is not read.  A NaN an operation produces is 0x7fc00000; a copied value keeps its bits.
 *   Encode: NONE = the shader's output with gamma_before_output == 0; SHADER = its linearToSRGB (:154-158), x <=
 *     0.0031308 ? 12.92*x : 1.055*pow(x, 1/2.2) - 0.055; SRGB = what an sRGB back buffer stores (the reference's default,
 *     window.rs:94-127): 0 for x <= 0 or NaN, 12.92*x below 0.0031308, 1.055*pow(x, 0.41666) - 0.055 below 1, else 1.
 *     pow(x, y) = exp(y * log(x)) with the library's own logf / expf.
 *   Frame: RGBA8 = (uint8_t)(saturate(x)*255 + 0.5) per channel (NaN -> 0), alpha 255, the clear colour (0, 0, 0, 255)
 *     outside the rectangle (window.rs:247), rows top-down, bytes R, G, B, A.  RGB32F = the three floats before
 *     quantisation, 0 outside. */
typedef enum yk_present_encode { YK_PRESENT_ENCODE_NONE = 0, YK_PRESENT_ENCODE_SHADER = 1, YK_PRESENT_ENCODE_SRGB = 2 } yk_present_encode;
typedef enum yk_present_format { YK_PRESENT_RGBA8 = 0, YK_PRESENT_RGB32F = 1 } yk_present_format;
typedef struct yk_present_desc {
    uint16_t window_x, window_y; /* the window (frame.get_dimensions()) */
    uint32_t encode;             /* yk_present_encode */
    uint32_t format;             /* yk_present_format */
} yk_present_desc;               /* 12 bytes */
typedef struct yk_present_rect {
    int32_t x0, y0;         /* top-down window coordinates of the first column and row */
    uint32_t width, height; /* either may be 0 */
} yk_present_rect;
/* The target rectangle of a res_x x res_y film in a window_x x window_y window, unclipped.  A host function.
 * YK_ERR_INVALID_ARGUMENT: a zero dimension, NULL out. */
yk_status yk_present_target_rect(uint16_t res_x, uint16_t res_y, uint16_t window_x, uint16_t window_y, yk_present_rect* out);
/* Host buffers: film_rgb row-major RGB (res_y, res_x, 3); out (window_y, window_x) pixels of 4 bytes (RGBA8) or of three
 * floats (RGB32F).  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).
 * YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero film or window dimension, an unknown encode or format, an output that
 * overlaps the film. */
yk_status yk_present(yk_context* ctx, const yk_present_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, void* out);
/* The same on device buffers, enqueued on `stream` (NULL = the context's): one kernel writes every window pixel, the
 * letterbox included; no host synchronisation, no allocation, no work buffer.  d_film_rgb and d_out need 4-byte
 * alignment (anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched). */
yk_status yk_present_device(yk_context* ctx, const yk_present_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                            void* d_out, void* stream);
/* An 8-bit PNG: channels 3 (RGB) or 4 (RGBA), non-interlaced, filter type 0 on every row, the data in stored deflate
 * blocks.  pixels: row-major, row 0 = top, `channels` bytes a pixel — what yk_present writes as RGBA8.  Host only.
 * YK_ERR_INVALID_ARGUMENT: NULL path or pixels, a zero dimension, channels other than 3 or 4, a file that cannot be written. */
yk_status yk_write_png(const char* path, uint32_t width, uint32_t height, uint32_t channels, const uint8_t* pixels);

/* ---- denoise: first-hit guides and an edge-avoiding a-trous filter, between the film and the tone map ----
 * The reference shows its raw Monte-Carlo film; this pass is the library's own.  The filter is the edge-avoiding a-trous
 * wavelet transform (Dammertz et al., HPG 2010) with a colour stop, a normal stop and a plane-distance stop.  Its rule is
 * stated next to each expression in yuki_amd/csrc/yk_denoise.h, and the host and the device instance agree bit for bit.
 * In short (binary32, every operation separate, no FMA, exp = the library's expf, a NaN an operation produces is
 * 0x7fc00000):
 *   Input: the film's RGB; with a sample table every channel is divided by (float)samples[flat] where that count is > 0,
 *     flat by the tone map's index rule (floor / ceil mismatch included).
 *   Iteration i = 0 .. iterations-1, step s = 1 << i, colour scale sigma_color / (float)(1 << i); every iteration reads
 *     the previous iteration's colours of all pixels.  iterations = 0 returns the normalised film, copied as bits.
 *   Taps: dy = -2..2 outside, dx = -2..2 inside, Q = P + s*(dx, dy), skipped outside the film; h = k[|dx|]*k[|dy|] with
 *     k = (3/8, 1/4, 1/16).  The centre tap has weight h alone.  Any other tap: w = h*exp(-e), e = (a_c + a_n) + a_p,
 *     a_c = ((dr*dr + dg*dg) + db*db) / (sigma_c,i * sigma_c,i); both hits: a_n = |ns_P - ns_Q|^2 / sigma_normal^2 and
 *     a_p = d*d / sigma_plane^2 with d = dot(ns_P, p_Q - p_P); both misses: a_n = a_p = 0; a hit and a miss: w = 0.
 *     A tap whose weight is 0 or NaN is skipped, so an infinite or NaN pixel stays where it is and does not spread.
 *   Output: sum(w * c_Q) / sum(w) per channel. */
typedef struct yk_guide {
    float ns[3]; /* si.shading.n as the ShadingNormals integrator reads it (not halved, not offset); 0 on a miss */
    float hit;   /* 1.0f on a hit, 0.0f on a miss */
    float p[3];  /* si.p; 0 on a miss */
    float t;     /* Hit.t; 0 on a miss */
} yk_guide;      /* 32 bytes: a filter tap is two 16-byte loads */
typedef struct yk_denoise_desc {
    uint32_t iterations; /* 0 .. 8 */
    float sigma_color, sigma_normal, sigma_plane; /* each > 0; +inf switches its stop off */
} yk_denoise_desc;
/* The guides of a res_x x res_y film, row-major: one ray per pixel through the pixel centre, Camera::ray((x + 0.5, y + 0.5)),
 * traced by the render loop's closest-hit kernels; spheres are served like triangles.  Synchronous, `out` is a host array
 * of res_x * res_y records.  YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero resolution, a scene of another device. */
yk_status yk_render_guides(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y, yk_guide* out);
/* The same into device memory (16-byte aligned), ordered on `stream` (NULL = the context's) without waiting on the host.
 * Guides depend on the camera and the scene only: render them again when either changes, not with every pass. */
yk_status yk_render_guides_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y,
                                  void* d_guides, void* stream);
/* Host buffers: film_rgb and out_rgb row-major RGB (res_y, res_x, 3), guides res_x * res_y records; `samples` = Film.samples
 * in FilmTile.index order (ceil(res_x / tile_dim) * ceil(res_y / tile_dim) entries) or NULL for a film that does not
 * accumulate.  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).  out_rgb may equal film_rgb.
 * YK_ERR_INVALID_ARGUMENT: iterations > 8, a sigma that is <= 0 or NaN, a NULL pointer, a zero resolution, tile_dim 0,
 * guides that overlap the output, an output that overlaps the film without being equal to it. */
yk_status yk_denoise(yk_context* ctx, const yk_denoise_desc* desc, const float* film_rgb, const yk_guide* guides, uint16_t res_x,
                     uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb);
/* The same on device buffers, enqueued on `stream` (NULL = the context's) without waiting for the device: one launch per
 * iteration.  `samples` is a HOST table (copied before the call returns, through the same pinned staging as the tone
 * map's).  The two ping-pong buffers between iterations (16 bytes a pixel each) belong to the context: allocated on first
 * use and again when a larger film comes.  d_film_rgb and d_out_rgb need 4-byte alignment, d_guides 16-byte alignment
 * (anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched).  d_out_rgb may equal d_film_rgb.
 * Context option "denoise_lds_max_step" (0, 1 or 2, default 2): iterations with a step up to it stage their taps in LDS. */
yk_status yk_denoise_device(yk_context* ctx, const yk_denoise_desc* desc, const void* d_film_rgb, const void* d_guides, uint16_t res_x,
                            uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream);

/* ---- temporal: the film across camera moves — reprojected history, between the film and the denoiser ----
 * The reference clears its film when the camera moves; these two passes are the library's own.  "Reproject" carries the
 * history of the previous view (a mean and a sample count per pixel) to the current view through the first-hit guides of
 * both; "blend" folds the current view's film into it.  The rule is stated next to each expression in
 * yuki_amd/csrc/yk_temporal.h; the host and the device instance agree bit for bit (binary32, every operation separate, no
 * FMA, a NaN an operation produces is 0x7fc00000, a value that is only copied keeps its bits).
 * Intended use: while a camera stands, every displayed frame is blend(R, film, samples) with R reprojected ONCE when the
 * camera moved (R NULL before the first move); the last blend's history output is the next move's previous history, and
 * the guides of that view are its previous guides.  Downstream passes take the blended RGB with samples = NULL.
 * Reprojected radiance is exact for diffuse surfaces only: on glass and metal it lags the view.  max_history is the
 * loosest bound on that lag (a new sample always weighs at least m / (max_history + m)); yk_history_rectify, run before
 * the blend, is the tight one: it clips a history the current frame contradicts and shrinks its count.
 * Reproject, current pixel P with guide G[P]:
 *   1. G[P] a miss: the all-zero record.
 *   2. p_cam = camera_to_world_inv' . p_P, r = raster_to_camera_inv' . p_cam (the point transform of Camera::ray; ' = the
 *      previous camera).  The homogeneous w of the second transform <= 0 or NaN: zero record.
 *   3. fx = r.x - 0.5, fy = r.y - 0.5; NaN, < -1 or >= (float)res on either axis: zero record.  x0 = floor(fx), ax = fx - x0.
 *   4. Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), b = (1 - ax | ax) * (1 - ay | ay).  A tap is skipped when it lies
 *      outside the film, b == 0, its previous guide is a miss, its n is <= 0 or NaN, a channel of it is NaN or infinite,
 *      d = dot(ns_P, p_Q - p_P) has |d| > plane_tolerance or is NaN, or dot(ns_P, ns_Q) < normal_cos_min or is NaN.
 *   5. sw = sum b over the taps taken; 0: zero record; else rgb = sum(b * c_Q) / sw, n = sum(b * n_Q) / sw.
 * Blend, per pixel: m = (float)samples[flat] (the tone map's index rule) or 1 without a table; c = the film's RGB, divided
 *   by m with a table where m > 0; n = min(h.n, max_history).  The history is absent when the pointer is NULL, n is <= 0
 *   or NaN, or a channel of h is not finite; the current view when m == 0.  Both absent: zeros.  Only the history absent:
 *   (c, m).  Only the current view absent: (h.rgb, n).  Neither: t = n + m, rgb = (n*h + m*c) / t, the record is (rgb, t). */
typedef struct yk_history {
    float rgb[3]; /* the mean radiance */
    float n;      /* the effective number of samples behind it; 0 = no history */
} yk_history;     /* 16 bytes; 16-byte aligned on the device */
typedef struct yk_temporal_desc {
    float plane_tolerance; /* scene units, > 0; +inf switches the plane test off */
    float normal_cos_min;  /* [-1, 1] */
    float max_history;     /* >= 1 */
} yk_temporal_desc;
/* Host buffers: res_x * res_y records each, row-major.  ctx NULL = the host instance on the CPU, else on ctx's device
 * (synchronous).  YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero resolution, a parameter out of range or NaN, an output
 * that overlaps any input. */
yk_status yk_history_reproject(yk_context* ctx, const yk_temporal_desc* desc, const yk_history* prev_history, const yk_guide* prev_guides,
                               const yk_camera* prev_camera, const yk_guide* guides, uint16_t res_x, uint16_t res_y, yk_history* out_history);
/* The same on device buffers (all 16-byte aligned; anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched), enqueued
 * on `stream` (NULL = the context's) without waiting for the device: one launch, no allocation.  The camera is read before
 * the call returns. */
yk_status yk_history_reproject_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_prev_history, const void* d_prev_guides,
                                      const yk_camera* prev_camera, const void* d_guides, uint16_t res_x, uint16_t res_y, void* d_out_history,
                                      void* stream);
/* film_rgb row-major RGB (res_y, res_x, 3); `samples` and tile_dim as yk_denoise takes them; history may be NULL; either
 * output may be NULL, not both.  out_history may equal history and out_rgb may equal film_rgb.
 * YK_ERR_INVALID_ARGUMENT: a NULL desc or film, a zero resolution, tile_dim 0, a parameter out of range or NaN, both outputs
 * NULL, an output that overlaps an input without being equal to its own counterpart, outputs that overlap each other. */
yk_status yk_history_blend(yk_context* ctx, const yk_temporal_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y,
                           uint16_t tile_dim, const uint32_t* samples, const yk_history* history, yk_history* out_history, float* out_rgb);
/* The same on device buffers, enqueued on `stream` (NULL = the context's) without waiting for the device: one launch.
 * `samples` is a HOST table (copied before the call returns, through the pinned staging of the tone map and the denoiser);
 * its device copy belongs to the context, allocated on first use and again when a larger table comes.  d_film_rgb and
 * d_out_rgb need 4-byte alignment, the histories 16-byte alignment (anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched). */
yk_status yk_history_blend_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                                  uint16_t tile_dim, const uint32_t* samples, const void* d_history, void* d_out_history, void* d_out_rgb,
                                  void* stream);

/* ---- motion: the film across moves of the geometry — surface ids, previous positions, reprojection through them ----
 * After yk_scene_update a pixel's first hit lies on a surface point that stood somewhere else in the previous frame, so
 * yk_history_reproject (which projects the CURRENT position into the previous camera) carries the wrong history or none.
 * Three passes, the library's own; the rule is stated next to each expression in yuki_amd/csrc/yk_motion.h and
 * yk_temporal.h, and the host and the device instance agree bit for bit (binary32, every operation separate, no FMA, a NaN
 * an operation produces is 0x7fc00000, a value that is only copied keeps its bits).
 * Intended use: the caller keeps the vertex array it gave to the previous yk_scene_update (or to creation): the scene
 * copies what it is given.  Then: update(new) -> yk_render_guides_ids -> yk_surface_motion(prev_points = the OLD array)
 * -> yk_history_reproject_moved -> blend, denoise, tone map as after a camera move.
 * Ids: one trace per view, the guide pass itself; the id is the identity of the first hit: the source shape as
 *   yk_trace_closest reports it and the hit's barycentrics (TriHit b0, b1, b2), the operands of si.p.
 * Motion, per pixel, the cases in this order:
 *   1. ids.shape == YK_SURFACE_NONE or guides.hit == 0: the all-zero record.
 *   2. shape >= n_triangles + n_spheres: the all-zero record; the index is never followed.
 *   3. shape >= n_triangles (sphere k = shape - n_triangles): without a previous sphere table (yk_surface_motion)
 *      (guides.p as bits, 1): the sphere did not move.  With one (yk_surface_motion_spheres, after yk_scene_apply_edit
 *      moved spheres): q = xf_point(world_to_object of the scene's CURRENT record k, p), q = q * (radius_prev / radius)
 *      unless the two radii have equal bits, p_prev = xf_point(object_to_world of the PREVIOUS record k, q), every
 *      component canonical; known = 1.  The point keeps its place in the sphere's object space, scaled with the radius.
 *   4. A triangle with vertex indices i0, i1, i2: p_prev = P'[i0]*b0 + P'[i1]*b1 + P'[i2]*b2 per component, products first,
 *      summed left to right (the expression of si.p), P' = prev_points; known = 1.
 * Reproject-moved: yk_history_reproject's rule with p_P := motion.p_prev; known == 0 gives the zero record as a miss does;
 *   ns_P and the hit flag come from the CURRENT guide.  So the point projected into the previous camera is the previous
 *   position, and the plane test d = dot(ns_P, p_Q - p'_P) runs in the previous frame's world, where the previous guides
 *   live — with the CURRENT normal: exact for a translation, approximate under a rotation (the error is the tap distance
 *   times the sine of the turn), and a surface that turns by more than acos(normal_cos_min) between two frames loses its
 *   history.  Carried radiance is the radiance the surface HAD: shadows and reflections of things that moved lag until
 *   yk_history_rectify (run after this pass, before the blend) clips them to the current frame, or max_history ends them.
 * Not handled: lights (a light carries no film; what its move changes in the picture is yk_history_rectify's business),
 * shapes whose count or indices changed, yk_multi scenes. */
#define YK_SURFACE_NONE 0xffffffffu
typedef struct yk_surface_id {
    uint32_t shape; /* source shape index as yk_trace_closest reports it (a sphere is n_triangles + k); YK_SURFACE_NONE on a miss */
    float b[3];     /* the hit's barycentrics b0, b1, b2 (TriHit); 0 for a sphere and on a miss */
} yk_surface_id;    /* 16 bytes; 16-byte aligned on the device */
typedef struct yk_motion {
    float p_prev[3]; /* where the pixel's surface point stood under prev_points (world space) */
    float known;     /* 1.0f, or 0.0f: no previous position (then p_prev is 0) */
} yk_motion;         /* 16 bytes; 16-byte aligned on the device */
/* yk_render_guides with the ids beside the guides: the same single trace; the guides are byte for byte yk_render_guides'.
 * Either output may be NULL, not both.  YK_ERR_INVALID_ARGUMENT: as yk_render_guides, both outputs NULL. */
yk_status yk_render_guides_ids(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y,
                               yk_guide* out_guides, yk_surface_id* out_ids);
/* The same into device memory (both 16-byte aligned, not overlapping; anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched), ordered on `stream` as yk_render_guides_device. */
yk_status yk_render_guides_ids_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y,
                                      void* d_guides, void* d_ids, void* stream);

/* ---- guides through glass: the records of the surface a pixel SHOWS (the rule: yuki_amd/csrc/yk_guides_through.h) ----
 * yk_render_guides_ids describes the first hit of the pixel's centre ray; where that is glass the records describe the pane
 * — one normal, one plane, an albedo of ones — and not what is seen through it.  This pass follows glass, the renderer's
 * only delta material, and writes the records at the first hit that is not glass.  Per pixel, k = 0 and ray_0 the guide
 * pass's ray: trace ray_k; a miss gives the all-zero guide, the id (YK_SURFACE_NONE, 0, 0, 0) and through = k; a hit on
 * anything but glass, or with k == max_through, gives guide = (ns, 1, p, T_k) of THIS hit, its id and through = k, where
 * T_0 = t_0 and T_k = T_{k-1} + t_k in binary32; a glass hit with k < max_through continues with the transmission lobe's
 * direction (Bsdf::sample_f restricted to SPECULAR | TRANSMISSION, as Whitted asks for it) unless Kt is exactly black or
 * the lobe is totally internally reflected, else with the reflection lobe's unless Kr is exactly black, else the glass
 * hit is final; ray_{k+1} = spawn_ray(p, n, wi), wi not renormalised.  The record layouts are yk_render_guides_ids', so
 * every pass that takes guides or ids takes these.  max_through = 0: yk_render_guides_ids byte for byte.
 * Limits: one branch per interface (a pane's mirror image is not guided); the albedo behind tinted glass ignores Kt; p is
 * the real position of the surface seen, not a virtual image (reprojection and motion through refraction are approximate);
 * metal and glossy are not followed; yk_multi scenes are not served. */
#define YK_GUIDES_THROUGH_MAX 8
/* Host buffers of res_x * res_y records each, row-major; out_through: the interfaces crossed, 0 .. max_through.  Any output
 * may be NULL, not all three.  YK_ERR_INVALID_ARGUMENT: as yk_render_guides_ids, max_through > YK_GUIDES_THROUGH_MAX. */
yk_status yk_render_guides_through(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y,
                                   uint32_t max_through, yk_guide* out_guides, yk_surface_id* out_ids, uint32_t* out_through);
/* The same into device memory (guides and ids 16-byte aligned, through 4-byte aligned, no two overlapping; anything else:
 * YK_ERR_INVALID_ARGUMENT, nothing is launched), ordered on `stream` as yk_render_guides_device: 1 + max_through closest-hit
 * traces with one k_guides_step each, no host read-back between them, no allocation beyond the guide pass's. */
yk_status yk_render_guides_through_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, uint16_t res_x, uint16_t res_y,
                                          uint32_t max_through, void* d_guides, void* d_ids, void* d_through, void* stream);

/* Host buffers: res_x * res_y records each, row-major; prev_points holds 3 floats for each of the scene's n_vertices (the
 * call cannot see its length: the caller answers for it).  ctx NULL = the host instance on the CPU, else on ctx's device
 * (synchronous).  The host instance reads the scene's vertex indices on the host: a host-only scene keeps them; for a
 * scene in device memory (yk_scene_create, yk_scene_create_device) they are copied back from its device with every call.
 * YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero resolution, an output that overlaps an input, with a context a scene of
 * another device. */
yk_status yk_surface_motion(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides,
                            const float* prev_points, uint16_t res_x, uint16_t res_y, yk_motion* out);
/* The same on device buffers (ids, guides and output 16-byte aligned, prev_points 4-byte aligned, the output overlapping no
 * input; anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched), enqueued on `stream` (NULL = the context's) without
 * waiting for the device: one launch, no allocation.  An id whose shape is out of range is answered as in the rule. */
yk_status yk_surface_motion_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides,
                                   const float* d_prev_points, uint16_t res_x, uint16_t res_y, void* d_out, void* stream);
/* Motion with the sphere case: prev_spheres holds the scene's n_spheres records as they were BEFORE the last
 * yk_scene_apply_edit (the caller keeps the table it gave, as it keeps prev_points); the current records are the scene's
 * own.  prev_spheres NULL is yk_surface_motion byte for byte; prev_points may be NULL for a scene without triangles.
 * Everything else as yk_surface_motion / yk_surface_motion_device (d_prev_spheres 4-byte aligned); the records go to
 * yk_history_reproject_moved unchanged. */
yk_status yk_surface_motion_spheres(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides,
                                    const float* prev_points, const yk_sphere_desc* prev_spheres, uint16_t res_x, uint16_t res_y, yk_motion* out);
yk_status yk_surface_motion_spheres_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides,
                                           const float* d_prev_points, const void* d_prev_spheres, uint16_t res_x, uint16_t res_y, void* d_out, void* stream);
/* Motion from matrices, for a scene moved by yk_scene_transform: yk_surface_motion's rule with P'[i] := the per-vertex rule
 * of yk_scene_transform applied to the scene's REST point i under the PREVIOUS record of the triangle's mesh
 * (tri_mesh[shape]); then the same barycentric expression and the same case order.  The caller keeps 128 bytes a mesh from
 * the previous frame instead of 12 bytes a vertex.  prev_transforms holds the scene's n_meshes records as the previous
 * yk_scene_transform got them; NULL: the scene stood at rest.  (A scene that was never transformed is its own rest pose.)
 * prev_spheres NULL: the spheres did not move; otherwise yk_surface_motion_spheres' case.  The records are not tested: what
 * yk_scene_transform accepted is fine here.  Buffers, alignment (d_prev_transforms 4-byte aligned), ordering and errors as
 * yk_surface_motion[_spheres][_device]; the device call is one launch without an allocation, and its gather is the rule's:
 * the range test stands before the first dependent load, no load sits under a per-pixel branch (a lane that is no triangle
 * asks for triangle 0 and drops the answer), a scene without triangles loads nothing. */
yk_status yk_surface_motion_transforms(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, const yk_guide* guides,
                                       const yk_mesh_transform* prev_transforms, const yk_sphere_desc* prev_spheres, uint16_t res_x, uint16_t res_y, yk_motion* out);
yk_status yk_surface_motion_transforms_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, const void* d_guides,
                                              const void* d_prev_transforms, const void* d_prev_spheres, uint16_t res_x, uint16_t res_y, void* d_out, void* stream);
/* yk_history_reproject through the motion records; arguments and errors as yk_history_reproject, plus `motion`. */
yk_status yk_history_reproject_moved(yk_context* ctx, const yk_temporal_desc* desc, const yk_history* prev_history,
                                     const yk_guide* prev_guides, const yk_camera* prev_camera, const yk_guide* guides,
                                     const yk_motion* motion, uint16_t res_x, uint16_t res_y, yk_history* out_history);
/* The same on device buffers, as yk_history_reproject_device (d_motion 16-byte aligned too). */
yk_status yk_history_reproject_moved_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_prev_history,
                                            const void* d_prev_guides, const yk_camera* prev_camera, const void* d_guides,
                                            const void* d_motion, uint16_t res_x, uint16_t res_y, void* d_out_history, void* stream);

/* ---- albedo: textures under the denoiser — first-hit albedo from surface ids, and the a-trous filter on radiance / albedo ----
 * yk_denoise filters radiance, so on a textured surface it either blurs the texture (an open colour stop) or keeps the
 * noise (a closed one).  Two passes, the library's own; the rule is stated next to each expression in
 * yuki_amd/csrc/yk_albedo.h, and the host and the device instance agree bit for bit (binary32, every operation separate, no
 * FMA, divisions correctly rounded, a NaN an operation produces is 0x7fc00000, a value that is only copied keeps its bits).
 * Intended use: yk_render_guides_ids -> yk_surface_albedo -> yk_denoise_albedo where yk_denoise stood; the ids and the
 * albedo depend on the camera and the scene only, as the guides do.  After a temporal blend the blended RGB goes in with
 * samples = NULL as it goes into yk_denoise: the history stays in radiance.
 * Albedo, per pixel, the cases in this order:
 *   1. ids.shape == YK_SURFACE_NONE: (1, 1, 1, 0).
 *   2. shape >= n_triangles + n_spheres: (1, 1, 1, 0); the index is never followed.
 *   3. The material is tri_material[shape] for a triangle, spheres[shape - n_triangles].material for a sphere.  An index
 *      outside materials[]: (1, 1, 1, 0), never followed.  Not YK_MAT_MATTE (glass, metal, glossy): (1, 1, 1, 0).
 *   4. An untextured matte: (Kd as bits, 1).
 *   5. A textured matte on a triangle: uv = (uv0*b0 + uv1*b1) + uv2*b2 per component, products first, summed left to
 *      right; uv0..2 the mesh's uvs at the triangle's indices, or (0,0), (1,0), (1,1) where the mesh has none.  The record
 *      is (the texel ImageTexture::evaluate reads there, as bits, 1).
 *   6. A textured matte on a sphere: (1, 1, 1, 0).
 * Demodulated denoise: yk_denoise's rule with
 *   the divisor d per pixel and channel: a where a is finite and a >= YK_ALBEDO_FLOOR; 1 where a is NaN or infinite;
 *     YK_ALBEDO_FLOOR otherwise.  `known` is not read: the records of cases 1-3 and 6 are all ones;
 *   in: after the normalisation by the sample table every channel is divided by d, once per pixel; the iterations run on
 *     these colours, so sigma_color acts on demodulated radiance;
 *   out: the last iteration's sum(w * c_Q) / sum(w) is multiplied by the pixel's own d;
 *   iterations = 0: the normalised film, copied as bits: no division, no product.
 * Pixel mean (yk_albedo_mean, yk_render_albedo_mean): where texels or edges are smaller than a pixel, the record of one
 *   ray through the pixel centre is not the albedo of what the film averaged; these entry points write the mean of the
 *   first-hit albedo over an s x s grid of sub-pixel rays into the same yk_albedo record, which every consumer takes
 *   unchanged.
 *   Sub-samples: output pixel (x, y) of a res_x x res_y film covers the pixels (s*x + i, s*y + j), i, j = 0..s-1, of the
 *     (s*res_x) x (s*res_y) film of the same view: yk_camera_init with res = (s*res_x, s*res_y) and otherwise the same
 *     parameters.  The sub-rays are that camera's pixel-centre rays, exactly what yk_render_guides_ids traces.
 *   Per sub-sample: the record of its id by the six cases above; an unknown one enters the sum as (1, 1, 1).
 *   Mean, per channel: the first value (j = 0, i = 0), then every further one added in binary32 with j outer and i inner,
 *     left to right, every addition separate; one correctly rounded division by (float)(s*s); a NaN this produces is
 *     0x7fc00000.  known = 1 if any sub-sample is known, else 0; a block of unknown sub-samples is (1, 1, 1, 0) exactly.
 *     s = 1 copies the one record: yk_surface_albedo's, bit for bit.
 *   Range: 1 <= s <= YK_ALBEDO_MEAN_MAX_S; s*res_x and s*res_y <= 65535 (pixel coordinates travel in 16 bits each).
 * Not handled: glass, metal and glossy surfaces, textured spheres, yk_multi scenes.  The mean is over a regular grid, not
 *   over the film's own samples; an edge pixel between a matte and a non-matte surface mixes its albedo with ones. */
#define YK_ALBEDO_FLOOR 0.015625f /* 2^-6, exact */
typedef struct yk_albedo {
    float a[3];  /* the first hit's diffuse albedo; (1, 1, 1) where it is not known */
    float known; /* 1.0f, or 0.0f: nothing to demodulate by */
} yk_albedo;     /* 16 bytes; 16-byte aligned on the device */
/* Host buffers: res_x * res_y records each, row-major.  ctx NULL = the host instance on the CPU, else on ctx's device
 * (synchronous).  The host instance reads the scene's indices, uvs, materials and texels on the host: a host-only scene keeps
 * them; for a scene in device memory they are copied back from its device with every call.
 * YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero resolution, an output that overlaps the ids, with a context a scene of
 * another device. */
yk_status yk_surface_albedo(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids, uint16_t res_x, uint16_t res_y,
                            yk_albedo* out);
/* The same on device buffers (both 16-byte aligned, not overlapping; anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched), enqueued on `stream` (NULL = the context's) without waiting for the device: one launch, no allocation. */
yk_status yk_surface_albedo_device(yk_context* ctx, const yk_scene* scene, const void* d_ids, uint16_t res_x, uint16_t res_y,
                                   void* d_out, void* stream);
/* The pixel-mean albedo from the ids of the large film: the reduction alone.  ids_ss holds (s*res_x) * (s*res_y) records,
 * row-major; out res_x * res_y.  ctx NULL = the host instance (it reads the scene's tables as yk_surface_albedo does), else
 * on ctx's device (synchronous).
 * YK_ERR_INVALID_ARGUMENT: a NULL pointer, a zero resolution, s outside 1..YK_ALBEDO_MEAN_MAX_S, s*res_x or s*res_y over
 * 65535, an output that overlaps the ids, with a context a scene of another device. */
#define YK_ALBEDO_MEAN_MAX_S 8u
yk_status yk_albedo_mean(yk_context* ctx, const yk_scene* scene, const yk_surface_id* ids_ss, uint16_t res_x, uint16_t res_y,
                         uint32_t s, yk_albedo* out);
/* The same on device buffers (both 16-byte aligned, not overlapping; anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched), enqueued on `stream` (NULL = the context's) without waiting for the device: one launch, no allocation. */
yk_status yk_albedo_mean_device(yk_context* ctx, const yk_scene* scene, const void* d_ids_ss, uint16_t res_x, uint16_t res_y,
                                uint32_t s, void* d_out, void* stream);
/* The fused route: traces the large film and reduces it, bit for bit yk_albedo_mean of yk_render_guides_ids at
 * (s*res_x, s*res_y) under camera_ss — the yk_camera of THAT resolution.  The large film is never materialised: it is
 * traced in bands of output rows whose ids go through a scratch the context owns (64 MiB, allocated by the first call; the
 * context option "albedo_mean_band_rows" sets the output rows per band, 0 = as many as fit the scratch; only a band that
 * needs more than the scratch holds allocates again).  Needs a context, as yk_render_guides does.  The _device form is
 * ordered on `stream` (NULL = the context's) as yk_render_guides_device is; d_out is 16-byte aligned.
 * YK_ERR_INVALID_ARGUMENT, nothing launched: as yk_albedo_mean, a NULL camera, a misaligned output. */
yk_status yk_render_albedo_mean(yk_context* ctx, const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x, uint16_t res_y,
                                uint32_t s, yk_albedo* out);
yk_status yk_render_albedo_mean_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera_ss, uint16_t res_x,
                                       uint16_t res_y, uint32_t s, void* d_out, void* stream);
/* yk_denoise with the albedo records; arguments and errors as yk_denoise, plus: a NULL albedo, an albedo that overlaps the
 * output. */
yk_status yk_denoise_albedo(yk_context* ctx, const yk_denoise_desc* desc, const float* film_rgb, const yk_guide* guides,
                            const yk_albedo* albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                            float* out_rgb);
/* The same on device buffers, as yk_denoise_device (d_albedo 16-byte aligned too): a preparing launch, then one launch per
 * iteration; both ping-pong buffers of the context are used from two iterations on. */
yk_status yk_denoise_albedo_device(yk_context* ctx, const yk_denoise_desc* desc, const void* d_film_rgb, const void* d_guides,
                                   const void* d_albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                   void* d_out_rgb, void* stream);

/* ---- guided upsampling: a film rendered at 1/s resolution rebuilt at full resolution ----
 * A caller who wants a frame sooner renders a smaller film; a bilinear stretch of it blurs every texture and smears every
 * silhouette.  yk_upsample takes the low film to full resolution through the first-hit guides of BOTH resolutions: a
 * joint-bilateral upsample of demodulated radiance, remodulated with the full-resolution albedo.  It sits between the low
 * film (or its denoiser) and the tone map.  The library's own pass; the rule is stated next to each expression in
 * yuki_amd/csrc/yk_upsample.h, and the host and the device instance agree bit for bit (binary32, every operation separate,
 * no FMA, divisions correctly rounded, exp = the library's expf, a NaN an operation produces is 0x7fc00000, a value that
 * is only copied keeps its bits).
 * Geometry: the low film is low_res_x x low_res_y, the full film exactly (s*low_res_x) x (s*low_res_y), both <= 65535:
 *   yk_albedo_mean's relation, full pixel (s*X + i, s*Y + j) lies in low pixel (X, Y).  Per axis t = (float)(2i + 1 - s) /
 *   (float)(2s); t < 0: x0 = X - 1 and ax = t + 1.0f, otherwise x0 = X and ax = t.
 * Low pixel Q, once per pixel: c_Q = the low film's RGB, normalised by the low film's sample table where one is given
 *   (yk_denoise's input rule on the LOW grid), with albedo each channel divided by the divisor of Q's low albedo record
 *   (yk_denoise_albedo's divisor).
 * Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), b = (1 - ax | ax) * (1 - ay | ay), accumulated in that order.  A tap
 *   is skipped when it lies outside the low film, b == 0, the hit class of the FULL guide of P differs from the LOW guide
 *   of Q, a channel of c_Q is NaN or infinite, or its weight is 0 or NaN.  Two hits: w = b * exp(-(a_n + a_p)) with
 *   yk_denoise's normal and plane terms of (P = full guide, Q = low guide); two misses: w = b.
 * Output: sw = sum w; sw != 0: rgb = sum(w * c_Q) / sw per channel; sw == 0: c of the containing low pixel (X, Y), as bits.
 *   With albedo each channel is then multiplied by the divisor of P's FULL albedo record.  out_weight, optional: sw per
 *   full pixel, 0 exactly where the fallback ran (those pixels can be handed to the pixel-list route; that hand-off is
 *   not built).
 * The low albedo is the mean albedo of the low pixel over the full pixels it covers: yk_albedo_mean at factor s of the
 *   FULL film's ids.
 * Limits: a low pixel's film value averages its footprint while its guide is one centre ray, so full pixels beside a
 *   silhouette inherit a mixed value; a feature no low centre ray hits falls back to the containing pixel; glass, metal
 *   and glossy surfaces are not demodulated; yk_multi scenes are not served; temporal history at full resolution over
 *   upsampled frames is not addressed (carry the history at low resolution and upsample last).  Where texels are smaller
 *   than a pixel the albedo records of both resolutions must be pixel means (yk_albedo_mean) for the pass to gain anything.
 * Measured: on textured-city, 4 spp at 48 x 27 -> 96 x 54 against 1024 spp, 0.90 x the error of a bilinear
 *   stretch with pixel-mean albedo records, 1.00 x with the centre ray's; on one MI355X at 1920 x 1080 the kernel takes
 *   39.8 us at s = 2, and a 4-spp frame with guides, albedo, denoise and tone map 16.8 ms through s = 2 against 26.3 ms. */
#define YK_UPSAMPLE_MAX_S 8u /* = YK_ALBEDO_MEAN_MAX_S */
typedef struct yk_upsample_desc {
    uint32_t s;         /* 1 .. YK_UPSAMPLE_MAX_S */
    float sigma_normal; /* > 0; +inf: no normal stop */
    float sigma_plane;  /* > 0, scene units; +inf: no plane stop */
} yk_upsample_desc;
/* Host buffers.  low_rgb: low_res_x * low_res_y * 3 floats; low_guides and low_albedo: one record per low pixel; guides and
 * albedo: one record per FULL pixel; out_rgb: 3 floats per full pixel; out_weight: one float per full pixel, or NULL.
 * low_albedo and albedo are given both (the demodulated route) or neither.  tile_dim and samples (may be NULL) belong to
 * the LOW film, as yk_denoise's.  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).
 * YK_ERR_INVALID_ARGUMENT: a NULL required pointer, a zero resolution or tile_dim, s outside 1..YK_UPSAMPLE_MAX_S,
 * s*low_res_x or s*low_res_y over 65535, a sigma that is <= 0 or NaN, one albedo without the other, an output that overlaps
 * any input or the other output. */
yk_status yk_upsample(yk_context* ctx, const yk_upsample_desc* desc, const float* low_rgb, const yk_guide* low_guides,
                      const yk_albedo* low_albedo, uint16_t low_res_x, uint16_t low_res_y, uint16_t tile_dim, const uint32_t* samples,
                      const yk_guide* guides, const yk_albedo* albedo, float* out_rgb, float* out_weight);
/* The same on device buffers (guides and albedo records 16-byte aligned, RGB and weight 4-byte aligned; anything else, or a
 * refusal above: YK_ERR_INVALID_ARGUMENT, nothing is launched), enqueued on `stream` (NULL = the context's) without
 * waiting for the device: one launch, no allocation beyond the context's copy of the sample table.  `samples` is a HOST
 * table, copied before the call returns. */
yk_status yk_upsample_device(yk_context* ctx, const yk_upsample_desc* desc, const void* d_low_rgb, const void* d_low_guides,
                             const void* d_low_albedo, uint16_t low_res_x, uint16_t low_res_y, uint16_t tile_dim,
                             const uint32_t* samples, const void* d_guides, const void* d_albedo, void* d_out_rgb,
                             void* d_out_weight, void* stream);

/* ---- variance: carried luminance moments steer the a-trous filter ----
 * yk_denoise's colour stop sigma_color / 2^i is one global constant: a film that yk_history_blend has carried for 32
 * samples gets the blur of a film of 4.  Three passes, the library's own (after Schied et al., "Spatiotemporal
 * Variance-Guided Filtering", HPG 2017); the rule is stated next to each expression in yuki_amd/csrc/yk_variance.h, and the
 * host and the device instance agree bit for bit (binary32, every operation separate, no FMA, divisions correctly rounded,
 * exp = the library's expf, a NaN an operation produces is 0x7fc00000, a value that is only copied keeps its bits).
 * Intended use, per frame: every pass is rendered into a cleared film; yk_history_blend folds it into the colour history and
 * yk_moments_blend folds the SAME film into the moments; when the camera or the geometry moves the moments buffer goes
 * through yk_history_reproject[_moved] cast to yk_history (same layout, same taps, same weights, same skip set as the colour
 * history); then yk_variance(moments, blended RGB, samples = NULL) -> yk_denoise_variance(blended RGB, variance) where
 * yk_denoise stood.
 * Luminance l(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b.
 * Moments blend, per pixel: c and m as yk_history_blend reads them; l = l(c), ll = l*l; n = min(h.n, max_history).  The
 *   moments are absent when the pointer is NULL, n is <= 0 or NaN, or a field is not finite; the current view when m == 0
 *   or ll is not finite (a non-finite pixel never enters the moments).  Both absent: zeros.  Only the moments absent:
 *   (l, ll, 1, m).  Only the current view absent: (h.m1, h.m2, h.frames * (n / h.n), n).  Neither: t = n + m — the count
 *   yk_history_blend writes, bit for bit — m1 = (n*h.m1 + m*l) / t, m2 = (n*h.m2 + m*ll) / t,
 *   frames = h.frames * (n / h.n) + 1.
 * Variance, per pixel: where the moments are present and frames >= 2 the temporal estimate max(0, m2 - m1*m1) / (frames - 1)
 *   (with an albedo divided by the square of the luminance of the pixel's own divisors: an approximation, exact for a grey
 *   albedo); everywhere else spatial_scale times the weighted variance of l over the 7 x 7 window of the normalised (with an
 *   albedo: demodulated) film, the weights being yk_denoise's normal and plane stops without a kernel and without a colour
 *   stop; taps outside the film, of the other hit class, of weight 0 or NaN, or whose l*l is not finite are skipped, the
 *   centre is always taken.  NaN or negative is written as 0; +inf stays and switches the colour stop off for that pixel.
 * Filter: yk_denoise's rule (taps, kernel, normal and plane stops, skip rule, always-taken centre, iterations = 0, in-place
 *   output, albedo as yk_denoise_albedo) with a_c = (dl*dl) / (sigma_variance^2 * g + epsilon), dl the luminance difference
 *   of the two colours, g the 3 x 3 Gaussian (1/4, 1/8, 1/16) of the variance around P at unit spacing over the taps inside
 *   the film whose variance is finite, renormalised (g = +inf where P's own variance is; sigma_variance = +inf: the stop is
 *   off); no / 2^i.  The variance travels with the colours: var' = sum(w*w * var_Q) / (sum w)^2 over the taken taps whose
 *   variance is finite; an infinite variance stays where it is and does not spread.
 * Limits: variance of luminance only; yk_multi scenes are not served; the temporal estimate inherits what lag
 *   yk_history_rectify leaves the history on glass and metal (it shrinks the moments' count with the history's). */
typedef struct yk_moments {
    float m1;     /* the mean luminance */
    float m2;     /* the mean squared luminance of the frame means */
    float frames; /* the effective number of frames behind them */
    float n;      /* the effective number of samples, yk_history's n */
} yk_moments;     /* 16 bytes, the layout of yk_history; 16-byte aligned on the device */
typedef struct yk_variance_desc {
    uint32_t iterations;                             /* 0 .. 8 */
    float sigma_variance, sigma_normal, sigma_plane; /* each > 0; +inf switches its stop off */
    float epsilon;                                   /* >= 0: added to the colour stop's denominator */
    float spatial_scale;                             /* >= 0: the factor on the spatial estimate */
} yk_variance_desc;
/* film_rgb, `samples` and tile_dim as yk_history_blend takes them; `desc` may be the one given to yk_history_blend (only
 * max_history is used, all of it is checked); moments may be NULL; out_moments may equal moments.
 * YK_ERR_INVALID_ARGUMENT: a NULL desc, film or output, a zero resolution, tile_dim 0, a parameter out of range or NaN, an
 * output that overlaps the film, or the moments without being equal to them. */
yk_status yk_moments_blend(yk_context* ctx, const yk_temporal_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y,
                           uint16_t tile_dim, const uint32_t* samples, const yk_moments* moments, yk_moments* out_moments);
/* The same on device buffers, enqueued on `stream` (NULL = the context's) without waiting for the device: one launch.
 * d_film_rgb needs 4-byte alignment, the moments 16-byte alignment (anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched). */
yk_status yk_moments_blend_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                                  uint16_t tile_dim, const uint32_t* samples, const void* d_moments, void* d_out_moments, void* stream);
/* moments and albedo may be NULL; out_variance holds res_x * res_y floats.  ctx NULL = the host instance.
 * YK_ERR_INVALID_ARGUMENT: a NULL desc, film, guides or output, a zero resolution, tile_dim 0, iterations > 8, a sigma that
 * is <= 0 or NaN, an epsilon or spatial_scale that is < 0 or NaN, an output that overlaps an input. */
yk_status yk_variance(yk_context* ctx, const yk_variance_desc* desc, const yk_moments* moments, const float* film_rgb,
                      const yk_guide* guides, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                      const uint32_t* samples, float* out_variance);
/* The same on device buffers, one launch on `stream`: film and variance 4-byte aligned, moments, guides and albedo 16-byte
 * aligned (anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched). */
yk_status yk_variance_device(yk_context* ctx, const yk_variance_desc* desc, const void* d_moments, const void* d_film_rgb,
                             const void* d_guides, const void* d_albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                             const uint32_t* samples, void* d_out_variance, void* stream);
/* yk_denoise with the variance image; albedo may be NULL; out_rgb may equal film_rgb.  Errors as yk_denoise's, plus: a NULL
 * variance, a variance or an albedo that overlaps the output, an epsilon that is < 0 or NaN. */
yk_status yk_denoise_variance(yk_context* ctx, const yk_variance_desc* desc, const float* film_rgb, const yk_guide* guides,
                              const float* variance, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                              const uint32_t* samples, float* out_rgb);
/* The same on device buffers, as yk_denoise_albedo_device: a preparing launch, then one launch per iteration through the
 * context's ping-pong buffers; film, variance and output 4-byte aligned, guides and albedo 16-byte aligned. */
yk_status yk_denoise_variance_device(yk_context* ctx, const yk_variance_desc* desc, const void* d_film_rgb, const void* d_guides,
                                     const void* d_variance, const void* d_albedo, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                                     const uint32_t* samples, void* d_out_rgb, void* stream);

/* ---- history rectification: carried radiance clipped to the current frame ----
 * A carried history is right for the previous view, the previous lighting and the previous positions.  This pass compares
 * it with the frame at hand, before yk_history_blend folds that frame in: after yk_history_reproject[_moved] when something
 * moved, on the last blend's history while the view stands (lights and materials change under a still camera too).  The
 * rule is stated next to each expression in yuki_amd/csrc/yk_rectify.h; the host and the device instance agree bit for bit
 * (binary32, every operation separate, no FMA, division and sqrtf correctly rounded, a NaN an operation produces is
 * 0x7fc00000, a value that is only copied keeps its bits).
 * Per pixel P, with m_Q and c_Q the count and the colour of film pixel Q as yk_history_blend reads them (m = 1 and the
 * film's bits without a table; with one, m = (float)samples[flat] and c divided by m where m > 0):
 *   1. Taps: the (2 radius + 1)^2 pixels around P, row-major; taken when inside the film, m_Q != 0 and c_Q finite in all
 *      three channels; k of them are.  A tap outside the film is never read.
 *   2. The output is history[P]'s 16 bytes when the history is absent by the blend's test (n <= 0 or NaN, a channel not
 *      finite), k < 2, a mu_c or e_c below is not finite, or no channel is clipped.
 *   3. Per channel over the taken taps in tap order: mu = sum(c) / k; sigma = sqrtf(sum((c - mu)(c - mu)) / k);
 *      e = gamma * sigma; lo = mu - e, hi = mu + e.
 *   4. out_c = h_c < lo ? lo : (h_c > hi ? hi : h_c); f_c = e / |h_c - mu| for a clipped channel (in [0, 1]) and 1 for
 *      any other; f = the least of the three.
 *   5. n' = n * f: how much of the history the clip kept.  n' == 0 makes the history absent, and the blend starts over.
 *   6. With moments: where the history was clipped and the moments record is present (n > 0, the other fields finite),
 *      its n becomes n' (the history's bits) and its frames are multiplied by f; m1 and m2 keep their bits.  Every other
 *      record is copied.
 * Limits: a per-channel RGB box, no chroma space; m1 and m2 stay stale after a clip; a history that is wrong but lies inside
 * the current frame's noise box stays; yk_multi scenes are not served. */
typedef struct yk_rectify_desc {
    uint32_t radius; /* 1 .. 3: the window is (2 radius + 1)^2 pixels */
    float gamma;     /* >= 0: the half-width of the box in standard deviations; +inf: every pixel passes through */
} yk_rectify_desc;
/* film_rgb, `samples` and tile_dim as yk_history_blend takes them; moments may be NULL, and out_moments is NULL exactly
 * then.  out_history may equal history and out_moments may equal moments: a pixel reads only its own records, the window
 * reads the film.  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).
 * YK_ERR_INVALID_ARGUMENT: a NULL desc, film, history or out_history, a zero resolution, tile_dim 0, a radius outside
 * 1 .. 3, a gamma that is < 0 or NaN, out_moments without moments or moments without out_moments, an output that overlaps
 * an input without being equal to its own counterpart, outputs that overlap each other. */
yk_status yk_history_rectify(yk_context* ctx, const yk_rectify_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y,
                             uint16_t tile_dim, const uint32_t* samples, const yk_history* history, const yk_moments* moments,
                             yk_history* out_history, yk_moments* out_moments);
/* The same on device buffers, enqueued on `stream` (NULL = the context's) without waiting for the device: one launch, and
 * no allocation beyond the temporal pass's staged sample table (`samples` is a HOST table, copied before the call returns).
 * d_film_rgb needs 4-byte alignment, the records 16-byte alignment (anything else: YK_ERR_INVALID_ARGUMENT, nothing is
 * launched). */
yk_status yk_history_rectify_device(yk_context* ctx, const yk_rectify_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                                    uint16_t tile_dim, const uint32_t* samples, const void* d_history, const void* d_moments,
                                    void* d_out_history, void* d_out_moments, void* stream);

/* ---- despeckle: film outliers clamped to their neighbourhood ----
 * A pixel of the CURRENT frame's film that is far brighter than everything around it (a firefly) enters yk_history_blend at
 * full weight, widens yk_history_rectify's box, inflates the luminance moments and survives the à-trous filter.  This pass
 * runs first in a frame, on the film, before all of them: a pixel whose luminance exceeds `gain` times the rank-th largest
 * luminance among the OTHER pixels of its (2 radius + 1)^2 window is scaled down to that bound, its chromaticity kept.  It
 * reads the film and nothing else (no guides).  The rule is stated next to each expression in yuki_amd/csrc/yk_despeckle.h;
 * the host and the device instance agree bit for bit (binary32, every operation separate, no FMA, division correctly
 * rounded, a NaN an operation produces is 0x7fc00000, a value that is only copied keeps its bits).
 * Luminance l(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b (yk_variance's).  Finite: neither NaN nor +-inf.
 * Per pixel P, with m_Q and c_Q the count and the colour of film pixel Q as yk_history_blend reads them (m = 1 and the
 * film's bits without a table; with one, m = (float)samples[flat] and c = film / m per channel where m > 0), and s_P the
 * three floats the film STORES at P (s_P = c_P without a table):
 *   1. m_P == 0: the output is s_P.
 *   2. Taps: the (2 radius + 1)^2 - 1 pixels around P without P, row-major; taken when inside the film, m_Q != 0 and c_Q
 *      finite in all three channels; k of them are, l_Q = l(c_Q).  A tap outside the film is never read.
 *      k < max(min_taps, rank): the output is s_P.
 *   3. v = the rank-th largest l_Q (as a multiset); a v that is not > 0 counts as +0.  bound = gain * v; where
 *      bound < floor, bound = floor.  A NaN bound (+inf * 0) : the output is s_P.
 *   4. c_P finite in all three channels: where l_P = l(c_P) > bound, the output is s_P * (bound / l_P) per channel — one
 *      division, one multiplication a channel — and the mask is 1; the factor is in [0, 1).  Otherwise the output is s_P.
 *   5. c_P not finite: with YK_DESPECKLE_REPAIR, per channel the sum of the taken taps' c_Q in tap order (sequential, from
 *      0), divided by (float)k, and with a table multiplied by m_P; the mask is 2.  Without the flag the output is s_P.
 * The output film uses the input's convention: a film of sums stays a film of sums, with the same sample table.
 * A negative v counting as 0 changes no bound at a finite gain > 0 (gain * v < 0 <= floor either way); it makes
 * gain = +inf, floor = 0 the identity on every film: +inf * v is +inf, which nothing exceeds, or the NaN of step 3.
 * Limits: biased by design — it removes energy from heavy-tailed light transport (caustics, small bright emitters seen
 * through glossy paths) and does not vanish as the film converges: it belongs in front of an accumulating or denoising
 * chain, not on a film meant to converge.  Luminance only.  A real glint narrower than the window's rank is clamped like a
 * firefly.  yk_multi scenes are not served. */
#define YK_DESPECKLE_REPAIR 1u /* yk_despeckle_desc::flags: a pixel that is not finite becomes the mean of its taken taps */
typedef struct yk_despeckle_desc {
    uint32_t radius;   /* 1 .. 2: the (2 radius + 1)^2 - 1 pixels around P */
    uint32_t rank;     /* 1 .. 4: the rank-th largest neighbour luminance bounds P (1 = the maximum) */
    uint32_t min_taps; /* >= rank: fewer taken taps and P passes through */
    uint32_t flags;    /* YK_DESPECKLE_REPAIR */
    float gain;        /* >= 0, +inf allowed (nothing is clamped), NaN refused; -0 is taken as +0 */
    float floor;       /* >= 0, finite: a luminance below which nothing is clamped; -0 is taken as +0 */
} yk_despeckle_desc;
/* film_rgb, `samples` and tile_dim as yk_history_blend takes them.  out_rgb: res_x * res_y * 3 floats.  out_mask (may be
 * NULL): one byte a pixel, 0 untouched, 1 clamped, 2 repaired.  out_counts (may be NULL): two words, the pixels clamped and
 * the pixels repaired.  ctx NULL = the host instance on the CPU, else on ctx's device (synchronous).
 * YK_ERR_INVALID_ARGUMENT: a NULL desc, film or out_rgb, a zero resolution, tile_dim 0, a radius outside 1 .. 2, a rank
 * outside 1 .. 4, min_taps < rank, an unknown flag, a gain that is < 0 or NaN, a floor that is < 0, NaN or infinite, an
 * out_rgb that overlaps film_rgb (a pixel reads its neighbours' input: the pass does not run in place), a mask or counts
 * that overlap a film or each other. */
yk_status yk_despeckle(yk_context* ctx, const yk_despeckle_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y,
                       uint16_t tile_dim, const uint32_t* samples, float* out_rgb, uint8_t* out_mask, uint32_t* out_counts);
/* The same on device buffers, enqueued on `stream` (NULL = the context's) without waiting for the device: one launch (and
 * a memset of the two count words), and no allocation beyond the temporal pass's staged sample table (`samples` is a HOST
 * table, copied before the call returns).  The films and the counts need 4-byte alignment (anything else:
 * YK_ERR_INVALID_ARGUMENT, nothing is launched). */
yk_status yk_despeckle_device(yk_context* ctx, const yk_despeckle_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y,
                              uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* d_out_mask, void* d_out_counts,
                              void* stream);

/* ---- adaptive sampling: per-pixel statistics choose where the next samples go ----
 * The accumulating entry points give every pixel of a tile the same number of samples.  Here a film carries, beside its
 * RGB sums, one yk_pixel_stats record a pixel; a selection pass lists the pixels that are still noisy, a render takes that
 * list as it is, and a fold adds the results to the film and the statistics.  The library's own rule (the reference has
 * no adaptive sampler), stated next to each expression in yuki_amd/csrc/yk_adaptive.h; the host and the device instance
 * agree bit for bit, the order of the list included (binary32, every operation separate, no FMA, divisions correctly
 * rounded, a NaN an operation produces is 0x7fc00000).
 * Luminance l(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b (yk_variance's).
 * Fold of one sample c: drawn += 1 always; ll = l(c)*l(c) NaN or infinite: nothing else changes (a non-finite sample never
 *   enters the film or the statistics); otherwise film_sum += c (three adds), n += 1, d = l - mean,
 *   mean' = mean + d / (float)n, m2' = m2 + d * (l - mean')  (Welford, in sample order).
 * Wants: n < min_samples, or m2 > (threshold^2 * ((nf - 1) * nf)) * ((mean + epsilon) * (mean + epsilon)), nf = (float)n,
 *   threshold^2 computed once: (standard error of the mean) > threshold * (mean + epsilon), squared.  NaN compares false.
 * Selected: eligible (drawn + round_passes <= max_samples) and (wants, or dilate and one of the 8 neighbours inside the
 *   film wants — eligible itself or not).
 * Order of the list: tiles of 16 x 16 (a constant of the rule, not a film's tile_dim) over the ceil grid in row-major
 *   tile order, row-major inside a tile, clipped at the film's edges.  Entry = (x | y << 16, drawn).
 * Resolve: rgb = film_sum / (float)n where n > 0, zeros otherwise; variance of the mean = m2 / ((nf - 1) * nf) where
 *   n >= 2, +inf otherwise, NaN or negative written as 0: the image yk_denoise_variance takes as `variance`.
 * All zeros is the cleared state of film_sum and of the statistics.
 * Limits: luminance only; yk_multi scenes are not served; selecting on the samples' own variance biases the estimate
 *   slightly (the dilation and the floor on min_samples bound that, they do not remove it). */
typedef struct yk_pixel_stats {
    float mean;     /* running mean of the luminance of the samples taken */
    float m2;       /* sum of squared deviations from it */
    uint32_t n;     /* samples taken */
    uint32_t drawn; /* sample indices consumed: the pixel's next sample index */
} yk_pixel_stats;   /* 16 bytes; 16-byte aligned on the device */
typedef struct yk_adaptive_desc {
    uint32_t min_samples;  /* >= 2 */
    uint32_t max_samples;  /* min_samples .. 2^24 */
    uint32_t round_passes; /* 1 .. 0xFFFF: samples a selected pixel takes per round */
    uint32_t max_rounds;   /* yk_render_adaptive_device: 0 = until nothing is selected */
    uint32_t dilate;       /* 0 | 1 */
    float threshold;       /* > 0 */
    float epsilon;         /* >= 0 */
} yk_adaptive_desc;
typedef struct yk_adaptive_info {
    uint32_t rounds;       /* rounds rendered by this call */
    uint32_t converged;    /* 1: the last selection was empty; 0: max_rounds stopped the call */
    uint32_t first_pixels; /* entries of the first round's list */
    uint32_t last_pixels;  /* entries of the last rendered round's list */
    uint64_t samples, rays, shadow_rays;
} yk_adaptive_info;
/* A list of (pixel, first sample index) entries in device memory with room for res_x * res_y of them: filled by
 * yk_adaptive_select_device or yk_pixel_list_set, rendered by yk_render_pixel_list_device.  It belongs to `ctx` and must be
 * destroyed before it. */
typedef struct yk_pixel_list yk_pixel_list;
yk_status yk_pixel_list_create(yk_context* ctx, uint16_t res_x, uint16_t res_y, yk_pixel_list** out);
void yk_pixel_list_destroy(yk_pixel_list* list);
/* Host entries (xy = x | y << 16), checked on the host before the upload: every pixel inside the list's resolution, no pixel
 * twice, passes 1 .. 0xFFFF, sample + passes <= 2^24 (else YK_ERR_INVALID_ARGUMENT and the list is left as it was).
 * n may be 0.  Synchronous. */
yk_status yk_pixel_list_set(yk_pixel_list* list, const uint32_t* xy, const uint32_t* sample, uint32_t n, uint32_t passes);
/* The entries back on the host (either array may be NULL), at most `cap`; *out_n = the list's entry count. */
yk_status yk_pixel_list_read(const yk_pixel_list* list, uint32_t* out_xy, uint32_t* out_sample, uint32_t cap, uint32_t* out_n);
/* The selection.  out_xy / out_sample hold res_x * res_y words each (either may be NULL); *out_n = the number selected.
 * ctx NULL = the host instance.  YK_ERR_INVALID_ARGUMENT: a NULL desc, stats or out_n, a zero resolution, min_samples < 2,
 * max_samples < min_samples or > 2^24, round_passes 0 or > 0xFFFF, dilate > 1, threshold <= 0 or NaN, epsilon < 0 or NaN. */
yk_status yk_adaptive_select(yk_context* ctx, const yk_adaptive_desc* desc, const yk_pixel_stats* stats, uint16_t res_x, uint16_t res_y,
                             uint32_t* out_xy, uint32_t* out_sample, uint32_t* out_n);
/* The same on device statistics (16-byte aligned) into a list of the same resolution (anything else:
 * YK_ERR_INVALID_ARGUMENT, nothing is launched): three launches on `stream` (NULL = the context's), then the count is read
 * back — 4 bytes, one stream synchronisation — into *out_n and the list, with passes = round_passes and
 * sample_end = max_samples. */
yk_status yk_adaptive_select_device(yk_context* ctx, const yk_adaptive_desc* desc, const void* d_stats, uint16_t res_x, uint16_t res_y,
                                    yk_pixel_list* list, uint32_t* out_n, void* stream);
/* The fold: passes_rgb holds n_passes x n x RGB, pass-major (yk_render_pixel_list_device's output); entry e's values are
 * folded in pass order into film_sum and stats at its pixel.  The entries are checked on the host: every pixel inside the
 * film, none twice.  ctx NULL = the host instance.  n may be 0. */
yk_status yk_adaptive_accumulate(yk_context* ctx, const uint32_t* xy, uint32_t n, const float* passes_rgb, uint32_t n_passes, uint16_t res_x,
                                 uint16_t res_y, float* film_sum, yk_pixel_stats* stats);
/* The same for a list on device buffers, one launch on `stream` without waiting: passes and film 4-byte aligned, statistics
 * 16-byte aligned, no two buffers overlapping, the list of the call's resolution, n_passes 1 .. the list's passes
 * (anything else: YK_ERR_INVALID_ARGUMENT, nothing is launched). */
yk_status yk_adaptive_accumulate_device(yk_context* ctx, const yk_pixel_list* list, const void* d_passes_rgb, uint32_t n_passes, uint16_t res_x,
                                        uint16_t res_y, void* d_film_sum, void* d_stats, void* stream);
/* out_rgb (res_x * res_y * 3) and out_variance (res_x * res_y) may each be NULL, not both.  ctx NULL = the host instance. */
yk_status yk_adaptive_resolve(yk_context* ctx, const float* film_sum, const yk_pixel_stats* stats, uint16_t res_x, uint16_t res_y, float* out_rgb,
                              float* out_variance);
/* The same on device buffers, one launch on `stream`: alignment and overlap rules as yk_adaptive_accumulate_device. */
yk_status yk_adaptive_resolve_device(yk_context* ctx, const void* d_film_sum, const void* d_stats, uint16_t res_x, uint16_t res_y,
                                     void* d_out_rgb, void* d_out_variance, void* stream);
/* Integrator::render(accumulating = true) for a pixel list: passes sample .. sample + n_passes - 1 of every entry, raw
 * values, pass-major: d_out_rgb holds n_passes x n x RGB, each value bit for bit what the accumulating tile render writes
 * for that pixel at that sample index.  n_passes 1 .. the list's passes; a list whose sample_end exceeds the sampler's
 * samples per pixel is refused before anything is launched; an empty list returns YK_OK with nothing launched.  Chunks,
 * batches, work sets, stats and cancel as yk_render_tile_list_passes_device. */
yk_status yk_render_pixel_list_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                      const yk_integrator_desc* integrator, const yk_pixel_list* list, uint32_t n_passes, void* d_out_rgb,
                                      void* stream, yk_render_stats* stats, yk_cancel_fn cancel, void* user);
/* The driver: select -> stop when nothing is selected or max_rounds is reached -> render the list with round_passes,
 * folding every chunk's samples straight into d_film_sum and d_stats (no pass-major buffer exists) -> again.  It continues
 * from whatever the statistics hold: cleared buffers select every pixel (n < min_samples); a later call with a larger
 * max_samples refines.  max_samples may not exceed the sampler's samples per pixel.  Synchronous (one count read-back per
 * round).  On YK_ERR_CANCELLED film and statistics are undefined.  `info` may be NULL. */
yk_status yk_render_adaptive_device(yk_context* ctx, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                    const yk_integrator_desc* integrator, const yk_adaptive_desc* desc, uint16_t res_x, uint16_t res_y,
                                    void* d_film_sum, void* d_stats, void* stream, yk_adaptive_info* info, yk_cancel_fn cancel, void* user);

/* ---- per-stage entry points (parity tests, profiling) ------------------------- */
/* BoundingVolumeHierarchy::intersect (bvh.rs:160-232) for n host rays.
 * out_shape: source shape index or -1; counters as IntersectionResult. */
yk_status yk_trace_closest(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d,
                           const float* t_max /* NULL = inf */, int32_t* out_shape, float* out_t, float* out_bary /* 3n */,
                           uint32_t* out_node_tests, uint32_t* out_node_hits, uint32_t* out_shape_tests);
/* BoundingVolumeHierarchy::any_intersect (bvh.rs:235-302) */
yk_status yk_trace_any(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d,
                       const float* t_max, const int32_t* area_light /* NULL = none */, uint8_t* out_hit);
/* Sampler start_pixel_sample + draws, evaluated on the device.  A sample_index at or past the samples per pixel is served as
 * the reference computes it (accumulation runs past them), except for a stratified sampler whose samples per pixel are no
 * power of two: there the reference's permutation walk need not end, and the call returns YK_ERR_INVALID_ARGUMENT. */
yk_status yk_sampler_sequence(yk_context* ctx, const yk_sampler_desc* sampler, uint16_t px, uint16_t py, uint32_t sample_index,
                              const uint8_t* dims, size_t n_draws, float* out /* 2 per draw */);
/* Camera::ray for every pixel of a tile at one sample index (camera.rs:105-114) */
yk_status yk_camera_rays(yk_context* ctx, const yk_camera* camera, const yk_sampler_desc* sampler, const yk_tile* tile,
                         uint32_t sample_index, float* out_o, float* out_d);
/* device libm used by the kernels: fn 0 sin, 1 cos, 2 tan, 3 log, 4 acos, 5 atan2(x=y_in,y=x_in),
 * 6 sqrt, 7 a/b, 8 f64-sqrt helper, 9 / 10 f32::min / max; 11..27 work on packed triples (n = 3 x count):
 * 11 Vec3::dot, 12 cross, 13 len, 14 normalized, 15 max_dimension, 16 abs, 17 Normal::dot_v, 18 the kx/ky/kz
 * permutation of Triangle::intersect, 19 / 20 Vec3::min / max, 21 Normal::faceforward_v, 22 a + b, 23 a - b,
 * 24 a * b.x, 25 a / b.x, 26 -a, 27 len_sqr (result in out[3k..3k+2]); scalar again: 28 / 29 the sine / cosine of the
 * shared-reduction pair the shading code calls (the same bits as fn 0 / 1) */
yk_status yk_device_math(yk_context* ctx, int fn, size_t n, const float* a, const float* b, float* out);
/* The HOST instance of the same scalar functions (fn 0..5, 28, 29 as above; 30 expf): what the loaders, the camera, the spot
 * light and the roughness remap evaluate on the CPU.  Needs no device. */
yk_status yk_host_math(int fn, size_t n, const float* a, const float* b, float* out);
/* Bsdf::f and Bsdf::sample_f on the device for n (wo, wi|u) pairs against one material */
yk_status yk_bsdf_eval(yk_context* ctx, const yk_material_desc* material, size_t n, const float* n_geom,
                       const float* n_shading, const float* dpdu, const float* wo, const float* wi, float* out_f);
yk_status yk_bsdf_sample(yk_context* ctx, const yk_material_desc* material, size_t n, const float* n_geom,
                         const float* n_shading, const float* dpdu, const float* wo, const float* u, float* out8);

/* Light::sample_li (lights/mod.rs:29-32; point_light.rs:27-50, spot_light.rs:32-80, distant_light.rs:24-43,
 * rectangular_light.rs:46-71) on the device for n surface points against one light, and the ray of the
 * VisibilityTester it returns (visibility.rs:21-23, interaction.rs:44-59).  out: 18 floats per point —
 * l[3], li[3], pdf, has_vis (0/1), area_light (light_index or -1), p1[3], shadow-ray origin[3], direction[3]. */
yk_status yk_light_sample(yk_context* ctx, const yk_light_desc* light, int32_t light_index, size_t n, const float* p,
                          const float* n_geom, const float* u, float* out18);

/* The SurfaceInteraction the integrators read (triangle.rs:141-226, sphere.rs:79-116, interaction.rs:95-164) of the closest hit
 * of n rays, traced by the closest-hit kernel as the render loop launches it.  route 0 builds it from the leaf-order slot that
 * kernel reports, as the Path wavefront, the debug integrators and the guide pass do; route 1 from the source shape through the
 * scene's index-addressed arrays, as Whitted and yk_li_debug do: the two must agree bit for bit.  out: YK_SURFACE_FLOATS floats
 * per ray — hit (0/1), t, p[3], n[3], shading n[3], shading dpdu[3], wo[3], u, v, material, area_light (-1 = none), source shape
 * (-1 on a miss; the three ids as floats, exact below 2^24), barycentrics b0 b1 b2 (0 for a sphere), and the origin[3] of
 * Interaction::spawn_ray (interaction.rs:27-40) for a ray that leaves the hit along ray_d.  A sphere's uv is computed only in a
 * scene with image textures, as in a render.  A miss is all zeros but for the shape.  (Stage tests.) */
#define YK_SURFACE_FLOATS 28
yk_status yk_surface(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d, int32_t route,
                     float* out);

size_t yk_sizeof(int what);

/* ---- several GPUs ------------------------------------------------------
 * The reference renders from ONE process: RenderManager spawns its workers
 * (renderer/render_manager.rs:78-97), hands out the film's tiles — "interleave tiles" is its own
 * TODO (render_manager.rs:206-210) — and every finished tile is written back by
 * Film::update_tile (film.rs:210-282).  yk_multi is that for the GPUs of a node:
 *   - one context and one host thread per device (the thread enqueues that device's render);
 *   - the scene's BVH is built once on the host and copied to every device;
 *   - tile i of the film's outward spiral (film.rs:333-376) belongs to device i mod G; every
 *     device renders its tiles into a dense tile-major slab in its own HBM;
 *   - ONE exchange: the slabs move into device 0's memory with RCCL point-to-point calls
 *     (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd — a gather: tiles are disjoint, so
 *     nothing is reduced) issued on the contexts' own streams, i.e. ordered after each render
 *     without host synchronisation; xGMI links are point to point, every slab takes its own;
 *   - device 0 scatters the slabs into the row-major film (Film::update_tile).
 * Results are bit for bit those of a single-device render of the same film.
 * RCCL is loaded on first use (dlopen: a process that already has it — PyTorch — shares it);
 * without it yk_multi_create on more than one device returns YK_ERR_UNSUPPORTED. */
typedef struct yk_multi yk_multi;
typedef struct yk_multi_scene yk_multi_scene;
typedef struct yk_multi_film yk_multi_film;
/* devices: HIP ordinals, devices[0] assembles the film.  n_devices == 1 is a plain one-GPU
 * render through the same code (no communicator unless "rccl_loopback" is set). */
yk_status yk_multi_create(const int* devices, uint32_t n_devices, yk_multi** out);
/* The same with flags:
 *   YK_MULTI_PEER_COPY       the slabs travel by hipMemcpyPeerAsync on device 0's stream (behind an event of the
 *                            sender's stream) instead of RCCL send / recv — no RCCL needed; also option "peer_copy";
 *   YK_MULTI_SHARED_DEVICES  ranks may name the same device (RCCL refuses two ranks on one device, so this implies
 *                            the peer copy): G ranks on ONE GPU run the deal, the per-rank tile lists, the slab
 *                            layout, the exchange ordering and device 0's scatter exactly as G GPUs would — what a
 *                            one-GPU box can test of the G > 1 path (tests/test_multi_gpu.py). */
#define YK_MULTI_SHARED_DEVICES 1u
#define YK_MULTI_PEER_COPY 2u
yk_status yk_multi_create_ex(const int* devices, uint32_t n_devices, uint32_t flags, yk_multi** out);
/* The deal, without a device: the tiles of `rank` among `n_ranks` — spiral tile i of film_tiles(res, tile_dim)
 * (film.rs:333-376, 409-475) goes to rank i mod n_ranks (render_manager.rs:206-210).  Returns the number of tiles
 * of the rank (0 on a bad argument), writes up to `cap` of them to `out` (may be NULL) and the rank's pixel count
 * to *out_pixels (may be NULL): its slab holds 3 x that many floats, tile after tile, rows top to bottom. */
size_t yk_multi_deal(uint16_t res_x, uint16_t res_y, uint16_t tile_dim, uint32_t n_ranks, uint32_t rank, yk_tile* out, size_t cap,
                     uint64_t* out_pixels);
/* Destroy the films and scenes made from it first or afterwards, in any order; a render must not be in flight. */
void yk_multi_destroy(yk_multi* m);
uint32_t yk_multi_device_count(const yk_multi* m);
/* The context of rank r (options, yk_last_error); owned by the yk_multi. */
yk_context* yk_multi_context(yk_multi* m, uint32_t rank);
/* yk_context_set_option on every context; plus "rccl_loopback" (0 | 1): rank 0's own slab also
 * takes the exchange path (to itself) — exercises the collective on a single GPU; "peer_copy" (0 | 1). */
yk_status yk_multi_set_option(yk_multi* m, const char* key, int64_t value);
yk_status yk_multi_last_error(const yk_multi* m, char* buf, size_t cap);
/* BoundingVolumeHierarchy::new once, one copy per device. */
yk_status yk_multi_scene_create(yk_multi* m, const yk_scene_desc* desc, yk_multi_scene** out);
void yk_multi_scene_destroy(yk_multi_scene* scene);
yk_status yk_multi_scene_get_info(const yk_multi_scene* scene, yk_scene_info* out);
/* The film (film.rs:67-113) and its tile queue: film_tiles(res, tile_dim) dealt round-robin,
 * prepared per device (yk_tile_list), slabs, and the row-major RGB film in device 0's memory. */
yk_status yk_multi_film_create(yk_multi* m, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, yk_multi_film** out);
void yk_multi_film_destroy(yk_multi_film* film);
/* device-0 pointer to res_x * res_y RGB float triples, row-major */
void* yk_multi_film_device_ptr(const yk_multi_film* film);
/* Render the whole film.  film_rgb: host buffer (res_x * res_y * 3 floats) or NULL; stats: sums
 * over the devices (seconds: the slowest device) or NULL.  With both NULL the call only
 * enqueues work (renders, exchange, scatter) and returns: yk_multi_sync waits for it, after
 * which yk_multi_film_device_ptr holds the frame.
 * cancel: the user's predicate is never called concurrently and never again after it returned non-zero — the
 * reference's is a consuming FnMut polled by one thread (render_worker.rs:240-249) — although every device's host
 * thread polls: they share a latch, and the first non-zero answer stops ALL devices (YK_ERR_CANCELLED).  With a
 * predicate the per-device renders are synchronous (it is polled about every 100 us while the GPUs work, see
 * yk_cancel_fn); the film then holds nothing defined. */
yk_status yk_multi_render_film(yk_multi* m, const yk_multi_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                               const yk_integrator_desc* integrator, yk_multi_film* film, float* film_rgb, yk_render_stats* stats,
                               yk_cancel_fn cancel, void* user);
/* The accumulating film over all devices (integrators/mod.rs:146-161 accumulating = true + film.rs:260-272): passes
 * first_sample .. first_sample + n_passes - 1 of EVERY tile in one submission, each added to the film on device 0 —
 * bit for bit the film n_passes single-device submissions produce.  yk_multi_film_clear zeroes the film (a new
 * accumulation: FilmSettings.clear), stream-ordered on device 0. */
yk_status yk_multi_accumulate_film(yk_multi* m, const yk_multi_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                   const yk_integrator_desc* integrator, yk_multi_film* film, uint32_t first_sample, uint32_t n_passes,
                                   float* film_rgb, yk_render_stats* stats, yk_cancel_fn cancel, void* user);
yk_status yk_multi_film_clear(yk_multi* m, yk_multi_film* film);
/* yk_context_interrupt on every rank's context: stops a frame in flight from any thread (the frame's call returns
 * YK_ERR_CANCELLED if it was synchronous); the next frame is unaffected. */
yk_status yk_multi_interrupt(yk_multi* m);
yk_status yk_multi_sync(yk_multi* m);

/* One process per GPU (MPI-style hosts, torch.distributed launchers): the same exchange between
 * processes.  Rank 0 obtains an id (ncclGetUniqueId) and hands it to the other ranks by its own
 * means; every rank then joins with its context (ncclCommInitRank).  yk_dist_gather moves
 * `count` floats from every rank's d_send into rank 0's d_recv[rank * count ...] on `stream`
 * (NULL: the context's stream), without host synchronisation; d_recv is ignored elsewhere.
 * `count` MUST be the same on every rank (the padded maximum of the slab sizes: a rank's send and rank 0's
 * receive are matched by count, unequal values hang the exchange).  The RCCL found at run time must report a 2.x
 * version >= 2.7 (ncclGetVersion), anything else is YK_ERR_UNSUPPORTED. */
#define YK_DIST_ID_BYTES 128
typedef struct yk_dist yk_dist;
yk_status yk_dist_unique_id(uint8_t id[YK_DIST_ID_BYTES]);
yk_status yk_dist_create(yk_context* ctx, const uint8_t id[YK_DIST_ID_BYTES], uint32_t rank, uint32_t world, yk_dist** out);
void yk_dist_destroy(yk_dist* dist);
yk_status yk_dist_gather(yk_dist* dist, const void* d_send, void* d_recv, size_t count, void* stream);

/* ---- many render workers, one device ---------------------------------------------------------------------------
 * The reference renders with num_cpus - 1 worker threads, each calling Integrator::render for ONE tile at a time
 * (render_manager.rs:78-97, render_worker.rs:205-256).  yk_combiner_render_tile is that call for such a thread: it blocks
 * until its tile is rendered, and the calls that are waiting at the same time are merged into one yk_render_tiles
 * submission (the first waiter leads it, the others follow) on one of the combiner's contexts ("lanes": up to
 * n_contexts submissions in flight; all on one device, each context once).  Every caller receives exactly the
 * pixels a single-tile call returns.  max_tiles: most tiles per submission (0 = 64); linger_us: how long a caller
 * that finds itself alone waits for company before it submits.
 *   accumulating_sample < 0: Integrator::render(accumulating = false) — all samples of the pixel, the mean stored;
 *   otherwise accumulating = true with FilmTile.sample = accumulating_sample (one sample, raw value).
 *   Only calls for the same scene, camera, sampler, integrator and mode share a submission.
 *   stats (may be NULL): times are the submission's; rays / shadow_rays / samples are the submission's counts shared
 *   out by tile area with the remainder to the leading call — exact in sum over the callers, which is how the
 *   reference uses them (render_manager.rs:277-281).
 *   cancel: polled by the calling thread itself about every 100 us while it waits (the reference's predicate consumes
 *   a channel message, render_worker.rs:240-249, so it must fire in its own worker).  Fired while the tile is still
 *   queued: the call returns YK_ERR_CANCELLED at once.  Fired while the tile is part of a running submission: that
 *   submission is interrupted; callers whose predicate has fired return YK_ERR_CANCELLED, the other callers' tiles
 *   are queued again — nobody is handed pixels of an interrupted job. */
typedef struct yk_combiner yk_combiner;
typedef struct yk_combiner_info {
    uint64_t submissions, tiles, requeued; /* submissions made, tiles rendered through them, tiles queued again after an interruption */
    uint32_t largest_submission, lanes;
} yk_combiner_info;
yk_status yk_combiner_create(yk_context* const* contexts, uint32_t n_contexts, uint32_t max_tiles, uint32_t linger_us, yk_combiner** out);
void yk_combiner_destroy(yk_combiner* combiner); /* no call may be waiting in it */
yk_status yk_combiner_render_tile(yk_combiner* combiner, const yk_scene* scene, const yk_camera* camera, const yk_sampler_desc* sampler,
                                  const yk_integrator_desc* integrator, const yk_tile* tile, int32_t accumulating_sample, float* tile_pixels,
                                  yk_render_stats* stats, yk_cancel_fn cancel, void* user);
yk_status yk_combiner_get_info(const yk_combiner* combiner, yk_combiner_info* out);
yk_status yk_combiner_last_error(const yk_combiner* combiner, char* buf, size_t cap);

/* ---- scene input -------------------------------------------
 * The reference's loaders, host-only (no device needed): they produce the flattened
 * scene description yk_scene_create consumes plus the camera and film settings the
 * reference's `load` functions return.
 *   yk_load_ply   Scene::ply          scene/mod.rs:99-152 + ply::load scene/ply.rs:19-130
 *                 (white matte, fit-to-unit-cube transform, point light, 640x480 camera)
 *   yk_load_pbrt  scene::pbrt::load   scene/pbrt/mod.rs:94-857 — the subset the reference
 *                 implements: perspective Camera, Film resolution, LookAt, Translate/Scale/
 *                 Rotate, Attribute/Transform blocks, Include, (Make)NamedMaterial/Material
 *                 {matte,glass,glossy,metal}, LightSource {infinite,distant,point}, Shape
 *                 {sphere,trianglemesh,plymesh}, Texture "spectrum" "imagemap" for matte Kd.
 *   yk_load_mitsuba  scene::mitsuba::load  scene/mitsuba/mod.rs:28-218 — Mitsuba 2.1.0 XML as far as
 *                 the reference reads it: sensor (fov, fov_axis, transform), default resx / resy,
 *                 bsdf {diffuse,twosided,dielectric}, emitter {constant,point,spot}, shape "ply" with
 *                 a transform; everything is mirrored by scale(-1, 1, 1) on the way in.
 *   yk_load_scene    try_load_scene  app/util.rs:15-63 — one of the three by file extension.
 * split_method / max_shapes_in_node are SceneLoadSettings (scene/mod.rs:25-39) and are
 * copied into the description.  Errors: where the reference returns LoadError or panics
 * the call returns non-zero and yk_loader_last_error() (thread-local) holds the reason. */
/* ImageTexture::new(path) (textures/image_texture.rs:66-70,114-141): decode an image file
 * into RGB f32 (u8 / 255, u16 / 65535, float as is, no gamma, alpha dropped).  The decoder
 * is chosen from the file extension like image::io::Reader::open: .png, .bmp, .tga,
 * .ppm/.pnm, .qoi, .ff (farbfeld), .exr (scan-line, none/ZIPS/ZIP); the `image` crate's
 * remaining formats (JPEG, GIF, TIFF, WebP, HDR ...) return YK_ERR_UNSUPPORTED; grey files
 * are the reference's "Unsupported image format".  out->rgb is owned by the library:
 * yk_image_texture_free. */
yk_status yk_image_texture_load(const char* path, yk_texture_desc* out);
void yk_image_texture_free(yk_texture_desc* tex);

typedef struct yk_loaded_scene yk_loaded_scene;
yk_status yk_load_ply(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out);
yk_status yk_load_pbrt(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out);
/* scene::mitsuba::load (scene/mitsuba/mod.rs:28-218) */
yk_status yk_load_mitsuba(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out);
/* app/util.rs:15-63 try_load_scene: by extension — "ply", "xml", "pbrt" (exact, case-sensitive like the
 * reference's match); anything else YK_ERR_INVALID_ARGUMENT with the reference's message ("Unknown extension
 * 'x'", "Expected a file with an extension", "Scene does not exist '...'").  The empty path (the Cornell box
 * in the reference) is YK_ERR_INVALID_ARGUMENT here: that scene is built by the caller (scenes.cornell()). */
yk_status yk_load_scene(const char* path, uint32_t split_method, uint32_t max_shapes_in_node, yk_loaded_scene** out);
/* Pointers written into *desc stay valid until yk_loaded_scene_destroy.  camera->res_x/res_y
 * carry FilmSettings.res; *tile_dim its tile_dim (16).  camera / tile_dim may be NULL. */
yk_status yk_loaded_scene_get(const yk_loaded_scene* loaded, yk_scene_desc* desc, yk_camera_params* camera, uint16_t* tile_dim);
void yk_loaded_scene_destroy(yk_loaded_scene* loaded);
const char* yk_loader_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* YUKI_HIP_H */
