// yk_internal.h — library-private definitions shared by the host files of the library (yk_context.cpp,
// yk_scene.cpp, yk_scene_change.cpp, yk_render.cpp, yk_stages.cpp: the single-device entry points; yk_multi.cpp: several devices of
// one process, RCCL): the objects behind the opaque handles of include/yuki_hip.h.  Not installed.
// Two private headers build on it: yk_staging.h (the staged arrays of a host-array entry point, the one user of
// yk_context::scratch) and yk_film_call.h (what the film passes' argument checks share).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "yk_device.h"
#include "yk_host.h"
#include "yk_kernels.h"
#include "yk_scene_input.h"
#include "yk_scene_records.h"

using namespace yk;

// ------------------------------------------------------------------ helpers
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t want) {
        if (want <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
// `bytes` of a host array into `buf`, grown to hold them (never smaller than 16 bytes)
static inline hipError_t put_host_array(DevBuf& buf, const void* src, size_t bytes) {
    hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
    if (e == hipSuccess && bytes) e = hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice);
    return e;
}

// ... and what a failed device call says to the code that falls back instead of failing (YK_LAYOUT_REASON_*); clears the error
static inline uint32_t layout_reason_of(hipError_t e) {
    (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? YK_LAYOUT_REASON_OUT_OF_MEMORY : YK_LAYOUT_REASON_DEVICE_ERROR;
}

// A function's device temporaries: freed on every way out, unless handed on.
struct DevScratch {
    std::vector<void*> all;
    hipError_t err = hipSuccess;  // of the allocation that failed
    ~DevScratch() {
        for (void* p : all) (void)hipFree(p);
    }
    template <class T> bool get(T*& out, size_t count) {
        void* p = nullptr;
        if ((err = hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16))) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        all.push_back(p);
        out = reinterpret_cast<T*>(p);
        return true;
    }
    template <class T> void give(T* p, size_t count, DevBuf& to) {  // hands one buffer on to a new owner
        all.erase(std::find(all.begin(), all.end(), (void*)p));
        to.release();
        to.p = p;
        to.bytes = std::max<size_t>(count * sizeof(T), 16);
    }
};

#define YK_ALBEDO_MEAN_SCRATCH ((size_t)64 << 20)  // the band scratch budget of yk_render_albedo_mean (the measurement)
#define YK_BVH_SMALL_RANGE 32  // default of "bvh_small_range" (profiles/bvh_build_device.json: the sweep that chose it)

struct yk_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string last_error;
    int n_cu = 256;
    // options
    int64_t batch_paths = 128 << 20;
    int64_t packet_bounces = 1;         // leading bounces whose closest-hit rays use the wave-packet kernel (camera rays are coherent); 0 = never
    int64_t packet_shadow_bounces = 1;  // same for the shadow rays towards point / spot / distant lights (their own queue)
    int64_t nee_skip = 2;        // light work no result reads that the light loops leave out, a bit mask (yk_device.h, YK_NEE_SKIP_*): 2 no trace of a shadow ray whose contribution is +-0; 0 = every ray
    int64_t shade_reorder = 1;   // deal the paths of a shade block to its lanes sorted by material kind (bounces > 0)
    int64_t overlap_shadow = 1;  // run {trace_any, accumulate}(b) on a side stream beside trace_closest(b+1)
    int64_t wide_bvh = 2;   // scenes created afterwards: 0 binary nodes only, 1 traverse the 4-wide collapse, 2 keep both and pick per job
    int64_t top_nodes = YK_TOP_MAX; // interior nodes (capped by what the kernels were built for) of the first tree levels the traversal kernels keep in LDS
    int64_t bvh_builder = 0;       // scenes created afterwards: 0 the host recursion builds the tree, 1 the device builder where the input qualifies (yk_bvh_build.hip)
    int64_t bvh_small_range = YK_BVH_SMALL_RANGE;  // ranges of at most this many shapes are finished by one lane each
    int64_t scene_layout = 0;      // scenes created afterwards: 0 the device records are laid out on the host and uploaded, 1 on the device (yk_scene_layout.hip)
    int64_t trace_stage_kernel = 0;  // which kernels yk_trace_closest / yk_trace_any launch (yk_stages.cpp): 0 generic, API flavour | 1 generic, render-loop flavour | 2 wave packets
    int64_t update_top_block = 1;    // yk_scene_update, device route: 1 the tree's top levels of at most a block's lanes are finished by one block | 0 one launch per level throughout (the measurement)
    int64_t sample_buf_cap = (int64_t)64 << 30;
    int64_t time_kernels = 1;
    int64_t streams = 2;  // batches in flight (1 or 2): the second stream's launches fill the first one's tails
    // per-stream work buffers
    struct WorkSet {
        DevBuf path[2][4];
        DevBuf hit, pend, shO, shD, shC, vis, shq, shO2, shD2, shq2, ctrl, spill, spill_side;
        size_t cap_paths = 0;
        unsigned cap_lights = 0, cap_area = 0, cap_delta = 0;
        hipStream_t stream = nullptr;
        hipStream_t side = nullptr;  // shadow rays + accumulate of bounce b run here beside trace of bounce b+1
        hipEvent_t done = nullptr, ev_shade = nullptr, ev_acc = nullptr;
        hipEvent_t ev_batch = nullptr;  // end of the work set's latest batch (pacing of interruptible jobs, yk_render.cpp)
    } ws[2];
    DevBuf sample_buf, pixel_xy, pixel_aux, tiles, tile_off, counters, stats4, hit4;
    DevBuf tile_sample, pixel_sample;  // an accumulating render's per-tile sample indices and the per-pixel table made of them
    DevBuf film_tiles, film_tile_off, film_pixel_xy;  // yk_film_update_tiles_device's tables: on the caller's stream, so not the render's
    DevBuf scratch[8];  // the staged arrays of the host-array entry point in progress: indexed by yk_staging.h only
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;  // hand-over between a caller's stream and the context's own
    // Interruption (yk_device.h, CancelRef): cancel_host[0] is the word the kernels poll across PCIe (pinned, mapped, coherent host
    // memory; cancel_host_dev is its device address); cancel_raised remembers that a submission left it set — the next one waits
    // for the context's streams before it clears the word, so that no kernel of the interrupted submission resumes.
    unsigned* cancel_host = nullptr;  // [0] the word, [16] a constant 1: the source of the host's copy into the device word
    const unsigned* cancel_host_dev = nullptr;
    hipStream_t cancel_stream = nullptr;  // carries that copy past the kernels in flight (made after the context's first interruption)
    bool want_cancel_stream = false;
    std::atomic<bool> cancel_raised{false};
    // the tone map's buffers (yk_tonemap.hip), grown on first use
    struct ToneMapState {
        DevBuf partials, bounds, samples;  // per-block (min, max) pairs, the bounds slot, the sample table on the device
        uint32_t* staging = nullptr;       // pinned host copy the sample table is uploaded from
        size_t staging_words = 0;
        hipEvent_t staged = nullptr;       // the latest upload out of `staging`
    } tonemap;
    // the denoiser's buffers (yk_denoise.hip), grown on first use and again when a larger film comes
    struct DenoiseState {
        DevBuf ping[2];   // the colours between two iterations, 16 bytes a pixel each
        DevBuf samples;   // the sample table on the device (staged through the tone map's pinned copy)
        int64_t lds_max_step = 2;  // "denoise_lds_max_step": iterations with a step up to this (0, 1 or 2) stage their taps in LDS (the measurement that chose 2)
    } denoise;
    // the temporal passes' buffer (yk_temporal.hip), grown on first use
    struct TemporalState {
        DevBuf samples;   // blend's sample table on the device (staged through the tone map's pinned copy)
    } temporal;
    // the overlay pass's buffers (yk_overlay.hip), grown on first use
    struct OverlayState {
        DevBuf ids;        // one u32 a pixel: the winning ordinal + 1
        int64_t coop_min = 32;  // "overlay_coop_min": segments of at least this many pixels are drawn by a whole wave
    } overlay;
    // the adaptive selection's scratch (yk_adaptive.hip), grown on first use: a selection ends with a synchronisation, so
    // the next one finds it free whatever stream it runs on
    struct AdaptiveState {
        DevBuf rank;        // one u32 a pixel: the rank inside its 16 x 16 tile, or ~0 where the pixel is not selected
        DevBuf tile_count;  // one u32 a tile: the tile's count, then its base; one more word: the total
    } adaptive;
    // the fused pixel-mean albedo's scratch (yk_render_albedo_mean, yk_render.cpp): the ids of one band of the large film
    struct AlbedoMeanState {
        DevBuf ids_band;        // YK_ALBEDO_MEAN_SCRATCH bytes from the first call on; more only for a band that needs more
        int64_t band_rows = 0;  // "albedo_mean_band_rows": output rows per band; 0 = as many as fit the scratch budget
    } albedo_mean;
    // the exposure meter's buffers (yk_exposure.hip), grown on first use
    struct ExposureState {
        DevBuf slot;     // EX_SUB_SLOTS x EX_SLOT_WORDS u32: partial histograms and side counts, zeroed on the stream before every pass
        DevBuf samples;  // the sample table on the device (staged through the tone map's pinned copy)
        int64_t wave_combine = 1;  // "exposure_wave_combine": a wave whose lanes all hit one bin adds once
    } exposure;
    // every entry point that touches the context's buffers or streams holds this: calls on one
    // context from several host threads (the reference's tile workers) are serialised
    std::recursive_mutex mu;
    // the guided upsample's buffer (yk_upsample.hip), grown on first use.  It stands after every older member: their
    // offsets, and with them the objects of the files that do not know this pass, stay what they were.
    struct UpsampleState {
        DevBuf samples;  // the LOW film's sample table on the device (staged through the tone map's pinned copy)
    } upsample;
};

typedef yk_context::WorkSet WorkSet;
static const uint32_t YK_WIDE_MAX_PATHS = 6u << 20;  // jobs up to this many paths traverse the 4-wide nodes (wide_bvh = 2)

// A tree in HBM: the builder's 32-byte nodes (8 words each, yk_bvh_build.h), every node's depth and the leaf order —
// left there by build_bvh_device for the device layout, or uploaded for it from a host-built tree.
struct DeviceTree {
    DevBuf nodes, depth, order;
    uint32_t n_nodes = 0, n_shapes = 0;
    uint32_t root_words[8] = {};  // node 0
    void release() {
        nodes.release();
        depth.release();
        order.release();
    }
};

struct yk_scene {
    int device = -1;  // a scene belongs to the device, not to the context that made it: any context there renders it, and it may outlive them
    // One host tree may serve the copies of a scene on several devices (yk_multi_scene).  Its scalars (depth, max_leaf_shapes)
    // are always there; a device-built, device-laid scene leaves `nodes` and `shape_order` in HBM (tree_nodes, tree_order)
    // until something reads them: every reader of the two arrays goes through scene_host_tree().
    std::shared_ptr<const HostBvh> bvh;
    std::shared_ptr<HostBvh> bvh_lazy;  // the same object, writable: set while the arrays are still to be fetched
    DevBuf tree_nodes, tree_order;
    // tree_fetched says whether the host arrays are current; a device-route update (yk_scene_update.hip) clears it again
    mutable std::mutex tree_mu;
    mutable std::atomic<uint32_t> tree_fetched{1};
    yk_scene_layout_info layout = {};
    size_t record_bytes[7] = {};  // exact sizes of the seven record buffers (YK_RECORDS_*; a DevBuf is never smaller than 16 bytes)
    uint32_t n_triangles = 0, n_spheres = 0, n_lights = 0, n_delta_lights = 0;
    uint32_t n_materials = 0, n_meshes = 0, n_textures = 0;
    bool wide_auto = false;  // both node layouts on the device: the 4-wide one is used for jobs below YK_WIDE_MAX_PATHS
    yk_scene_info info;
    yk_bvh_build_info build_info;
    // source shape -> device BSDF kind of its material (the kind bits of a render-loop hit word).  A scene made from device arrays
    // (yk_scene_create_device) has no host copy of tri_material: it keeps the kind of every material and of every sphere
    // (lazy_mat_kind, lazy_sphere_kind) and fills the table from its device copy on the first call that reads it: every reader
    // goes through scene_shape_kind().
    mutable std::vector<uint8_t> shape_kind;
    std::vector<uint8_t> lazy_mat_kind, lazy_sphere_kind;
    bool shape_kind_lazy = false;
    mutable std::once_flag kind_once;
    mutable std::atomic<uint32_t> kind_fetched{1};
    // device
    DevBuf nodes, nodes4, top_nodes, top_nodes_any, tris, prim_shade, prim_attr, indices, points, normals, uvs, tri_mesh, tri_material, tri_area_light, mesh_flags, materials, lights, spheres, texels, tex_info;
    DevScene dev;
    bool on_device = false;
    // What a change in place needs after creation (yk_scene_update.h, yk_scene_change.h).
    struct UpdateState {
        uint32_t n_vertices = 0;
        bool has_normals = false, has_uvs = false;
        LayoutOptions opt;  // the context's "top_nodes" / "wide_bvh" at creation: every layout of the scene, then and at an update, reads these
        std::vector<float> sphere_bounds;     // six floats a sphere: Sphere::world_bound as at creation or as the last edit left it
        std::vector<uint8_t> mat_kind;        // device BSDF kind (MK_*) per material
        std::vector<uint8_t> light_kind;      // yk_light_kind per light: an edit keeps it
        // the plan of the device route, built by the first update that takes it: the tree's nodes and order stay in
        // tree_nodes / tree_order; depth = every node's depth; list = the interior nodes grouped by depth (level_off[d] ..
        // level_off[d + 1] holds depth d + 1), then the leaves (from level_off[n_levels])
        bool planned = false;
        DevBuf depth, list, sphere_b, mat_kind_d, words;
        std::vector<uint32_t> level_off;
        yk_scene_update_info info = {};
        yk_scene_edit_info edit_info = {};
    } upd;
    // A scene's arrays on the host: what a host-only scene keeps (`host`; points: the vertices the tree was last fitted to; materials
    // and spheres follow an edit), and what scene_host_arrays() fills for a call on a scene in device memory.  Every reader goes there.
    struct HostCopy {
        std::vector<uint32_t> indices, tri_mesh, mesh_flags;
        std::vector<int32_t> tri_material, tri_area_light;  // (the last one and the normals: only ever fetched)
        std::vector<float> points, normals, uvs;
        std::vector<Material> materials;
        std::vector<DevSphere> spheres;
        std::vector<float4> texels;
        std::vector<uint4> tex_info;
    } host;
    // What yk_scene_transform keeps between calls (yk_scene_transform.h): the rest pose, snapshotted by the first transform after
    // creation or an update, and the table vertex -> mesh.  A scene in device memory keeps them there (rest_points, rest_normals,
    // vertex_mesh: two words a vertex; mesh_words: per mesh its lit bit, then its kind of the call in progress), a host-only
    // scene in the vectors.  It stands after every older member: their offsets, and with them the objects of the files that
    // do not know this call, stay what they were.
    struct TransformState {
        bool active = false;   // the rest copy is valid
        bool shared = false;   // a vertex is indexed by triangles of two meshes: every transform is refused
        DevBuf rest_points, rest_normals, vertex_mesh, mesh_words, cost_words;
        std::vector<float> h_rest_points;                  // a host-only scene (it keeps no normals)
        std::vector<uint32_t> h_vertex_mesh, h_mesh_lit;
        std::vector<uint32_t> flags_created;  // YK_MESH_* per mesh as creation made them (the rest pose on the host)
        yk_scene_transform_info info = {};
    } xf;
};

// The device scene a job of `n` rays traverses: with both node layouts present the 4-wide one
// serves small jobs only (see run_bounces).
static inline DevScene dev_scene_for(const yk_scene* scene, uint64_t n) {
    DevScene ds = scene->dev;
    if (scene->wide_auto && n > YK_WIDE_MAX_PATHS) ds.nodes4 = nullptr;
    return ds;
}

// A tile list prepared once and reused every frame (the GPU worker renders the same tiles
// over and over): host copy + the device pixel table, so that rendering and the film update
// need no upload and no host synchronisation.
struct yk_tile_list {
    int device = -1;
    std::vector<yk_tile> tiles;
    std::vector<uint16_t> samples;  // empty: plain film
    std::vector<uint32_t> off;      // n_tiles + 1 pixel offsets
    DevBuf pixel_xy, pixel_sample;
};

// (pixel, first sample index) entries in HBM with room for every pixel of a res_x x res_y film (yk_adaptive.h): filled by
// the selection kernels or by yk_pixel_list_set, which checks what it uploads — no kernel indexes a film with a
// coordinate that was not checked.
struct yk_pixel_list {
    yk_context* ctx = nullptr;
    uint32_t res_x = 0, res_y = 0;
    uint32_t n = 0;           // entries, known to the host
    uint32_t passes = 0;      // the round size the entries were chosen for
    uint32_t sample_end = 0;  // sample + passes <= sample_end for every entry
    DevBuf pixel_xy, pixel_sample;
};

// The message of a call that has no context to leave it in (a host-only scene): per thread, read and cleared by
// yk_last_error(NULL, ...).
inline std::string& host_last_error() {
    static thread_local std::string msg;
    return msg;
}
static inline yk_status fail(yk_context* ctx, yk_status st, const std::string& msg) {
    if (ctx)
        ctx->last_error = msg;
    else
        host_last_error() = msg;
    return st;
}

#define YK_LOCK(ctx) std::lock_guard<std::recursive_mutex> yk_lock_((ctx)->mu)
#define HIP_TRY(ctx, expr)                                                                                           \
    do {                                                                                                             \
        hipError_t _e = (expr);                                                                                      \
        if (_e != hipSuccess) {                                                                                      \
            return fail(ctx, _e == hipErrorOutOfMemory ? YK_ERR_OUT_OF_MEMORY : YK_ERR_DEVICE,                       \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                                          \
        }                                                                                                            \
    } while (0)

// No exception crosses the C ABI (undefined behaviour for a Rust caller, an abort under ctypes): entry points that
// allocate host memory are function-try-blocks ending in this handler.
#define YK_CATCH(ctx)                                                                                         \
    catch (const std::bad_alloc&) { return fail(ctx, YK_ERR_OUT_OF_MEMORY, "host allocation failed"); }      \
    catch (const std::exception& e) { return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string("exception: ") + e.what()); }


// The inputs of the scene pipeline as yk_scene_create derives them from a description on the host — the
// reference's BVH (BoundingVolumeHierarchy::new, bvh.rs:39-115), the small tables, the context's LayoutOptions — and, where
// the host lays out, the records.  Built once; uploaded to one device or to every device of a yk_multi.
struct SceneImage;
// What yk_build_scene_image builds: who builds the tree, who lays out the records, and the YK_LAYOUT_REASON_* to report
// where the device layout was asked for but is not attempted.
struct SceneBuild {
    bool device_builder, device_layout;
    uint32_t layout_reason;
};
yk_status yk_build_scene_image(yk_context* opt_ctx, const yk_scene_desc* d, std::shared_ptr<SceneImage>& out, const SceneBuild& what);
yk_status yk_upload_scene_image(yk_context* ctx, const std::shared_ptr<SceneImage>& img, yk_scene** out);

// The scene's host tree with its node and shape-order arrays, copied back from HBM on the first call when the scene kept
// them there (thread-safe).  NULL when that copy fails.
const HostBvh* scene_host_tree(const yk_scene* scene);

// A scene's arrays on the host, as scene_host_tree() gives its tree: `mask` says which (HOST_*).  A host-only scene answers
// with its kept copy (`who` prefixes its refusals), a scene in device memory with copies fetched and size-checked for the call.
enum : uint32_t { HOST_INDICES = 1u, HOST_POINTS = 2u, HOST_NORMALS = 4u, HOST_UVS = 8u, HOST_TRI_MESH = 16u, HOST_TRI_MATERIAL = 32u, HOST_TRI_AREA_LIGHT = 64u,
                  HOST_MESH_FLAGS = 128u, HOST_MATERIALS = 256u, HOST_SPHERES = 512u, HOST_TEXTURES = 1024u /* tex_info and texels */ };
struct HostArrays {
    const yk_scene::HostCopy* arrays = nullptr;  // the scene's, or `fetched`
    yk_scene::HostCopy fetched;
    const yk_scene::HostCopy* operator->() const { return arrays; }
};
yk_status scene_host_arrays(yk_context* ctx, const yk_scene* scene, uint32_t mask, const std::string& who, HostArrays& out);

// The scene's shape -> BSDF kind table, filled from the device copy of tri_material on the first call when the scene was
// made from device arrays (thread-safe).  NULL when that copy fails.
const std::vector<uint8_t>* scene_shape_kind(const yk_scene* scene);

static inline double now_seconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ------------------------------------------------------------------ yk_bvh_build.hip
// The level-synchronous builder (yk_bvh_build.h) on the device and its host instance.  Both return true with the
// host recursion's tree in `out`, or false with bi.reason set and `out` untouched: the caller then runs build_bvh.
// With `keep`, build_bvh_device leaves nodes, depths and order in HBM (DeviceTree) instead of copying them back: `out` then
// receives the scalars only and its two arrays stay empty.
bool build_bvh_device(yk_context* ctx, const std::vector<ShapeBounds>& bounds, uint32_t max_shapes_in_node, uint32_t split_method, uint32_t small_range, HostBvh& out, yk_bvh_build_info& bi,
                      DeviceTree* keep = nullptr);
// The same with the bounds (six floats a shape: min.xyz, max.xyz) given as a host array or, d_bounds != NULL, in HBM already.
bool build_bvh_device(yk_context* ctx, const ShapeBounds* h_bounds, const float* d_bounds, size_t n_bounds, uint32_t max_shapes_in_node, uint32_t split_method, uint32_t small_range, HostBvh& out,
                      yk_bvh_build_info& bi, DeviceTree* keep);
bool build_bvh_levels(const std::vector<ShapeBounds>& bounds, uint32_t max_shapes_in_node, uint32_t split_method, uint32_t small_range, HostBvh& out, yk_bvh_build_info& bi);

// ------------------------------------------------------------------ yk_scene_layout.hip
// The device records of `s` (nodes, nodes4, top_nodes, top_nodes_any, tris, prim_shade, prim_attr; s->layout, s->record_bytes)
// from the tree in HBM and the scene's own uploaded arrays.  d_user_order (may be NULL): the caller's shape order, applied to
// tree.order in place first (*order_applied says whether that happened).  Returns YK_LAYOUT_REASON_NONE, or the reason with the scene's records undefined.
// "top_nodes" and "wide_bvh" are s->upd.opt, the values captured at creation, as for the host layout.
uint32_t layout_scene_device(yk_context* ctx, yk_scene* s, const DeviceTree& tree, const uint32_t* d_user_order, const uint8_t* d_mat_kind, bool has_attr, uint32_t tree_depth, bool* order_applied);

// ------------------------------------------------------------------ yk_scene_update.hip, yk_scene_edit.hip
// The device route of a change in place, step by step (yk_scene_change.cpp runs them; the refit rule is yk_scene_update.h's): the
// plan, built once and kept; stage, one kernel that tests the caller's array and raises *flag, nothing of the scene written; commit,
// device-to-device copies into the scene's arrays; refit, from the scene's own arrays, the boxes (`boxes` false: the tree stays) and
// the layout's records, with their times.  Every step returns YK_LAYOUT_REASON_*: NONE, or why the host route must rewrite the scene.
uint32_t plan_scene_update(yk_context* ctx, yk_scene* s);
uint32_t refit_scene_device(yk_context* ctx, yk_scene* s, bool boxes, double* seconds_boxes, double* seconds_records);
// points (yk_scene_update), after the plan, the context's device current: *flag non-zero says a coordinate is not finite
uint32_t stage_points_device(yk_context* ctx, yk_scene* s, const float* d_points, uint32_t* flag);
uint32_t commit_points_device(yk_context* ctx, yk_scene* s, const float* d_points, const float* d_normals);
// spheres (yk_scene_apply_edit).  d_in: n_spheres yk_sphere_desc records in HBM (4-byte aligned).  stage writes the DevSphere
// table, the six-float bounds and the material column into `staged` (scratch of the caller) and raises *flag (YK_SPHERES_*);
// commit copies them into the scene's sphere table and the plan's bounds, and back to the host (bounds, material column).
enum { YK_SPHERES_NOT_FINITE = 1u, YK_SPHERES_MATERIAL = 2u };
struct StagedSpheres {
    DevSphere* table = nullptr;
    float* bounds = nullptr;
    int32_t* material = nullptr;
};
uint32_t stage_spheres_device(yk_context* ctx, yk_scene* s, const void* d_in, DevScratch& tmp, StagedSpheres* staged, uint32_t* flag);
uint32_t commit_spheres_device(yk_context* ctx, yk_scene* s, const StagedSpheres& staged, std::vector<int32_t>* material);

// ------------------------------------------------------------------ yk_scene_transform.hip
// The steps of yk_scene_transform on a scene in device memory (the rule: yk_scene_transform.h), each YK_LAYOUT_REASON_*:
// snapshot: the rest copy and the table vertex -> mesh where the scene has none yet (s->xf; rest_bytes go into device_bytes),
//   with tree_cost_rest from the tree in HBM (`tree_on_device`) or from the host tree;
// stage: the per-mesh kinds and the check pass over d_transforms (n_meshes records in HBM): *flag gets the XF_BAD_* bits,
//   counts[0 .. 1] the moved and flipped meshes; nothing of the scene is written;
// commit: the write pass: points, normals, mesh flags;
// tree_cost_device: the cost of the tree in s->tree_nodes.
uint32_t snapshot_rest_device(yk_context* ctx, yk_scene* s, bool tree_on_device);
uint32_t stage_transforms_device(yk_context* ctx, yk_scene* s, const void* d_transforms, uint32_t* flag, uint32_t* counts);
uint32_t commit_transforms_device(yk_context* ctx, yk_scene* s, const void* d_transforms);
uint32_t tree_cost_device(yk_context* ctx, yk_scene* s, double* cost);
// the rest copy goes, the mesh flags are creation's again (yk_scene_update*); the scene's device is current
yk_status drop_rest(yk_context* ctx, yk_scene* s);

// ------------------------------------------------------------------ yk_scene_input.hip
// The input stage of yk_scene_create_device (yk_scene_input.h); both enqueue on `st` and return the launch status.
// Checks: d_words receives the first failing per-triangle check, the first triangle that breaks the area-light rule and,
// with d_order, whether it is a permutation of n_shapes shapes (d_seen: one bit a shape).  They read the index arrays and
// d_light_kind (yk_light_kind per light) only.
hipError_t enqueue_geometry_checks(hipStream_t st, const inp::Geometry& g, const uint8_t* d_light_kind, const uint32_t* d_order, uint32_t n_shapes, uint32_t* d_seen, inp::CheckWords* d_words);
// d_sb[6 p ..]: the world bound of the shape at position p of the shape order (d_order, may be NULL); d_sphere_bounds: six
// floats a sphere.  Only for arrays the checks have passed.  Sets d_words->non_finite (cleared by enqueue_geometry_checks)
// when a triangle has a coordinate that is not finite.
hipError_t enqueue_shape_bounds(hipStream_t st, const float* d_points, const uint32_t* d_indices, const uint32_t* d_order, const float* d_sphere_bounds, uint32_t n_triangles, uint32_t n_shapes, float* d_sb,
                                inp::CheckWords* d_words);

// ------------------------------------------------------------------ yk_tonemap.hip
// A host sample table (Film.samples: one entry per tile of the film, partial tiles included) -> `dst` on the device, enqueued
// on `st`.  It goes through the context's pinned staging (tonemap.staging), so the upload is truly asynchronous; the staging
// is rewritten only once the previous upload out of it has run.
yk_status stage_sample_table(yk_context* ctx, hipStream_t st, const uint32_t* samples, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, DevBuf& dst);
// The same for a table the call may leave out: *d_samples is the table in `dst`, or NULL when `samples` is.
inline yk_status stage_samples(yk_context* ctx, hipStream_t st, const uint32_t* samples, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, DevBuf& dst, const uint32_t** d_samples) {
    *d_samples = nullptr;
    if (!samples) return YK_OK;
    yk_status s = stage_sample_table(ctx, st, samples, res_x, res_y, tile_dim, dst);
    if (s == YK_OK) *d_samples = dst.as<const uint32_t>();
    return s;
}

// ------------------------------------------------------------------ yk_adaptive.hip
// The selection (yk_adaptive.h) of device statistics of the list's resolution into `list`, on `st`; synchronises once to read
// the count, which it leaves in the list and in *out_n.  The caller holds the lock and has checked desc, pointer and list.
yk_status adaptive_select_into(yk_context* ctx, hipStream_t st, const yk_adaptive_desc* desc, const void* d_stats, yk_pixel_list* list, uint32_t* out_n);

// ------------------------------------------------------------------ yk_scene.cpp
// The exact sizes of a scene's seven record buffers (s->record_bytes) and the head of s->layout from what was laid out,
// for whoever laid it out.  n_wide: DevNode4 records; 0 says there is no 4-wide layout.
void set_record_layout(yk_scene* s, size_t n_interior, size_t n_wide, size_t n_top, size_t n_top_any, size_t n_shapes, bool has_attr, uint32_t root_ref, bool wide_auto);
// A host tree into HBM for device work (the device layout, the plan of the device-route update): nodes, every node's
// depth (lay::node_depths) and the order, with the counts and node 0.
hipError_t upload_host_tree(const HostBvh& bvh, DeviceTree& tree);
// The tree's three buffers become the scene's (tree_nodes, tree_order, upd.depth); what the scene held comes back in
// `tree`.  `lazy` (may be NULL): the host tree whose arrays are still to be fetched from them (scene_host_tree).
void adopt_device_tree(yk_scene* s, DeviceTree& tree, const std::shared_ptr<HostBvh>& lazy);
Material make_material(const yk_material_desc& m);  // per-hit constants folded (GGX alpha, Oren-Nayar A / B)
DevLight make_light(const yk_light_desc& l);
DevSphere make_sphere(const yk_sphere_desc& sp);  // with Transform::swaps_handedness of object_to_world
// host array -> device buffer.  Not put_host_array inside HIP_TRY: the context's message names the call that failed
// ("buf.ensure(bytes): ..." or "hipMemcpy(...): ..."), and those texts stay.
template <class T> static yk_status upload(yk_context* ctx, DevBuf& buf, const T* src, size_t count) {
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    HIP_TRY(ctx, buf.ensure(bytes));
    if (count) HIP_TRY(ctx, hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return YK_OK;
}
// The seven record vectors of a host layout into the scene's record buffers, and the sizes and layout head that go with them.
yk_status upload_records(yk_context* ctx, yk_scene* s, const SceneRecords& r);
// What the kernels are handed of the records and the root box (which reaches DevScene here only): at creation, and after a change.
void bind_records(yk_scene* s);
// every non-NULL array is device memory of ctx's device, and its allocation reaches as far as its count says
struct DeviceArray { const char* name; const void* p; size_t bytes; };
yk_status check_device_arrays(yk_context* ctx, std::initializer_list<DeviceArray> arrays);
// The context's stream waits for what the caller's stream (a hipStream_t, may be NULL) holds now: its arrays are complete there.
yk_status wait_for_caller_stream(yk_context* ctx, void* stream);

// ------------------------------------------------------------------ yk_render.cpp (used by yk_stages.cpp too)
// ctx->counters: 8 x u64 (closest-hit rays, shadow rays, ...) followed by a 4-word error block whose word
// YK_CTRL_ERR the traversal kernels set on a stack overflow and whose word YK_CTRL_CANCELLED says that the render was interrupted.
// Both are zeroed ONCE per call — the per-batch control blocks of the work sets are zeroed with every batch and must not hold the flags.
// The error block has a 128-byte line of its own: its word YK_CTRL_CANCELLED is read by every kernel that starts, the counters
// before it take an atomic per wave.
#define YK_COUNTER_BYTES 256
unsigned* error_block(yk_context* ctx);
CancelRef cancel_ref(yk_context* ctx);  // the context's interruption words, as the kernels take them
yk_status ensure_work_buffers(yk_context* ctx, WorkSet& ws, size_t paths, unsigned n_lights, unsigned n_delta_lights);
yk_status ensure_spill(yk_context* ctx, WorkSet& ws);
unsigned trace_grid(const yk_context* ctx);
PathBuffers path_buffers(WorkSet& ws, int which);
yk_status make_params(yk_context* ctx, const yk_sampler_desc* smp, const yk_integrator_desc* integ, RenderParams& prm);

struct KernelTimer {
    yk_context* ctx;
    bool on;
    std::vector<std::pair<int, int>> spans[3];  // 0 trace, 1 shadow, 2 shade
    size_t used = 0;
    int begin(hipStream_t s) {
        if (!on) return -1;
        if (used + 2 > ctx->ev_pool.size()) {
            size_t old = ctx->ev_pool.size();
            ctx->ev_pool.resize(old + 256);
            for (size_t i = old; i < ctx->ev_pool.size(); ++i) (void)hipEventCreate(&ctx->ev_pool[i]);
        }
        int a = (int)used;
        used += 2;
        (void)hipEventRecord(ctx->ev_pool[a], s);
        return a;
    }
    void end(int a, int cls, hipStream_t s) {
        if (a < 0) return;
        (void)hipEventRecord(ctx->ev_pool[a + 1], s);
        spans[cls].push_back(std::make_pair(a, a + 1));
    }
    double total(int cls) {
        double ms = 0.0;
        for (auto& sp : spans[cls]) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, ctx->ev_pool[sp.first], ctx->ev_pool[sp.second]) == hipSuccess) ms += t;
        }
        return ms * 1e-3;
    }
};

bool packet_kernel_traces_bounce(const yk_context* ctx, const yk_scene* scene, unsigned b);
// one batch of `n_paths` paths already generated into buffer 0; runs the bounce loop
void run_bounces(yk_context* ctx, WorkSet& ws, hipStream_t st, const yk_scene* scene, const RenderParams& prm, const uint32_t* pixel_xy,
                 const uint32_t* sample_index_tab, float4* sample_buf, KernelTimer& kt, unsigned long long* counters, bool coherent,
                 uint32_t n_paths, uint32_t sid_base, bool lean_camera_bounce, uint32_t* n_shadow_launches = nullptr);
