// yuki_hip.hpp — header-only C++17 mirror of the reference's interface for the Path
// hot path, over the C ABI of yuki_hip.h.  Names follow yuki's Rust types:
//
//   FilmSettings / FilmTile / film_tiles()     yuki/src/film.rs:14-65,409-475
//   CameraParameters / FoV / Camera            yuki/src/camera.rs:19-114
//   SamplerType::Uniform / ::Stratified        yuki/src/sampling/mod.rs:16-31
//   IntegratorType::{Path,Whitted,...}(params)  yuki/src/integrators/mod.rs:33-53
//   Integrator::render(scene, camera, sampler, tile, tile_pixels) -> ray count
//                                              yuki/src/integrators/mod.rs:120-185
//   Scene                                      yuki/src/scene/mod.rs:41-49
//
// Where the reference panics (assert!/unwrap) this wrapper throws yuki::Error
// carrying the yk_status.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "yuki_hip.h"

namespace yuki {

struct Error : std::runtime_error {
    yk_status status;
    Error(yk_status s, const std::string& what) : std::runtime_error(what), status(s) {}
};

inline void check(yk_status s, const yk_context* ctx = nullptr) {
    if (s == YK_OK) return;
    std::string msg = yk_status_string(s);
    if (ctx) {
        char buf[512] = {0};
        if (yk_last_error(ctx, buf, sizeof(buf)) == YK_OK && buf[0]) msg += std::string(": ") + buf;
    }
    throw Error(s, msg);
}

// film.rs:14-39
struct FilmSettings {
    uint16_t res_x = 640, res_y = 480;
    uint16_t tile_dim = 16;
    bool clear = true, accumulate = false, sixteenth_res = false;
};
// film.rs:43-65
using FilmTile = yk_tile;

// film.rs:409-475 — clipped tiles in outward-spiral order
inline std::vector<FilmTile> film_tiles(const FilmSettings& fs) {
    std::vector<FilmTile> t(yk_film_tiles(fs.res_x, fs.res_y, fs.tile_dim, nullptr, 0));
    yk_film_tiles(fs.res_x, fs.res_y, fs.tile_dim, t.data(), t.size());
    return t;
}

enum class FoV { X = 0, Y = 1 };
// camera.rs:24-41
struct CameraParameters {
    std::array<float, 3> position{0, 0, 0}, target{0, 0, 0}, up{0, 1, 0};
    FoV fov_axis = FoV::X;
    float fov_degrees = 0.0f;
};
// camera.rs:19-22,52-102
struct Camera {
    yk_camera matrices;
    Camera(const CameraParameters& p, const FilmSettings& fs) {
        yk_camera_params cp{};
        for (int k = 0; k < 3; ++k) {
            cp.position[k] = p.position[k];
            cp.target[k] = p.target[k];
            cp.up[k] = p.up[k];
        }
        cp.fov_axis = (uint32_t)p.fov_axis;
        cp.fov_degrees = p.fov_degrees;
        cp.res_x = fs.res_x;
        cp.res_y = fs.res_y;
        check(yk_camera_init(&cp, &matrices));
    }
};

// sampling/mod.rs:16-31; the seed is explicit (default: the reference's commented debug seed, uniform.rs:35)
struct SamplerType {
    static constexpr uint64_t DEBUG_SEED = 0x73B9642E74AC471CULL;
    static yk_sampler_desc Uniform(uint32_t pixel_samples, uint64_t seed = DEBUG_SEED) { return yk_sampler_desc{YK_SAMPLER_UNIFORM, pixel_samples, 1, 1, seed}; }
    static yk_sampler_desc Stratified(uint32_t nx, uint32_t ny, bool jitter_samples = true, uint64_t seed = DEBUG_SEED) {
        return yk_sampler_desc{YK_SAMPLER_STRATIFIED, nx, ny, jitter_samples ? 1u : 0u, seed};
    }
};

// integrators/path.rs:20-32
struct PathParams {
    uint32_t max_depth = 3;
    bool has_indirect_clamp = false;
    float indirect_clamp = 0.0f;
};
// integrators/whitted.rs:17-25
struct WhittedParams {
    uint32_t max_depth = 3;
};
struct IntegratorType {
    static yk_integrator_desc Whitted(const WhittedParams& p = WhittedParams()) { return yk_integrator_desc{YK_INTEGRATOR_WHITTED, p.max_depth, 0u, 0.0f}; }
    static yk_integrator_desc Path(const PathParams& p = PathParams()) { return yk_integrator_desc{YK_INTEGRATOR_PATH, p.max_depth, p.has_indirect_clamp ? 1u : 0u, p.indirect_clamp}; }
    static yk_integrator_desc BVHIntersections() { return yk_integrator_desc{YK_INTEGRATOR_BVH_INTERSECTIONS, 1, 0, 0.0f}; }
    static yk_integrator_desc GeometryNormals() { return yk_integrator_desc{YK_INTEGRATOR_GEOMETRY_NORMALS, 1, 0, 0.0f}; }
    static yk_integrator_desc ShadingNormals() { return yk_integrator_desc{YK_INTEGRATOR_SHADING_NORMALS, 1, 0, 0.0f}; }
    static yk_integrator_desc ShadingUVs() { return yk_integrator_desc{YK_INTEGRATOR_SHADING_UVS, 1, 0, 0.0f}; }
};

class Context {
   public:
    explicit Context(int device = 0) { check(yk_context_create(device, &h_)); }
    ~Context() { yk_context_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    yk_context* handle() const { return h_; }
    void set_option(const char* key, int64_t v) { check(yk_context_set_option(h_, key, v), h_); }
    // stop what the context has enqueued (any thread; yk_cancel_fn in yuki_hip.h)
    void interrupt() { check(yk_context_interrupt(h_), h_); }

   private:
    yk_context* h_ = nullptr;
};

// scene/mod.rs:41-49.  ctx == nullptr: host-only (BVH build / export, no GPU).
class Scene {
   public:
    Scene(Context* ctx, const yk_scene_desc& desc) : ctx_(ctx), n_lights_(desc.n_lights) { check(yk_scene_create(ctx ? ctx->handle() : nullptr, &desc, &h_), ctx ? ctx->handle() : nullptr); }
    // yk_scene_create_device: desc's large arrays are device pointers on ctx's device, produced on `stream` (a hipStream_t, or nullptr)
    struct FromDevice {};
    Scene(FromDevice, Context& ctx, const yk_scene_desc& desc, void* stream = nullptr) : ctx_(&ctx), n_lights_(desc.n_lights) { check(yk_scene_create_device(ctx.handle(), &desc, stream, &h_), ctx.handle()); }
    ~Scene() { yk_scene_destroy(h_); }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    yk_scene* handle() const { return h_; }
    uint32_t n_lights() const { return n_lights_; }
    yk_scene_info info() const {
        yk_scene_info i;
        check(yk_scene_get_info(h_, &i));
        return i;
    }
    yk_bvh_build_info build_info() const {  // who built the tree, and why not the device when "bvh_builder" asked for it
        yk_bvh_build_info i;
        check(yk_scene_get_build_info(h_, &i));
        return i;
    }
    yk_scene_layout_info layout_info() const {  // who laid the traversal records out ("scene_layout"), and whether the host tree is fetched
        yk_scene_layout_info i;
        check(yk_scene_get_layout_info(h_, &i));
        return i;
    }
    // yk_scene_update / yk_scene_update_device: the vertices move, the tree is refitted in place; normals may be nullptr (kept)
    void update(const float* points, const float* normals = nullptr) { check(yk_scene_update(ctx_ ? ctx_->handle() : nullptr, h_, points, normals), ctx_ ? ctx_->handle() : nullptr); }
    void update_device(const float* d_points, const float* d_normals = nullptr, void* stream = nullptr) { check(yk_scene_update_device(ctx_->handle(), h_, d_points, d_normals, stream), ctx_->handle()); }
    yk_scene_update_info update_info() const {  // the last update's route, reason and phase seconds; the plan's levels and bytes
        yk_scene_update_info i;
        check(yk_scene_get_update_info(h_, &i));
        return i;
    }
    // yk_scene_transform / yk_scene_transform_device: one matrix pair a mesh, absolute, relative to the rest pose the scene keeps
    void transform(const yk_mesh_transform* transforms) { check(yk_scene_transform(ctx_ ? ctx_->handle() : nullptr, h_, transforms), ctx_ ? ctx_->handle() : nullptr); }
    void transform_device(const void* d_transforms, void* stream = nullptr) { check(yk_scene_transform_device(ctx_->handle(), h_, d_transforms, stream), ctx_->handle()); }
    yk_scene_transform_info transform_info() const {  // the last transform's route and reason, the rest copy's bytes, the tree's cost now and at rest
        yk_scene_transform_info i;
        check(yk_scene_get_transform_info(h_, &i));
        return i;
    }
    std::vector<uint8_t> device_records(uint32_t which) const {  // test hook: one record buffer (YK_RECORDS_*) copied back
        size_t n = 0;
        check(yk_scene_read_records(h_, which, nullptr, 0, &n));
        std::vector<uint8_t> out(n);
        check(yk_scene_read_records(h_, which, out.data(), out.size(), &n));
        return out;
    }
    std::pair<std::vector<yk_bvh_node>, std::vector<uint32_t>> export_bvh() const {
        yk_scene_info i = info();
        std::vector<yk_bvh_node> nodes(i.n_nodes);
        std::vector<uint32_t> order(i.n_shapes);
        check(yk_scene_export_bvh(h_, nodes.data(), order.data()));
        return {std::move(nodes), std::move(order)};
    }
    // BoundingVolumeHierarchy::node_bounds (bvh.rs:121-157): six floats a box (p_min, p_max); -1 = every node, 0 = the root
    std::vector<float> node_bounds(int32_t target_level) const {
        std::vector<float> out(6 * yk_scene_node_bounds(h_, target_level, nullptr, 0));
        yk_scene_node_bounds(h_, target_level, out.data(), out.size() / 6);
        return out;
    }

   private:
    Context* ctx_;
    uint32_t n_lights_ = 0;
    yk_scene* h_ = nullptr;
};

// draw_visualizations (app/window.rs:1033-1063): RayVisualization and BvhVisualization drawn into a tone-mapped film.
using OverlayLine = yk_overlay_line;
// RayVisualization::set_rays (ray_visualization.rs:28-56)
inline std::vector<OverlayLine> overlay_ray_lines(const std::vector<yk_integrator_ray>& rays) {
    std::vector<OverlayLine> out(rays.size());
    check(yk_overlay_ray_lines(rays.data(), rays.size(), out.data()));
    return out;
}
// The rays of a debug sample (may be empty), then, when draw_level is set, the boxes of BVH level target_level (-1 = every level),
// under the world_to_clip of the scene's root box.  ctx == nullptr: the host instance.  film: row-major RGB, res.x * res.y * 3.
inline void draw_visualizations(Context* ctx, const Scene& scene, const yk_camera_params& camera_params, const std::vector<yk_integrator_ray>& rays,
                                bool draw_level, int32_t target_level, float* film) {
    const std::vector<float> root = scene.node_bounds(0);
    float m[16];
    check(yk_overlay_world_to_clip(&camera_params, root.data(), m));
    const std::vector<OverlayLine> lines = overlay_ray_lines(rays);
    const std::vector<float> boxes = draw_level ? scene.node_bounds(target_level) : std::vector<float>();
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_overlay_draw(c, m, lines.empty() ? nullptr : lines.data(), lines.size(), boxes.empty() ? nullptr : boxes.data(), boxes.size() / 6, film,
                          camera_params.res_x, camera_params.res_y), c);
}

// scene::pbrt::load / Scene::ply / scene::mitsuba::load (scene/pbrt/mod.rs:94, scene/mod.rs:99, scene/mitsuba/mod.rs:28): the parsed scene as a
// ready yk_scene_desc plus the CameraParameters and FilmSettings the reference's loaders return
class LoadedScene {
   public:
    enum class Format { Ply, Pbrt, Mitsuba, ByExtension };  // ByExtension: try_load_scene, app/util.rs:15-63
    LoadedScene(const std::string& path, Format format, uint32_t split_method = YK_SPLIT_SAH, uint32_t max_shapes_in_node = 1) {
        auto load = format == Format::Ply ? yk_load_ply : (format == Format::Pbrt ? yk_load_pbrt : (format == Format::Mitsuba ? yk_load_mitsuba : yk_load_scene));
        yk_status st = load(path.c_str(), split_method, max_shapes_in_node, &h_);
        if (st != YK_OK) throw Error(st, yk_loader_last_error());
        uint16_t tile_dim = 16;
        yk_camera_params cp;
        check(yk_loaded_scene_get(h_, &desc, &cp, &tile_dim));
        camera.position = {cp.position[0], cp.position[1], cp.position[2]};
        camera.target = {cp.target[0], cp.target[1], cp.target[2]};
        camera.up = {cp.up[0], cp.up[1], cp.up[2]};
        camera.fov_axis = cp.fov_axis == 0 ? FoV::X : FoV::Y;
        camera.fov_degrees = cp.fov_degrees;
        film.res_x = cp.res_x;
        film.res_y = cp.res_y;
        film.tile_dim = tile_dim;
    }
    ~LoadedScene() { yk_loaded_scene_destroy(h_); }
    LoadedScene(const LoadedScene&) = delete;
    LoadedScene& operator=(const LoadedScene&) = delete;
    yk_scene_desc desc{};  // valid while this object lives; pass to Scene(ctx, desc)
    CameraParameters camera;
    FilmSettings film;

   private:
    yk_loaded_scene* h_ = nullptr;
};

// app/util.rs:90-111
inline void write_exr(const std::string& path, uint32_t width, uint32_t height, const float* rgb) { check(yk_write_exr(path.c_str(), width, height, rgb)); }

// ScaleOutput::draw (app/renderpasses/scale_output.rs), the last pass of a frame: the rule is stated in yuki_hip.h.
inline yk_present_rect present_target_rect(uint16_t res_x, uint16_t res_y, uint16_t window_x, uint16_t window_y) {
    yk_present_rect r;
    check(yk_present_target_rect(res_x, res_y, window_x, window_y, &r));
    return r;
}
// The tone-mapped film (row-major RGB, res_x * res_y * 3) as the window's RGBA8 frame, rows top-down: window_x * window_y * 4
// bytes.  ctx == nullptr: the host instance.  encode: the reference's default is the sRGB back buffer.
inline std::vector<uint8_t> present_rgba8(Context* ctx, const float* film, uint16_t res_x, uint16_t res_y, uint16_t window_x, uint16_t window_y,
                                          uint32_t encode = YK_PRESENT_ENCODE_SRGB) {
    const yk_present_desc d = {window_x, window_y, encode, YK_PRESENT_RGBA8};
    std::vector<uint8_t> out((size_t)window_x * window_y * 4);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_present(c, &d, film, res_x, res_y, out.data()), c);
    return out;
}
// The same on device buffers, enqueued on `stream` (nullptr: the context's): one kernel, no allocation, no synchronisation.
inline void present_device(Context& ctx, const yk_present_desc& desc, const void* d_film, uint16_t res_x, uint16_t res_y, void* d_out, void* stream = nullptr) {
    check(yk_present_device(ctx.handle(), &desc, d_film, res_x, res_y, d_out, stream), ctx.handle());
}
// 8-bit PNG, channels 3 or 4, row 0 at the top
inline void write_png(const std::string& path, uint32_t width, uint32_t height, uint32_t channels, const uint8_t* pixels) {
    check(yk_write_png(path.c_str(), width, height, channels, pixels));
}

// Guides through glass (the rule is stated in yuki_hip.h and csrc/yk_guides_through.h): the guide and the surface id of the
// surface every pixel shows and the number of glass interfaces crossed on the way, res_x * res_y records each, row-major.
struct GuidesThrough {
    std::vector<yk_guide> guides;
    std::vector<yk_surface_id> ids;
    std::vector<uint32_t> through;
};
inline GuidesThrough render_guides_through(Context& ctx, const Scene& scene, const yk_camera& camera, uint16_t res_x, uint16_t res_y, uint32_t max_through = 4) {
    GuidesThrough g;
    const size_t n = (size_t)res_x * res_y;
    g.guides.resize(n);
    g.ids.resize(n);
    g.through.resize(n);
    check(yk_render_guides_through(ctx.handle(), scene.handle(), &camera, res_x, res_y, max_through, g.guides.data(), g.ids.data(), g.through.data()), ctx.handle());
    return g;
}
// The same into device buffers (any of the three may be nullptr, not all), ordered on `stream`; no read-back, no allocation.
inline void render_guides_through_device(Context& ctx, const Scene& scene, const yk_camera& camera, uint16_t res_x, uint16_t res_y, uint32_t max_through, void* d_guides,
                                         void* d_ids, void* d_through, void* stream = nullptr) {
    check(yk_render_guides_through_device(ctx.handle(), scene.handle(), &camera, res_x, res_y, max_through, d_guides, d_ids, d_through, stream), ctx.handle());
}

// Textures under the denoiser (the library's own passes; the rule is stated in yuki_hip.h and csrc/yk_albedo.h).
using Albedo = yk_albedo;
// The first-hit albedo of every pixel from yk_render_guides_ids' ids (res_x * res_y records, row-major).  ctx == nullptr: the
// host instance.
inline std::vector<Albedo> surface_albedo(Context* ctx, const Scene& scene, const yk_surface_id* ids, uint16_t res_x, uint16_t res_y) {
    std::vector<Albedo> out((size_t)res_x * res_y);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_surface_albedo(c, scene.handle(), ids, res_x, res_y, out.data()), c);
    return out;
}
// The same on device buffers, enqueued on `stream` (nullptr: the context's): one kernel, no allocation, no synchronisation.
inline void surface_albedo_device(Context& ctx, const Scene& scene, const void* d_ids, uint16_t res_x, uint16_t res_y, void* d_out, void* stream = nullptr) {
    check(yk_surface_albedo_device(ctx.handle(), scene.handle(), d_ids, res_x, res_y, d_out, stream), ctx.handle());
}
// The pixel-mean albedo: the mean of the first-hit albedo over the s x s block of the (s*res_x) x (s*res_y) film's ids under
// every output pixel (res_x * res_y records).  ctx == nullptr: the host instance.
inline std::vector<Albedo> albedo_mean(Context* ctx, const Scene& scene, const yk_surface_id* ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s) {
    std::vector<Albedo> out((size_t)res_x * res_y);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_albedo_mean(c, scene.handle(), ids_ss, res_x, res_y, s, out.data()), c);
    return out;
}
// The same on device buffers, enqueued on `stream` (nullptr: the context's): one kernel, no allocation, no synchronisation.
inline void albedo_mean_device(Context& ctx, const Scene& scene, const void* d_ids_ss, uint16_t res_x, uint16_t res_y, uint32_t s, void* d_out, void* stream = nullptr) {
    check(yk_albedo_mean_device(ctx.handle(), scene.handle(), d_ids_ss, res_x, res_y, s, d_out, stream), ctx.handle());
}
// The fused route: the large film traced in bands under `camera_ss` (the camera of (s*res_x, s*res_y)) and reduced, never whole.
inline void render_albedo_mean_device(Context& ctx, const Scene& scene, const yk_camera& camera_ss, uint16_t res_x, uint16_t res_y, uint32_t s, void* d_out,
                                      void* stream = nullptr) {
    check(yk_render_albedo_mean_device(ctx.handle(), scene.handle(), &camera_ss, res_x, res_y, s, d_out, stream), ctx.handle());
}
// yk_denoise on radiance / albedo: the film (row-major RGB; `samples` = Film.samples or nullptr) -> the denoised film.
inline std::vector<float> denoise_albedo(Context* ctx, const yk_denoise_desc& desc, const float* film, const yk_guide* guides, const Albedo* albedo, uint16_t res_x,
                                         uint16_t res_y, uint16_t tile_dim, const uint32_t* samples = nullptr) {
    std::vector<float> out((size_t)res_x * res_y * 3);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_denoise_albedo(c, &desc, film, guides, albedo, res_x, res_y, tile_dim, samples, out.data()), c);
    return out;
}
// The same on device buffers (d_out may be d_film), enqueued on `stream`: a preparing launch and one launch per iteration.
inline void denoise_albedo_device(Context& ctx, const yk_denoise_desc& desc, const void* d_film, const void* d_guides, const void* d_albedo, uint16_t res_x,
                                  uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out, void* stream = nullptr) {
    check(yk_denoise_albedo_device(ctx.handle(), &desc, d_film, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out, stream), ctx.handle());
}

// Variance-guided denoise (the library's own passes; the rule is stated in yuki_hip.h and csrc/yk_variance.h).
using Moments = yk_moments;
// The film yk_history_blend folds into the history, folded into the moments (nullptr: none yet).  ctx == nullptr: the host
// instance.  A moments buffer is reprojected by yk_history_reproject[_moved] cast to yk_history.
inline std::vector<Moments> moments_blend(Context* ctx, const yk_temporal_desc& desc, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                          const Moments* moments) {
    std::vector<Moments> out((size_t)res_x * res_y);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_moments_blend(c, &desc, film, res_x, res_y, tile_dim, samples, moments, out.data()), c);
    return out;
}
inline void moments_blend_device(Context& ctx, const yk_temporal_desc& desc, const void* d_film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                 const void* d_moments, void* d_out_moments, void* stream = nullptr) {
    check(yk_moments_blend_device(ctx.handle(), &desc, d_film, res_x, res_y, tile_dim, samples, d_moments, d_out_moments, stream), ctx.handle());
}
// History rectification, before history_blend / moments_blend on every frame (the rule is stated in yuki_hip.h and
// csrc/yk_rectify.h): the carried history clipped to the box of the current film around each pixel -> (history, moments);
// moments may be nullptr, the second vector is then empty.  ctx == nullptr: the host instance.
inline std::pair<std::vector<yk_history>, std::vector<Moments>> history_rectify(Context* ctx, const yk_rectify_desc& desc, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                                                                                const uint32_t* samples, const yk_history* history, const Moments* moments = nullptr) {
    std::vector<yk_history> out((size_t)res_x * res_y);
    std::vector<Moments> out_m(moments ? (size_t)res_x * res_y : 0);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_history_rectify(c, &desc, film, res_x, res_y, tile_dim, samples, history, moments, out.data(), moments ? out_m.data() : nullptr), c);
    return {std::move(out), std::move(out_m)};
}
// The same on device buffers (each output may be its own input; the moments both or neither), enqueued on `stream`: one launch.
inline void history_rectify_device(Context& ctx, const yk_rectify_desc& desc, const void* d_film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                   const void* d_history, const void* d_moments, void* d_out_history, void* d_out_moments, void* stream = nullptr) {
    check(yk_history_rectify_device(ctx.handle(), &desc, d_film, res_x, res_y, tile_dim, samples, d_history, d_moments, d_out_history, d_out_moments, stream), ctx.handle());
}
// Despeckle, first in a frame on the current frame's film, before history_rectify (the rule is stated in yuki_hip.h and
// csrc/yk_despeckle.h): a pixel far brighter than its neighbourhood is scaled down to gain x the rank-th largest luminance
// around it -> the film, in the input's convention.  mask (res_x * res_y bytes: 0 untouched, 1 clamped, 2 repaired) and
// counts (two words: clamped, repaired) may be nullptr.  ctx == nullptr: the host instance.
inline std::vector<float> despeckle(Context* ctx, const yk_despeckle_desc& desc, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples = nullptr,
                                    uint8_t* mask = nullptr, uint32_t* counts = nullptr) {
    std::vector<float> out((size_t)res_x * res_y * 3);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_despeckle(c, &desc, film, res_x, res_y, tile_dim, samples, out.data(), mask, counts), c);
    return out;
}
// The same on device buffers (the output is another buffer: the pass does not run in place), enqueued on `stream`: one launch.
inline void despeckle_device(Context& ctx, const yk_despeckle_desc& desc, const void* d_film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb,
                             void* d_out_mask = nullptr, void* d_out_counts = nullptr, void* stream = nullptr) {
    check(yk_despeckle_device(ctx.handle(), &desc, d_film, res_x, res_y, tile_dim, samples, d_out_rgb, d_out_mask, d_out_counts, stream), ctx.handle());
}
// The variance of the luminance of `film` as denoise_variance will filter it; moments and albedo may be nullptr.
inline std::vector<float> variance(Context* ctx, const yk_variance_desc& desc, const Moments* moments, const float* film, const yk_guide* guides, const Albedo* albedo, uint16_t res_x,
                                   uint16_t res_y, uint16_t tile_dim, const uint32_t* samples = nullptr) {
    std::vector<float> out((size_t)res_x * res_y);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_variance(c, &desc, moments, film, guides, albedo, res_x, res_y, tile_dim, samples, out.data()), c);
    return out;
}
inline void variance_device(Context& ctx, const yk_variance_desc& desc, const void* d_moments, const void* d_film, const void* d_guides, const void* d_albedo, uint16_t res_x,
                            uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_variance, void* stream = nullptr) {
    check(yk_variance_device(ctx.handle(), &desc, d_moments, d_film, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out_variance, stream), ctx.handle());
}
// yk_denoise with a colour stop that follows the variance image; albedo may be nullptr.
inline std::vector<float> denoise_variance(Context* ctx, const yk_variance_desc& desc, const float* film, const yk_guide* guides, const float* variance, const Albedo* albedo,
                                           uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples = nullptr) {
    std::vector<float> out((size_t)res_x * res_y * 3);
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_denoise_variance(c, &desc, film, guides, variance, albedo, res_x, res_y, tile_dim, samples, out.data()), c);
    return out;
}
// The same on device buffers (d_out may be d_film), enqueued on `stream`: a preparing launch and one launch per iteration.
inline void denoise_variance_device(Context& ctx, const yk_variance_desc& desc, const void* d_film, const void* d_guides, const void* d_variance, const void* d_albedo, uint16_t res_x,
                                    uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out, void* stream = nullptr) {
    check(yk_denoise_variance_device(ctx.handle(), &desc, d_film, d_guides, d_variance, d_albedo, res_x, res_y, tile_dim, samples, d_out, stream), ctx.handle());
}

// Adaptive sampling (the library's own passes; the rule is stated in yuki_hip.h and csrc/yk_adaptive.h): a film of RGB sums
// with one yk_pixel_stats a pixel, both zeros when cleared.  ctx == nullptr: the host instance.
using PixelStats = yk_pixel_stats;
// The selected pixels in the rule's order: (x | y << 16, the pixel's next sample index).
inline std::pair<std::vector<uint32_t>, std::vector<uint32_t>> adaptive_select(Context* ctx, const yk_adaptive_desc& desc, const PixelStats* stats, uint16_t res_x, uint16_t res_y) {
    std::vector<uint32_t> xy((size_t)res_x * res_y), sample((size_t)res_x * res_y);
    uint32_t n = 0;
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_adaptive_select(c, &desc, stats, res_x, res_y, xy.data(), sample.data(), &n), c);
    xy.resize(n);
    sample.resize(n);
    return {std::move(xy), std::move(sample)};
}
// passes: n_passes x xy.size() x RGB, pass-major; folded into film_sum and stats in place.
inline void adaptive_accumulate(Context* ctx, const std::vector<uint32_t>& xy, const float* passes, uint32_t n_passes, uint16_t res_x, uint16_t res_y, float* film_sum, PixelStats* stats) {
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_adaptive_accumulate(c, xy.data(), (uint32_t)xy.size(), passes, n_passes, res_x, res_y, film_sum, stats), c);
}
// The mean film and the variance of that mean (what denoise_variance takes); either output may be nullptr.
inline void adaptive_resolve(Context* ctx, const float* film_sum, const PixelStats* stats, uint16_t res_x, uint16_t res_y, float* out_rgb, float* out_variance) {
    yk_context* c = ctx ? ctx->handle() : nullptr;
    check(yk_adaptive_resolve(c, film_sum, stats, res_x, res_y, out_rgb, out_variance), c);
}
inline void adaptive_resolve_device(Context& ctx, const void* d_film_sum, const void* d_stats, uint16_t res_x, uint16_t res_y, void* d_out_rgb, void* d_out_variance, void* stream = nullptr) {
    check(yk_adaptive_resolve_device(ctx.handle(), d_film_sum, d_stats, res_x, res_y, d_out_rgb, d_out_variance, stream), ctx.handle());
}

// trait Integrator, integrators/mod.rs:92-186
class Integrator {
   public:
    Integrator(Context& ctx, yk_integrator_desc desc) : ctx_(ctx), desc_(desc) {}
    // Rounds of select -> render the selected pixels -> fold into the device film sums and statistics, until nothing is
    // selected (or desc.max_rounds); continues from what the buffers hold.  Synchronous.
    yk_adaptive_info render_adaptive_device(const Scene& scene, const Camera& camera, const yk_sampler_desc& sampler, const yk_adaptive_desc& desc, uint16_t res_x, uint16_t res_y,
                                            void* d_film_sum, void* d_stats, void* stream = nullptr, yk_cancel_fn cancel = nullptr, void* user = nullptr) const {
        yk_adaptive_info info{};
        check(yk_render_adaptive_device(ctx_.handle(), scene.handle(), &camera.matrices, &sampler, &desc_, &desc, res_x, res_y, d_film_sum, d_stats, stream, &info, cancel, user),
              ctx_.handle());
        return info;
    }
    // render(): one tile; tile_pixels holds >= tile area RGB triples; returns the ray count
    size_t render(const Scene& scene, const Camera& camera, const yk_sampler_desc& sampler, const FilmTile& tile, float* tile_pixels) const {
        uint64_t rays = 0;
        check(yk_render_tile(ctx_.handle(), scene.handle(), &camera.matrices, &sampler, &desc_, &tile, tile_pixels, &rays), ctx_.handle());
        return (size_t)rays;
    }
    // all tiles of a GPU worker in one submission; out_rgb tile-major
    yk_render_stats render_tiles(const Scene& scene, const Camera& camera, const yk_sampler_desc& sampler, const std::vector<FilmTile>& tiles, float* out_rgb,
                                 yk_cancel_fn cancel = nullptr, void* user = nullptr) const {
        yk_render_stats st{};
        check(yk_render_tiles(ctx_.handle(), scene.handle(), &camera.matrices, &sampler, &desc_, tiles.data(), tiles.size(), out_rgb, &st, cancel, user), ctx_.handle());
        return st;
    }

    // Integrator::render(accumulating = true): one sample (global index tile_samples[t]) per pixel, raw value;
    // n_passes > 1 renders samples tile_samples[t] .. + n_passes - 1 at once (out_rgb: n_passes x pixels x RGB, pass-major)
    yk_render_stats render_tiles_accumulating(const Scene& scene, const Camera& camera, const yk_sampler_desc& sampler, const std::vector<FilmTile>& tiles,
                                              const std::vector<uint16_t>& tile_samples, float* out_rgb, uint32_t n_passes = 1) const {
        if (tile_samples.size() != tiles.size()) throw Error(YK_ERR_INVALID_ARGUMENT, "one sample index per tile");
        yk_render_stats st{};
        check(yk_render_tiles_accumulating_passes(ctx_.handle(), scene.handle(), &camera.matrices, &sampler, &desc_, tiles.data(), tile_samples.data(), tiles.size(), n_passes,
                                                  out_rgb, &st, nullptr, nullptr),
              ctx_.handle());
        return st;
    }

    // Integrator::li_debug (integrators/mod.rs:103-115), Path only: per sample the radiance, the closest-hit ray count and its
    // rays in the reference's push order; the sampler is started at (pixel_xy[i], sample_index[i]) after `dimension` draws
    struct LiDebug {
        std::vector<float> li;  // n x RGB
        std::vector<uint32_t> ray_counts;
        std::vector<std::vector<yk_integrator_ray>> rays;
    };
    LiDebug li_debug(const Scene& scene, const yk_sampler_desc& sampler, size_t n, const float* ray_o, const float* ray_d, const uint16_t* pixel_xy,
                     const uint32_t* sample_index, uint32_t dimension = 2) const {
        const uint32_t cap = desc_.max_depth * (2u + scene.n_lights());  // always suffices
        LiDebug r;
        r.li.resize(3 * n);
        r.ray_counts.resize(n);
        std::vector<yk_integrator_ray> recs((size_t)n * cap);
        std::vector<uint32_t> n_rays(n);
        check(yk_li_debug(ctx_.handle(), scene.handle(), &sampler, &desc_, n, ray_o, ray_d, pixel_xy, sample_index, dimension, cap, r.li.data(),
                          r.ray_counts.data(), recs.data(), n_rays.data()),
              ctx_.handle());
        r.rays.resize(n);
        for (size_t i = 0; i < n; ++i) r.rays[i].assign(recs.begin() + i * cap, recs.begin() + i * cap + n_rays[i]);
        return r;
    }

   private:
    Context& ctx_;
    yk_integrator_desc desc_;
};

// The render workers' shared door to the device (render_manager.rs:78-97: num_cpus - 1 threads, each calling Integrator::render for
// one tile): calls that wait at the same time share a submission on one of the lanes' contexts (yk_combiner in yuki_hip.h).
class Combiner {
   public:
    explicit Combiner(const std::vector<Context*>& lanes, uint32_t max_tiles = 0, uint32_t linger_us = 100) {
        std::vector<yk_context*> h;
        for (Context* c : lanes) h.push_back(c->handle());
        check(yk_combiner_create(h.data(), (uint32_t)h.size(), max_tiles, linger_us, &c_));
    }
    ~Combiner() { yk_combiner_destroy(c_); }
    Combiner(const Combiner&) = delete;
    Combiner& operator=(const Combiner&) = delete;
    // Integrator::render for one FilmTile from a worker thread; accumulating_sample < 0: all samples of the pixel, the mean stored.
    // Returns the ray count (the submission's, shared out by tile area: exact in sum).  Throws Error(YK_ERR_CANCELLED) when the
    // caller's own predicate fired.
    size_t render(const Scene& scene, const Camera& camera, const yk_sampler_desc& sampler, const yk_integrator_desc& integrator, const FilmTile& tile,
                  float* tile_pixels, int32_t accumulating_sample = -1, yk_cancel_fn cancel = nullptr, void* user = nullptr) {
        yk_render_stats st{};
        const yk_status rc = yk_combiner_render_tile(c_, scene.handle(), &camera.matrices, &sampler, &integrator, &tile, accumulating_sample, tile_pixels, &st, cancel, user);
        if (rc != YK_OK) {
            char buf[512] = {0};
            yk_combiner_last_error(c_, buf, sizeof buf);
            throw Error(rc, buf);
        }
        return (size_t)st.rays;
    }
    yk_combiner_info info() const {
        yk_combiner_info i{};
        check(yk_combiner_get_info(c_, &i));
        return i;
    }

   private:
    yk_combiner* c_ = nullptr;
};

// All GPUs of the process behind one object — RenderManager's role for GPU workers
// (renderer/render_manager.rs:78-97: one worker per device; :206-210: interleaved tiles;
// film.rs:210-282: the write-back).  devices[0] assembles the film.
class Node {
   public:
    // flags: YK_MULTI_SHARED_DEVICES (ranks may name the same device: G ranks on one GPU), YK_MULTI_PEER_COPY (hipMemcpyPeerAsync instead of RCCL)
    explicit Node(const std::vector<int>& devices, uint32_t flags = 0) { check(yk_multi_create_ex(devices.data(), (uint32_t)devices.size(), flags, &m_)); }
    // the tiles of rank `rank` among `n_ranks` (render_manager.rs:206-210: spiral tile i -> rank i mod n_ranks); needs no device
    static std::vector<yk_tile> deal(const FilmSettings& fs, uint32_t n_ranks, uint32_t rank, uint64_t* pixels = nullptr) {
        std::vector<yk_tile> t(yk_multi_deal(fs.res_x, fs.res_y, fs.tile_dim, n_ranks, rank, nullptr, 0, nullptr));
        yk_multi_deal(fs.res_x, fs.res_y, fs.tile_dim, n_ranks, rank, t.data(), t.size(), pixels);
        return t;
    }
    ~Node() {
        if (film_) yk_multi_film_destroy(film_);
        if (scene_) yk_multi_scene_destroy(scene_);
        if (m_) yk_multi_destroy(m_);
    }
    Node(const Node&) = delete;
    Node& operator=(const Node&) = delete;
    uint32_t device_count() const { return yk_multi_device_count(m_); }
    void set_option(const char* key, int64_t value) { mcheck(yk_multi_set_option(m_, key, value)); }
    // BoundingVolumeHierarchy::new once, one copy per device
    void set_scene(const yk_scene_desc& d) {
        if (scene_) yk_multi_scene_destroy(scene_);
        scene_ = nullptr;
        mcheck(yk_multi_scene_create(m_, &d, &scene_));
    }
    void set_film(const FilmSettings& fs) {
        if (film_) yk_multi_film_destroy(film_);
        film_ = nullptr;
        fs_ = fs;
        mcheck(yk_multi_film_create(m_, fs.res_x, fs.res_y, fs.tile_dim, &film_));
    }
    // every tile of the film on its device, the exchange, Film::update_tile: row-major RGB, res_x * res_y * 3 floats
    yk_render_stats render_film(const Camera& camera, const yk_sampler_desc& sampler, const yk_integrator_desc& integrator, float* film_rgb, yk_cancel_fn cancel = nullptr,
                                void* user = nullptr) {
        yk_render_stats st{};
        mcheck(yk_multi_render_film(m_, scene_, &camera.matrices, &sampler, &integrator, film_, film_rgb, &st, cancel, user));
        return st;
    }
    // the accumulating film over all devices (film.rs:260-272): passes first_sample .. + n_passes - 1 of every tile, added on device 0
    void clear_film() { mcheck(yk_multi_film_clear(m_, film_)); }
    yk_render_stats accumulate_film(const Camera& camera, const yk_sampler_desc& sampler, const yk_integrator_desc& integrator, uint32_t first_sample, uint32_t n_passes,
                                    float* film_rgb, yk_cancel_fn cancel = nullptr, void* user = nullptr) {
        yk_render_stats st{};
        mcheck(yk_multi_accumulate_film(m_, scene_, &camera.matrices, &sampler, &integrator, film_, first_sample, n_passes, film_rgb, &st, cancel, user));
        return st;
    }

   private:
    void mcheck(yk_status s) const {
        if (s == YK_OK) return;
        char buf[512] = {0};
        yk_multi_last_error(m_, buf, sizeof(buf));
        throw Error(s, std::string(yk_status_string(s)) + (buf[0] ? std::string(": ") + buf : std::string()));
    }
    yk_multi* m_ = nullptr;
    yk_multi_scene* scene_ = nullptr;
    yk_multi_film* film_ = nullptr;
    FilmSettings fs_;
};

}  // namespace yuki
