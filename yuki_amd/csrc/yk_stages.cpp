// yk_stages.cpp — the per-stage entry points of the C ABI: the device functions the kernels call, one stage at a
// time, for the stage-level parity tests (tests/test_gpu_stages.py) and profiling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "yk_film_call.h"
#include "yk_internal.h"
#include "yk_staging.h"

// "trace_stage_kernel" (yk_context_set_option): the kernels the two traversal stages launch.
//   0  k_trace_closest_pt / k_trace_any_pt, API flavour (source shape, t, barycentrics; vis = 0 / 1)
//   1  the same kernels as the render loop launches them: the closest-hit kernel reports the leaf-order hit word
//      (slot | BSDF kind bits), the any-hit kernel scatters its verdicts through a slot_of map (vis[slot] = 2)
//   2  the wave-packet kernels of yk_packet.hip, on the render's grid; the caller's ray order decides the packets
// A mode never falls back to another kernel: an argument it cannot honour is refused.
static yk_status check_stage_kernel(yk_context* ctx, const yk_scene* scene, bool closest, const float* t_max, bool wants_extras) {
    const int64_t mode = ctx->trace_stage_kernel;
    if (mode == 0) return YK_OK;
    if (wants_extras) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "trace_stage_kernel " + std::to_string(mode) + " reports shape ids only (no t, barycentrics or counters)");
    if (closest && t_max)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, mode == 1 ? "trace_stage_kernel 1: the render-loop closest-hit kernel takes no t_max"
                                                            : "trace_stage_kernel 2: the packet closest-hit kernel starts at t_max = inf");
    if (mode == 2 && scene->bvh->depth > 64) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "trace_stage_kernel 2: the packet kernels need a tree depth <= 64");
    return YK_OK;
}

// the grid run_bounces gives the packet kernels (yk_render.cpp)
static unsigned packet_grid(const yk_context* ctx) { return (unsigned)ctx->n_cu * packet_blocks_per_cu(); }

// slot_of of the stage's any-hit modes 1 and 2: reversed, so that a verdict written to its ray's own index shows
static const unsigned* upload_reversed_slots(Staging& sg, size_t n) {
    std::vector<uint32_t> slots(n);
    for (size_t k = 0; k < n; ++k) slots[k] = (uint32_t)(n - 1 - k);
    const unsigned* d_slots = sg.upload(slots.data(), n);
    if (sg.ok()) sg.check(hipStreamSynchronize(sg.stream));  // `slots` goes out of scope
    return d_slots;
}

extern "C" {

// ------------------------------------------------------------------ per-stage entry points
yk_status yk_trace_closest(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d, const float* t_max,
                           int32_t* out_shape, float* out_t, float* out_bary, uint32_t* out_node_tests, uint32_t* out_node_hits,
                           uint32_t* out_shape_tests) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !ray_o || !ray_d || !out_shape || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (yk_status rs = scene_on_context(ctx, scene, "")) return rs;
    if (n > 0xFFFFFF00ull) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "too many rays");
    const bool want_stats = out_node_tests || out_node_hits || out_shape_tests;
    yk_status wb = check_stage_kernel(ctx, scene, true, t_max, out_t || out_bary || want_stats);
    if (wb != YK_OK) return wb;
    const int64_t mode = ctx->trace_stage_kernel;
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    if ((wb = ensure_work_buffers(ctx, ctx->ws[0], n, scene->n_lights, scene->n_delta_lights)) != YK_OK) return wb;
    if ((wb = ensure_spill(ctx, ctx->ws[0])) != YK_OK) return wb;
    HIP_TRY(ctx, ctx->hit4.ensure(n * 16));
    if (want_stats) HIP_TRY(ctx, ctx->stats4.ensure(n * 16));
    const float* d_o = sg.upload(ray_o, n * 3);
    const float* d_d = sg.upload(ray_d, n * 3);
    const float* d_t_max = t_max ? sg.upload(t_max, n) : nullptr;
    if (!sg.ok()) return sg.status();
    PathBuffers pb = path_buffers(ctx->ws[0], 0);
    launch_pack_rays(st, n, d_o, d_d, pb.rayO, pb.rayD);
    unsigned* ctrl = ctx->ws[0].ctrl.as<unsigned>();
    HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, YK_CTRL_WORDS * 4, st));
    unsigned nn = (unsigned)n;
    HIP_TRY(ctx, hipMemcpyAsync(ctrl, &nn, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (mode == 0)
        launch_trace_closest(st, trace_grid(ctx), dev_scene_for(scene, n), pb.rayO, pb.rayD, d_t_max, ctrl, ctrl + YK_CTRL_HEADS,
                             ctx->ws[0].hit.as<int>(), ctx->hit4.as<float4>(), want_stats ? ctx->stats4.as<uint4>() : nullptr, ctx->ws[0].spill.as<uint2>(),
                             trace_grid(ctx) * trace_block_size(), ctrl, nullptr);
    else if (mode == 1)  // no t_max, no hit_out: the render loop's flavour (launch_trace_closest picks it from these two)
        launch_trace_closest(st, trace_grid(ctx), dev_scene_for(scene, n), pb.rayO, pb.rayD, nullptr, ctrl, ctrl + YK_CTRL_HEADS, ctx->ws[0].hit.as<int>(), nullptr,
                             nullptr, ctx->ws[0].spill.as<uint2>(), trace_grid(ctx) * trace_block_size(), ctrl, nullptr);
    else
        launch_trace_closest_packet(st, packet_grid(ctx), dev_scene_for(scene, n), pb.rayO, pb.rayD, ctrl, ctrl + YK_CTRL_HEADS, ctx->ws[0].hit.as<int>(), nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_shape, ctx->ws[0].hit.p, n * 4, hipMemcpyDeviceToHost, st));
    std::vector<float> h4;
    if (out_t || out_bary) {
        h4.resize(n * 4);
        HIP_TRY(ctx, hipMemcpyAsync(h4.data(), ctx->hit4.p, n * 16, hipMemcpyDeviceToHost, st));
    }
    std::vector<uint32_t> s4;
    if (want_stats) {
        s4.resize(n * 4);
        HIP_TRY(ctx, hipMemcpyAsync(s4.data(), ctx->stats4.p, n * 16, hipMemcpyDeviceToHost, st));
    }
    unsigned host_ctrl[4];
    HIP_TRY(ctx, hipMemcpyAsync(host_ctrl, ctrl, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (mode != 0) {  // hit word -> source shape (the scene's leaf-order table); its kind bits must be the shape's material's
        const HostBvh* tree = scene_host_tree(scene);
        if (!tree) return fail(ctx, YK_ERR_DEVICE, "the scene's shape order could not be copied back from the device");
        const std::vector<uint32_t>& order = tree->shape_order;
        const std::vector<uint8_t>* kinds = scene_shape_kind(scene);
        if (!kinds) return fail(ctx, YK_ERR_DEVICE, "the scene's triangle materials could not be copied back from the device");
        for (size_t i = 0; i < n; ++i) {
            const int32_t h = out_shape[i];
            if (h == -1) continue;
            const uint32_t prim = (uint32_t)h & YK_HIT_PRIM_MASK, kind = ((uint32_t)h >> YK_HIT_KIND_SHIFT) & 7u;
            if (h < 0 || prim >= order.size())
                return fail(ctx, YK_ERR_DEVICE, "trace_stage_kernel " + std::to_string(mode) + ": ray " + std::to_string(i) + " got hit word " + std::to_string(h));
            const uint32_t src = order[prim];
            if (kind != (*kinds)[src])
                return fail(ctx, YK_ERR_DEVICE, "trace_stage_kernel " + std::to_string(mode) + ": ray " + std::to_string(i) + " hit shape " + std::to_string(src) +
                                                     " with kind bits " + std::to_string(kind) + ", its material's kind is " + std::to_string((*kinds)[src]));
            out_shape[i] = (int32_t)src;
        }
    }
    for (size_t i = 0; i < n; ++i) {
        if (out_t) out_t[i] = out_shape[i] >= 0 ? h4[4 * i] : __builtin_inff();
        if (out_bary) {
            out_bary[3 * i] = out_shape[i] >= 0 ? h4[4 * i + 1] : 0.0f;
            out_bary[3 * i + 1] = out_shape[i] >= 0 ? h4[4 * i + 2] : 0.0f;
            out_bary[3 * i + 2] = out_shape[i] >= 0 ? h4[4 * i + 3] : 0.0f;
        }
        if (out_node_tests) out_node_tests[i] = s4[4 * i];
        if (out_node_hits) out_node_hits[i] = s4[4 * i + 1];
        if (out_shape_tests) out_shape_tests[i] = s4[4 * i + 2];
    }
    if (host_ctrl[YK_CTRL_ERR] & 1u) return fail(ctx, YK_ERR_STACK_OVERFLOW, "BVH traversal stack exceeded 64 entries (bvh.rs:174)");
    return YK_OK;
} YK_CATCH(ctx)

yk_status yk_surface(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d, int32_t route, float* out) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !ray_o || !ray_d || !out || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (route != 0 && route != 1) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "route: 0 = by leaf-order slot (hit_surface_prim), 1 = by source shape (hit_surface)");
    if (yk_status rs = scene_on_context(ctx, scene, "")) return rs;
    if (n > 0xFFFFFF00ull / YK_SURFACE_FLOATS) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "too many rays");
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    yk_status wb;
    if ((wb = ensure_work_buffers(ctx, ctx->ws[0], n, scene->n_lights, scene->n_delta_lights)) != YK_OK) return wb;
    if ((wb = ensure_spill(ctx, ctx->ws[0])) != YK_OK) return wb;
    const float* d_o = sg.upload(ray_o, n * 3);
    const float* d_d = sg.upload(ray_d, n * 3);
    float* d_out = sg.output(out, n * YK_SURFACE_FLOATS);
    if (!sg.ok()) return sg.status();
    PathBuffers pb = path_buffers(ctx->ws[0], 0);
    launch_pack_rays(st, n, d_o, d_d, pb.rayO, pb.rayD);
    unsigned* ctrl = ctx->ws[0].ctrl.as<unsigned>();
    HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, YK_CTRL_WORDS * 4, st));
    unsigned nn = (unsigned)n;
    HIP_TRY(ctx, hipMemcpyAsync(ctrl, &nn, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // the closest-hit kernel as the render loop launches it (no t_max, no hit_out): hit word = leaf-order slot | kind bits
    launch_trace_closest(st, trace_grid(ctx), dev_scene_for(scene, n), pb.rayO, pb.rayD, nullptr, ctrl, ctrl + YK_CTRL_HEADS, ctx->ws[0].hit.as<int>(), nullptr,
                         nullptr, ctx->ws[0].spill.as<uint2>(), trace_grid(ctx) * trace_block_size(), ctrl, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> words(n);
    unsigned host_ctrl[4];
    HIP_TRY(ctx, hipMemcpyAsync(words.data(), ctx->ws[0].hit.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(host_ctrl, ctrl, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (host_ctrl[YK_CTRL_ERR] & 1u) return fail(ctx, YK_ERR_STACK_OVERFLOW, "BVH traversal stack exceeded 64 entries (bvh.rs:174)");
    const HostBvh* tree = scene_host_tree(scene);  // the surface kernel indexes the leaf-order records by these words: none may lie outside them
    if (!tree) return fail(ctx, YK_ERR_DEVICE, "the scene's shape order could not be copied back from the device");
    for (size_t i = 0; i < n; ++i)
        if (words[i] != -1 && (words[i] < 0 || ((uint32_t)words[i] & YK_HIT_PRIM_MASK) >= tree->shape_order.size()))
            return fail(ctx, YK_ERR_DEVICE, "yk_surface: ray " + std::to_string(i) + " got hit word " + std::to_string(words[i]));
    launch_surface_test(st, dev_scene_for(scene, n), n, pb.rayO, pb.rayD, ctx->ws[0].hit.as<int>(), route, d_out);
    sg.check(hipGetLastError());
    return sg.finish();
} YK_CATCH(ctx)

yk_status yk_trace_any(yk_context* ctx, const yk_scene* scene, size_t n, const float* ray_o, const float* ray_d, const float* t_max,
                       const int32_t* area_light, uint8_t* out_hit) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!scene || !ray_o || !ray_d || !t_max || !out_hit || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (yk_status rs = scene_on_context(ctx, scene, "")) return rs;
    if (n > 0xFFFFFF00ull) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "too many rays");
    yk_status wb = check_stage_kernel(ctx, scene, false, t_max, false);
    if (wb != YK_OK) return wb;
    const int64_t mode = ctx->trace_stage_kernel;
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    if ((wb = ensure_work_buffers(ctx, ctx->ws[0], n, scene->n_lights, scene->n_delta_lights)) != YK_OK) return wb;
    if ((wb = ensure_spill(ctx, ctx->ws[0])) != YK_OK) return wb;
    const unsigned* slot_of = mode != 0 ? upload_reversed_slots(sg, n) : nullptr;
    const float* d_o = sg.upload(ray_o, n * 3);
    const float* d_d = sg.upload(ray_d, n * 3);
    const float* d_t_max = sg.upload(t_max, n);
    const int32_t* d_area_light = area_light ? sg.upload(area_light, n) : nullptr;
    if (!sg.ok()) return sg.status();
    launch_pack_shadow_rays(st, n, d_o, d_d, d_t_max, d_area_light, ctx->ws[0].shO.as<float4>(), ctx->ws[0].shD.as<float4>());
    unsigned* ctrl = ctx->ws[0].ctrl.as<unsigned>();
    HIP_TRY(ctx, hipMemsetAsync(ctrl, 0, YK_CTRL_WORDS * 4, st));
    unsigned nn = (unsigned)n;
    HIP_TRY(ctx, hipMemcpyAsync(ctrl, &nn, 4, hipMemcpyHostToDevice, st));
    if (slot_of) HIP_TRY(ctx, hipMemsetAsync(ctx->ws[0].vis.p, 0, n, st));  // as k_shade leaves it: the kernels only mark occluded slots
    HIP_TRY(ctx, hipStreamSynchronize(st));
    // the stage's queue: the packed rays, word 0 of the control block as their count (yk_device.h)
    const ShadowQueue q{ctx->ws[0].shO.as<float4>(), ctx->ws[0].shD.as<float4>(), const_cast<unsigned*>(slot_of), ctrl, ctrl + YK_CTRL_HEADS};
    if (mode == 2)
        launch_trace_any_packet(st, packet_grid(ctx), dev_scene_for(scene, n), q, ctx->ws[0].vis.as<unsigned char>(), nullptr);
    else
        launch_trace_any(st, trace_grid(ctx), dev_scene_for(scene, n), q, ctx->ws[0].vis.as<unsigned char>(), ctx->ws[0].spill.as<uint2>(),
                         trace_grid(ctx) * trace_block_size(), ctrl, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint8_t> vis(slot_of ? n : 0);
    HIP_TRY(ctx, hipMemcpyAsync(slot_of ? vis.data() : out_hit, ctx->ws[0].vis.p, n, hipMemcpyDeviceToHost, st));
    unsigned host_ctrl[4];
    HIP_TRY(ctx, hipMemcpyAsync(host_ctrl, ctrl, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (host_ctrl[YK_CTRL_ERR] & 1u) return fail(ctx, YK_ERR_STACK_OVERFLOW, "BVH traversal stack exceeded 64 entries (bvh.rs:174)");
    for (size_t k = 0; k < vis.size(); ++k) {  // ray k's verdict is in slot n - 1 - k: 2 occluded, 0 untouched
        const uint8_t v = vis[n - 1 - k];
        if (v != 0 && v != 2)
            return fail(ctx, YK_ERR_DEVICE, "trace_stage_kernel " + std::to_string(mode) + ": slot " + std::to_string(n - 1 - k) + " holds " + std::to_string(v));
        out_hit[k] = v == 2 ? 1 : 0;
    }
    return YK_OK;
} YK_CATCH(ctx)

yk_status yk_sampler_sequence(yk_context* ctx, const yk_sampler_desc* sampler, uint16_t px, uint16_t py, uint32_t sample_index, const uint8_t* dims,
                              size_t n_draws, float* out) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!sampler || !dims || !out || n_draws == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    RenderParams prm;
    yk_integrator_desc dummy = {YK_INTEGRATOR_PATH, 1, 0, 0.0f};
    yk_status ps = make_params(ctx, sampler, &dummy, prm);
    if (ps != YK_OK) return ps;
    // permutation_element (stratified.rs:147-178) walks a bijection of the next power of two until it lands below spp.  From an
    // index below spp the walk returns to it at the latest; from one at or past spp it may enter a cycle that lies wholly in
    // spp .. 2^k - 1 and never end, so those are refused here as the render entry points refuse them (a power of two has no such cycle).
    const uint32_t spp = prm.sampler.spp;
    if (sampler->kind == YK_SAMPLER_STRATIFIED && sample_index >= spp && (spp & (spp - 1)) != 0)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "stratified sample_index >= samples per pixel, and that is no power of two: the permutation walk need not end");
    Staging sg(ctx);
    const uint8_t* d_dims = sg.upload(dims, n_draws);
    float* d_out = sg.output(out, n_draws * 2);
    if (!sg.ok()) return sg.status();
    launch_sampler_sequence(sg.stream, prm.sampler, px, py, sample_index, d_dims, n_draws, d_out);
    sg.check(hipGetLastError());
    return sg.finish();
}

yk_status yk_camera_rays(yk_context* ctx, const yk_camera* camera, const yk_sampler_desc* sampler, const yk_tile* tile, uint32_t sample_index,
                         float* out_o, float* out_d) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!camera || !sampler || !tile || !out_o || !out_d) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (tile->x0 >= tile->x1 || tile->y0 >= tile->y1) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "Bounds2 with a dimension <= 0");
    RenderParams prm;
    yk_integrator_desc dummy = {YK_INTEGRATOR_PATH, 1, 0, 0.0f};
    yk_status ps = make_params(ctx, sampler, &dummy, prm);
    if (ps != YK_OK) return ps;
    if (sample_index >= prm.sampler.spp) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "sample_index >= samples per pixel");
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    const uint32_t npx = (uint32_t)(tile->x1 - tile->x0) * (uint32_t)(tile->y1 - tile->y0);
    const uint32_t spp = prm.sampler.spp;
    yk_status wb = ensure_work_buffers(ctx, ctx->ws[0], (size_t)npx * spp, 1, 0);
    if (wb != YK_OK) return wb;
    uint32_t off[2] = {0, npx};
    HIP_TRY(ctx, ctx->tiles.ensure(sizeof(yk_tile)));
    HIP_TRY(ctx, ctx->tile_off.ensure(8));
    HIP_TRY(ctx, ctx->pixel_xy.ensure((size_t)npx * 4));
    HIP_TRY(ctx, ctx->sample_buf.ensure((size_t)npx * spp * 16));
    std::vector<float> o((size_t)npx * spp * 3), d((size_t)npx * spp * 3);
    float* d_o = sg.output(o.data(), o.size());
    float* d_d = sg.output(d.data(), d.size());
    if (!sg.ok()) return sg.status();
    HIP_TRY(ctx, hipMemcpyAsync(ctx->tiles.p, tile, sizeof(yk_tile), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->tile_off.p, off, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    launch_pixel_table(st, ctx->tiles.as<yk_tile>(), ctx->tile_off.as<uint32_t>(), 1, npx, ctx->pixel_xy.as<uint32_t>());
    DevCamera cam;
    std::memcpy(cam.c2w, camera->camera_to_world, 64);
    std::memcpy(cam.r2c, camera->raster_to_camera, 64);
    PathBuffers pb = path_buffers(ctx->ws[0], 0);
    launch_raygen(st, cam, prm, ctx->pixel_xy.as<uint32_t>(), nullptr, 0, npx * spp, pb, ctx->sample_buf.as<float4>(), ctx->ws[0].ctrl.as<unsigned>());
    launch_unpack_rays(st, (size_t)npx * spp, pb.rayO, pb.rayD, d_o, d_d);
    sg.check(hipGetLastError());
    if (yk_status fs = sg.finish()) return fs;
    for (uint32_t p = 0; p < npx; ++p)
        for (int k = 0; k < 3; ++k) {
            out_o[3 * p + k] = o[3 * ((size_t)p * spp + sample_index) + k];
            out_d[3 * p + k] = d[3 * ((size_t)p * spp + sample_index) + k];
        }
    return YK_OK;
} YK_CATCH(ctx)

yk_status yk_host_math(int fn, size_t n, const float* a, const float* b, float* out) {
    if (!a || !out) return YK_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; ++i) {
        const float x = a[i], y = b ? b[i] : 0.0f;
        float sn, cs;
        switch (fn) {
            case 0: out[i] = det_sinf(x); break;
            case 1: out[i] = det_cosf(x); break;
            case 2: out[i] = det_tanf(x); break;
            case 3: out[i] = det_logf(x); break;
            case 4: out[i] = det_acosf(x); break;
            case 5: out[i] = det_atan2f(x, y); break;
            case 28: det_sincosf(x, sn, cs); out[i] = sn; break;
            case 29: det_sincosf(x, sn, cs); out[i] = cs; break;
            case 30: out[i] = det_expf(x); break;
            default: return YK_ERR_INVALID_ARGUMENT;
        }
    }
    return YK_OK;
}

yk_status yk_device_math(yk_context* ctx, int fn, size_t n, const float* a, const float* b, float* out) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!a || !out || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    Staging sg(ctx);
    const float* d_a = sg.upload(a, n);
    const float* d_b = b ? sg.upload(b, n) : nullptr;
    float* d_out = sg.output(out, n);
    if (!sg.ok()) return sg.status();
    launch_device_math(sg.stream, fn, n, d_a, d_b, d_out);
    sg.check(hipGetLastError());
    return sg.finish();
}

static yk_status bsdf_common(yk_context* ctx, const yk_material_desc* material, size_t n, const float* n_geom, const float* n_shading,
                             const float* dpdu, const float* wo, const float* x, int sample, float* out) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!material || !n_geom || !n_shading || !dpdu || !wo || !x || !out || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    Staging sg(ctx);
    const float* d_n_geom = sg.upload(n_geom, n * 3);
    const float* d_n_shading = sg.upload(n_shading, n * 3);
    const float* d_dpdu = sg.upload(dpdu, n * 3);
    const float* d_wo = sg.upload(wo, n * 3);
    const float* d_x = sg.upload(x, n * (sample ? 2 : 3));
    float* d_out = sg.output(out, n * (sample ? 8 : 3));
    if (!sg.ok()) return sg.status();
    launch_bsdf_test(sg.stream, make_material(*material), n, d_n_geom, d_n_shading, d_dpdu, d_wo, d_x, sample, d_out);
    sg.check(hipGetLastError());
    return sg.finish();
}

yk_status yk_bsdf_eval(yk_context* ctx, const yk_material_desc* material, size_t n, const float* n_geom, const float* n_shading, const float* dpdu,
                       const float* wo, const float* wi, float* out_f) {
    return bsdf_common(ctx, material, n, n_geom, n_shading, dpdu, wo, wi, 0, out_f);
}
yk_status yk_bsdf_sample(yk_context* ctx, const yk_material_desc* material, size_t n, const float* n_geom, const float* n_shading, const float* dpdu,
                         const float* wo, const float* u, float* out8) {
    return bsdf_common(ctx, material, n, n_geom, n_shading, dpdu, wo, u, 1, out8);
}

yk_status yk_light_sample(yk_context* ctx, const yk_light_desc* light, int32_t light_index, size_t n, const float* p, const float* n_geom,
                          const float* u, float* out18) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!light || !p || !n_geom || !u || !out18 || n == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null argument");
    if (light->kind > YK_LIGHT_RECT) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "unknown light kind");
    Staging sg(ctx);
    const float* d_p = sg.upload(p, n * 3);
    const float* d_n_geom = sg.upload(n_geom, n * 3);
    const float* d_u = sg.upload(u, n * 2);
    float* d_out = sg.output(out18, n * 18);
    if (!sg.ok()) return sg.status();
    launch_light_test(sg.stream, make_light(*light), light_index, n, d_p, d_n_geom, d_u, d_out);
    sg.check(hipGetLastError());
    return sg.finish();
}

}  // extern "C"
