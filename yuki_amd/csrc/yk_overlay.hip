// yk_overlay.hip — the ray and BVH-level overlays (app/renderpasses/ray_visualization.rs, bvh_visualization.rs) on gfx950, behind
// yk_overlay_draw and yk_overlay_draw_device, plus the host functions that feed them (yk_scene_node_bounds,
// yk_overlay_world_to_clip, yk_overlay_ray_lines).  The per-segment arithmetic is yk_overlay.h's, whose host instance
// yk_overlay_draw runs without a context.
//
// "The last primitive in list order wins a pixel" (rule 7) must not depend on scheduling, so the device draws in two passes
// over a context-owned u32 id buffer of res_x * res_y words, cleared on the stream:
//   - k_overlay_lines / k_overlay_boxes: every pixel a primitive covers does an integer atomicMax of (ordinal + 1) — order
//     independent, so the result is bitwise reproducible; no float atomics anywhere;
//   - k_overlay_resolve: a pixel whose id is not 0 gets the colour of that ordinal; no other pixel is touched, so the film
//     may be updated in place, at any 4-byte alignment.
// Work split:
//   - lines (a debug sample: dozens of segments, up to thousands of pixels each): one wave per line, the 64 lanes stride over
//     its pixels;
//   - boxes (a tree level: thousands; every level: millions, most edges a few pixels): 16 lanes per box, 4 boxes per wave.
//     Lanes 0-7 transform one corner each, the 8 outcodes are and-ed within the group, and a box wholly outside one clip
//     plane is dropped before any edge is set up; lanes 0-11 then take one edge each, reading its two corners with lane
//     shuffles.  An edge shorter than `coop_min` pixels is drawn by its own lane; longer ones are handed round the wave
//     one after the other (ballot + shuffles) and drawn by all 64 lanes, so that no lane serialises a film-long edge.
#include <hip/hip_runtime.h>

#include <cstring>
#include <deque>
#include <vector>

#include "yk_film_call.h"
#include "yk_libm.h"
#include "yk_overlay.h"
#include "yk_staging.h"

namespace {

constexpr unsigned OV_BLOCK = 256;        // 4 waves of 64
constexpr unsigned OV_MAX_BLOCKS = 2048;  // grid cap (8 blocks on each of 256 CUs); the rest is grid-strided
constexpr unsigned OV_BOX_LANES = 16;     // lanes per box
constexpr unsigned OV_BOXES_PER_BLOCK = OV_BLOCK / OV_BOX_LANES;
constexpr size_t OV_LINE_FLOATS = sizeof(yk_overlay_line) / sizeof(float);
static_assert(sizeof(yk_overlay_line) == 36, "yk_overlay_line is nine floats");

struct OvArgs {
    float m[16];  // world_to_clip, row-major
    uint32_t res_x, res_y;
    uint32_t n_lines;   // the ordinal of box 0's edge 0
    uint32_t coop_min;  // pixels from which a box edge is drawn by the whole wave
};

// The first pass's write.  A timing-only build (make EXTRA=-DYK_OVERLAY_TIMING_PLAIN_STORES OUT=... BUILD=...) stores
// instead, to price the atomics: its film depends on scheduling, so it is measured, never shipped.
__device__ __forceinline__ void ov_mark(uint32_t* ids, uint32_t index, uint32_t tag) {
#ifdef YK_OVERLAY_TIMING_PLAIN_STORES
    ids[index] = tag;
#else
    atomicMax(ids + index, tag);
#endif
}

// All 64 lanes draw one span; `tag` = ordinal + 1.
__device__ __forceinline__ void ov_draw_wave(const OvSpan& s, uint32_t tag, const OvArgs& a, uint32_t* ids, int lane) {
    for (int32_t k = s.k_lo + lane; k < s.k_hi; k += 64) {
        uint32_t index;
        if (ov_pixel(s, k, a.res_x, a.res_y, index)) ov_mark(ids, index, tag);
    }
}

// One wave per line.
__global__ __launch_bounds__(OV_BLOCK) void k_overlay_lines(const float* __restrict__ lines, uint32_t n_lines, uint32_t* ids, OvArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * OV_BLOCK + threadIdx.x) >> 6, n_waves = (gridDim.x * OV_BLOCK) >> 6;
    for (uint32_t i = wave; i < n_lines; i += n_waves) {
        const float* l = lines + OV_LINE_FLOATS * i;
        const OvClip c0 = ov_clip_point(a.m, l[0], l[1], l[2]);
        const OvClip c1 = ov_clip_point(a.m, l[3], l[4], l[5]);
        OvSpan s;
        if (!ov_span(c0, c1, a.res_x, a.res_y, s)) continue;
        ov_draw_wave(s, i + 1u, a, ids, (int)lane);
    }
}

// 16 lanes per box; every wave runs the same number of rounds, so that the shuffles below always see all 64 lanes.
__global__ __launch_bounds__(OV_BLOCK) void k_overlay_boxes(const float* __restrict__ boxes, uint32_t n_boxes, uint32_t* ids, OvArgs a) {
    const uint32_t lane = threadIdx.x & 63u, sub = threadIdx.x & (OV_BOX_LANES - 1u), base = lane & ~(OV_BOX_LANES - 1u);
    const uint32_t group = (blockIdx.x * OV_BLOCK + threadIdx.x) / OV_BOX_LANES, n_groups = gridDim.x * OV_BOXES_PER_BLOCK;
    const uint32_t rounds = (n_boxes + n_groups - 1u) / n_groups;
    for (uint32_t round = 0; round < rounds; ++round) {
        const uint64_t b64 = (uint64_t)round * n_groups + group;
        const bool valid = b64 < n_boxes;
        const uint32_t b = (uint32_t)b64;
        OvClip c{0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t code = 63u;
        if (valid && sub < 8u) {
            const float* box = boxes + 6u * (size_t)b;
            float x, y, z;
            ov_box_corner(box, sub, x, y, z);
            c = ov_clip_point(a.m, x, y, z);
            code = ov_outcode(c);
        }
        code &= __shfl_xor(code, 1, 64);
        code &= __shfl_xor(code, 2, 64);
        code &= __shfl_xor(code, 4, 64);
        code = __shfl(code, (int)base, 64);  // the and over the 8 corners: not 0 = every edge fails one plane at both ends
        const bool has = valid && sub < 12u && code == 0u;
        if (!__any(has)) continue;
        uint32_t i0, i1;
        ov_edge_ends(sub < 12u ? sub : 0u, i0, i1);
        const int l0 = (int)(base + i0), l1 = (int)(base + i1);
        const OvClip c0{__shfl(c.x, l0, 64), __shfl(c.y, l0, 64), __shfl(c.z, l0, 64), __shfl(c.w, l0, 64)};
        const OvClip c1{__shfl(c.x, l1, 64), __shfl(c.y, l1, 64), __shfl(c.z, l1, 64), __shfl(c.w, l1, 64)};
        OvSpan s{0, 0, 0u, 0.0f, 0.0f, 0.0f};
        uint32_t n = 0;
        if (has && ov_span(c0, c1, a.res_x, a.res_y, s)) n = (uint32_t)(s.k_hi - s.k_lo);
        const uint32_t tag = a.n_lines + 12u * b + sub + 1u;
        if (n != 0u && n < a.coop_min) {
            for (int32_t k = s.k_lo; k < s.k_hi; ++k) {
                uint32_t index;
                if (ov_pixel(s, k, a.res_x, a.res_y, index)) ov_mark(ids, index, tag);
            }
        }
        unsigned long long pending = __ballot(n >= a.coop_min);
        while (pending) {
            const int src = __ffsll((long long)pending) - 1;
            pending &= pending - 1ull;
            OvSpan w;
            w.k_lo = __shfl(s.k_lo, src, 64);
            w.k_hi = __shfl(s.k_hi, src, 64);
            w.x_major = __shfl(s.x_major, src, 64);
            w.a = __shfl(s.a, src, 64);
            w.m_a = __shfl(s.m_a, src, 64);
            w.slope = __shfl(s.slope, src, 64);
            ov_draw_wave(w, __shfl(tag, src, 64), a, ids, (int)lane);
        }
    }
}

// ids -> film: the colour of ordinal id - 1 where id != 0.
__global__ __launch_bounds__(OV_BLOCK) void k_overlay_resolve(const uint32_t* __restrict__ ids, const float* __restrict__ lines, uint32_t n_lines, uint32_t n_px, float* film) {
    const uint32_t stride = gridDim.x * OV_BLOCK;
    for (uint64_t p = blockIdx.x * OV_BLOCK + threadIdx.x; p < n_px; p += stride) {
        const uint32_t id = ids[p];
        if (id == 0u) continue;
        const uint32_t ordinal = id - 1u;
        float r, g, b;
        if (ordinal < n_lines) {
            const float* l = lines + OV_LINE_FLOATS * ordinal;
            r = l[6];
            g = l[7];
            b = l[8];
        } else {
            ov_box_colour((ordinal - n_lines) / 12u, r, g, b);
        }
        film[3 * p] = r;
        film[3 * p + 1] = g;
        film[3 * p + 2] = b;
    }
}

unsigned ov_grid(uint64_t items, unsigned per_block) { return (unsigned)std::min<uint64_t>((items + per_block - 1) / per_block, OV_MAX_BLOCKS); }

yk_status check_call(const float* m, const void* lines, size_t n_lines, const void* boxes, size_t n_boxes, const void* film, uint16_t res_x, uint16_t res_y) {
    if (!m || !film || res_x == 0 || res_y == 0 || (n_lines && !lines) || (n_boxes && !boxes)) return YK_ERR_INVALID_ARGUMENT;
    // ordinal + 1 is a u32
    if (n_lines > 0xFFFFFFFEull || n_boxes > 0xFFFFFFFEull / 12 || n_lines + 12 * n_boxes > 0xFFFFFFFEull) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue(yk_context* ctx, hipStream_t st, const float* m, const float* d_lines, size_t n_lines, const float* d_boxes, size_t n_boxes, float* d_film,
                  uint16_t res_x, uint16_t res_y) {
    if (n_lines == 0 && n_boxes == 0) return YK_OK;
    const uint32_t n_px = (uint32_t)res_x * res_y;
    auto& ov = ctx->overlay;
    HIP_TRY(ctx, ov.ids.ensure((size_t)n_px * 4));
    OvArgs a;
    std::memcpy(a.m, m, 64);
    a.res_x = res_x;
    a.res_y = res_y;
    a.n_lines = (uint32_t)n_lines;
    a.coop_min = (uint32_t)ov.coop_min;
    uint32_t* ids = ov.ids.as<uint32_t>();
    HIP_TRY(ctx, hipMemsetAsync(ids, 0, (size_t)n_px * 4, st));
    if (n_lines) hipLaunchKernelGGL(k_overlay_lines, dim3(ov_grid(n_lines, OV_BLOCK / 64)), dim3(OV_BLOCK), 0, st, d_lines, (uint32_t)n_lines, ids, a);
    if (n_boxes) hipLaunchKernelGGL(k_overlay_boxes, dim3(ov_grid(n_boxes, OV_BOXES_PER_BLOCK)), dim3(OV_BLOCK), 0, st, d_boxes, (uint32_t)n_boxes, ids, a);
    hipLaunchKernelGGL(k_overlay_resolve, dim3(ov_grid(n_px, OV_BLOCK)), dim3(OV_BLOCK), 0, st, ids, d_lines, (uint32_t)n_lines, n_px, d_film);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void host_segment(const OvClip& c0, const OvClip& c1, const float* rgb, float* film, uint16_t res_x, uint16_t res_y) {
    OvSpan s;
    if (!ov_span(c0, c1, res_x, res_y, s)) return;
    for (int32_t k = s.k_lo; k < s.k_hi; ++k) {
        uint32_t index;
        if (!ov_pixel(s, k, res_x, res_y, index)) continue;
        film[3 * (size_t)index] = rgb[0];
        film[3 * (size_t)index + 1] = rgb[1];
        film[3 * (size_t)index + 2] = rgb[2];
    }
}

// The host instance: the primitives one after the other in list order, each overwriting what it covers.
void host_draw(const float* m, const yk_overlay_line* lines, size_t n_lines, const float* boxes, size_t n_boxes, float* film, uint16_t res_x, uint16_t res_y) {
    for (size_t i = 0; i < n_lines; ++i) {
        const yk_overlay_line& l = lines[i];
        host_segment(ov_clip_point(m, l.p0[0], l.p0[1], l.p0[2]), ov_clip_point(m, l.p1[0], l.p1[1], l.p1[2]), l.rgb, film, res_x, res_y);
    }
    for (size_t b = 0; b < n_boxes; ++b) {
        OvClip c[8];
        for (uint32_t j = 0; j < 8; ++j) {
            float x, y, z;
            ov_box_corner(boxes + 6 * b, j, x, y, z);
            c[j] = ov_clip_point(m, x, y, z);
        }
        float rgb[3];
        ov_box_colour((uint32_t)b, rgb[0], rgb[1], rgb[2]);
        for (uint32_t e = 0; e < 12; ++e) {
            uint32_t i0, i1;
            ov_edge_ends(e, i0, i1);
            host_segment(c[i0], c[i1], rgb, film, res_x, res_y);
        }
    }
}

}  // namespace

extern "C" {

// BoundingVolumeHierarchy::node_bounds (bvh.rs:121-157), statement by statement.
size_t yk_scene_node_bounds(const yk_scene* scene, int32_t target_level, float* out_bounds, size_t cap) try {
    const HostBvh* tree = scene_host_tree(scene);
    if (!tree || tree->nodes.empty()) return 0;
    const std::vector<yk_bvh_node>& nodes = tree->nodes;
    size_t n = 0;
    auto push = [&](const yk_bvh_node& node) {
        if (out_bounds && n < cap) {
            std::memcpy(out_bounds + 6 * n, node.bmin, 12);
            std::memcpy(out_bounds + 6 * n + 3, node.bmax, 12);
        }
        ++n;
    };
    if (target_level <= 0) push(nodes[0]);
    struct Item {
        size_t index;
        int32_t level;
    };
    std::deque<Item> queue{Item{0, 1}};
    while (!queue.empty()) {
        const Item it = queue.front();
        queue.pop_front();
        if (target_level >= 0 && it.level > target_level) break;
        const yk_bvh_node& node = nodes[it.index];
        if (!node.is_leaf) {
            const size_t second = node.a;
            if (target_level < 0 || it.level == target_level) {
                push(nodes[it.index + 1]);
                push(nodes[second]);
            }
            queue.push_back(Item{it.index + 1, it.level + 1});
            queue.push_back(Item{second, it.level + 1});
        }
    }
    return n;
} catch (const std::exception&) {
    return 0;
}

// `world_to_clip` of RayVisualization::draw (ray_visualization.rs:80-150) and BvhVisualization::draw (bvh_visualization.rs:101-171).
yk_status yk_overlay_world_to_clip(const yk_camera_params* p, const float scene_bounds[6], float out[16]) {
    if (!p || !scene_bounds || !out || p->res_x == 0 || p->res_y == 0) return YK_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 6; ++k)
        if (!ov_finite(scene_bounds[k])) return YK_ERR_INVALID_ARGUMENT;
    bool ok = true;
    const Xf world_to_camera = xf_look_at(p->position, p->target, p->up, &ok);  // :87-91
    if (!ok) return YK_ERR_INVALID_ARGUMENT;
    const float* p0 = scene_bounds;
    const float* p1 = scene_bounds + 3;
    const V3 bb_points[8] = {V3{p0[0], p0[1], p0[2]}, V3{p0[0], p0[1], p1[2]}, V3{p0[0], p1[1], p0[2]}, V3{p0[0], p1[1], p1[2]},
                             V3{p1[0], p0[1], p0[2]}, V3{p1[0], p0[1], p1[2]}, V3{p1[0], p1[1], p0[2]}, V3{p1[0], p1[1], p1[2]}};  // :97-106
    const V3 position{p->position[0], p->position[1], p->position[2]};
    float zf = 0.0f;  // :108-110: fold(0.0, |acc, p| (p - position).len().max(acc)); f32::max returns the other operand for a NaN
    for (int k = 0; k < 8; ++k) zf = rmax(length(bb_points[k] - position), zf);
    if (!(zf > 0.0f) || !ov_finite(zf)) return YK_ERR_INVALID_ARGUMENT;
    const float zn = zf * 1e-5f;                             // :111
    const float half = p->fov_degrees * 0.5f;                // :116: (fov * 0.5).to_radians().tan()
    const float tan_half_fov = det_tanf(half * (YK_PI / 180.0f));
    float xf, yf;  // :117-126
    if (p->fov_axis == 0) {
        const float ar = (float)p->res_y / (float)p->res_x;
        xf = 1.0f / tan_half_fov;
        yf = 1.0f / (tan_half_fov * ar);
    } else {
        const float ar = (float)p->res_x / (float)p->res_y;
        xf = 1.0f / (tan_half_fov * ar);
        yf = 1.0f / tan_half_fov;
    }
    Xf camera_to_clip = xf_identity(), flip_y = xf_identity();  // only .m is read below
    const float c2c[16] = {xf, 0.0f, 0.0f, 0.0f, 0.0f, yf, 0.0f, 0.0f, 0.0f, 0.0f, (zf + zn) / (zf - zn), -(2.0f * zf * zn) / (zf - zn), 0.0f, 0.0f, 1.0f, 0.0f};  // :128-138
    std::memcpy(camera_to_clip.m, c2c, 64);
    flip_y.m[5] = -1.0f;  // :142-147
    const Xf trfn = xf_mul(flip_y, xf_mul(camera_to_clip, world_to_camera));  // :149
    // :152-157 transposes m for the GL uniform, which GLSL reads column-major: the shader's matrix is m again.
    std::memcpy(out, trfn.m, 64);
    for (int k = 0; k < 16; ++k)
        if (!ov_finite(out[k])) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

// RayVisualization::set_rays (ray_visualization.rs:28-56).
yk_status yk_overlay_ray_lines(const yk_integrator_ray* rays, size_t n, yk_overlay_line* out) {
    if (n > 32768 || (n && (!rays || !out))) return YK_ERR_INVALID_ARGUMENT;  // :53-54 index with u16
    for (size_t i = 0; i < n; ++i) {
        const yk_integrator_ray& r = rays[i];
        yk_overlay_line l;
        if (!ov_ray_colour(r.ray_type, l.rgb[0], l.rgb[1], l.rgb[2])) return YK_ERR_INVALID_ARGUMENT;
        for (int k = 0; k < 3; ++k) {
            l.p0[k] = r.o[k];
            float s = r.d[k] * r.t_max;  // :44 ray.o + ray.d * ray.t_max
            l.p1[k] = r.o[k] + s;
        }
        out[i] = l;
    }
    return YK_OK;
}

yk_status yk_overlay_draw(yk_context* ctx, const float world_to_clip[16], const yk_overlay_line* lines, size_t n_lines, const float* boxes, size_t n_boxes,
                          float* film_rgb, uint16_t res_x, uint16_t res_y) try {
    if (check_call(world_to_clip, lines, n_lines, boxes, n_boxes, film_rgb, res_x, res_y) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_overlay_draw: bad argument");
    if (!ctx) {
        host_draw(world_to_clip, lines, n_lines, boxes, n_boxes, film_rgb, res_x, res_y);
        return YK_OK;
    }
    if (n_lines == 0 && n_boxes == 0) return YK_OK;
    YK_LOCK(ctx);
    Staging sg(ctx);
    float* d_film = sg.inout(film_rgb, (size_t)res_x * res_y * 3);
    const yk_overlay_line* d_lines = sg.upload(lines, n_lines);
    const float* d_boxes = sg.upload(boxes, n_boxes * 6);
    return sg.run([&] { return enqueue(ctx, sg.stream, world_to_clip, reinterpret_cast<const float*>(d_lines), n_lines, d_boxes, n_boxes, d_film, res_x, res_y); });
} YK_CATCH(ctx)

yk_status yk_overlay_draw_device(yk_context* ctx, const float world_to_clip[16], const void* d_lines, size_t n_lines, const void* d_boxes, size_t n_boxes,
                                 void* d_film_rgb, uint16_t res_x, uint16_t res_y, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(world_to_clip, d_lines, n_lines, d_boxes, n_boxes, d_film_rgb, res_x, res_y) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_overlay_draw_device: bad argument");
    return enqueue(ctx, device_call_stream(ctx, stream), world_to_clip, reinterpret_cast<const float*>(d_lines), n_lines, reinterpret_cast<const float*>(d_boxes), n_boxes,
                   reinterpret_cast<float*>(d_film_rgb), res_x, res_y);
}

}  // extern "C"
