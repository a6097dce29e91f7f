// yk_variance.hip — the variance-guided denoise on gfx950, behind yk_moments_blend, yk_variance and yk_denoise_variance and
// their _device forms; the per-pixel arithmetic is yk_variance.h's, whose host instance these entry points run without a
// context.
//
// k_moments_blend: streaming, one lane per pixel, k_blend's sibling: three dword loads of the film, one 16-byte load and one
//   16-byte store of the records.  "No table" and "no history" are template variants.  A lane reads its own pixel only, and
//   before it writes it, so the output may be the input moments.
// k_variance: one lane per pixel, a block is a VR_TX x VR_TY tile of the film.  The temporal estimate is one 16-byte load
//   (two with an albedo) and a handful of VALU operations.  Whether the block evaluates the 7 x 7 window at all is decided
//   once per block (__syncthreads_or over "this lane has no temporal estimate"): after the first frames nearly no block
//   does.  A block that does stages the guides and the luminance of its tile plus a halo of 3 in LDS (38 x 14 records of two
//   float4: (ns, hit) and (p, l) — the luminance rides in the slot of the guide's unused t) and only the lanes that need
//   the window walk it.  Entries outside the film are neither written nor read.
// k_vprep: the film (normalised, with an albedo demodulated) and the sanitised variance as (r, g, b, var) records into the
//   context's ping buffer.
// k_atrous_var<S, LAST>: one launch per iteration, the shape of k_atrous.  S == 0 takes its taps from global memory; S == 1
//   and 2 stage colours (with the variance in the fourth float) and guides of the tile plus a halo of 2*S in LDS.  The 3 x 3
//   variance taps lie inside that halo, since 2*S >= 1.  "denoise_lds_max_step" picks the variant per step, as for
//   yk_denoise.  LAST writes RGB, multiplied by the pixel's own divisors when the albedo pointer is not NULL (a uniform
//   branch on a kernel argument).
// The ping-pong buffers and the staged sample table are the denoiser's (ctx->denoise), the blend's table the temporal
// pass's: the calls are ordered on one stream with those passes and never run beside them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_staging.h"
#include "yk_variance.h"

namespace {

constexpr unsigned VR_TX = 32, VR_TY = 8;  // 256 lanes: 4 waves of 64

// ------------------------------------------------------------------ moments blend
struct VrBlendIo {
    const float* film;
    const uint32_t* samples;
    const float4* moments;
    float4* out;
};

template <bool TABLE, bool HIST>
__global__ __launch_bounds__(256) void k_moments_blend(VrBlendIo io, TpParams a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.dn.res_x * a.dn.res_y) return;
    const float c[3] = {io.film[3 * (size_t)i], io.film[3 * (size_t)i + 1], io.film[3 * (size_t)i + 2]};
    float m = 1.0f;
    if (TABLE) {
        const uint32_t y = i / a.dn.res_x, x = i - y * a.dn.res_x;
        m = dn_count(a.dn, io.samples, x, y);
    }
    float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HIST) {
        const float4 v = io.moments[i];
        h[0] = v.x;
        h[1] = v.y;
        h[2] = v.z;
        h[3] = v.w;
    }
    float rec[4];
    vr_moments_pixel(a, TABLE, m, c, HIST ? h : nullptr, rec);
    io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

bool temporal_desc_ok(const yk_temporal_desc* d) {  // yk_history_blend's rule
    if (!d) return false;
    if (!(d->plane_tolerance > 0.0f)) return false;
    if (!(d->normal_cos_min >= -1.0f) || !(d->normal_cos_min <= 1.0f)) return false;
    if (!(d->max_history >= 1.0f)) return false;
    return true;
}

TpParams make_blend_params(const yk_temporal_desc* d, uint16_t res_x, uint16_t res_y, uint16_t tile_dim) {
    TpParams a{};
    dn_set_grid(a.dn, res_x, res_y, tile_dim);
    a.plane_tolerance = d->plane_tolerance;
    a.normal_cos_min = d->normal_cos_min;
    a.max_history = d->max_history;
    return a;
}

yk_status check_blend(const yk_temporal_desc* d, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* moments, const void* out) {
    if (!temporal_desc_ok(d) || !film || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * 16, film, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (moments && out != moments && overlaps(out, n_px * 16, moments, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue_blend(yk_context* ctx, hipStream_t st, const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                        const void* moments, void* out) {
    const TpParams a = make_blend_params(d, res_x, res_y, tile_dim);
    VrBlendIo io{};
    io.film = film;
    io.moments = reinterpret_cast<const float4*>(moments);
    io.out = reinterpret_cast<float4*>(out);
    if (samples) {
        yk_status ss = stage_sample_table(ctx, st, samples, res_x, res_y, tile_dim, ctx->temporal.samples);
        if (ss != YK_OK) return ss;
        io.samples = ctx->temporal.samples.as<const uint32_t>();
    }
    const uint32_t n_px = (uint32_t)res_x * res_y;
    const dim3 grid((n_px - 1) / 256 + 1), block(256);
    if (io.samples && io.moments) hipLaunchKernelGGL((k_moments_blend<true, true>), grid, block, 0, st, io, a);
    else if (io.samples) hipLaunchKernelGGL((k_moments_blend<true, false>), grid, block, 0, st, io, a);
    else if (io.moments) hipLaunchKernelGGL((k_moments_blend<false, true>), grid, block, 0, st, io, a);
    else hipLaunchKernelGGL((k_moments_blend<false, false>), grid, block, 0, st, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void blend_host(const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const yk_moments* moments, yk_moments* out) {
    const TpParams a = make_blend_params(d, res_x, res_y, tile_dim);
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            float c[3], h[4], rec[4];
            std::memcpy(c, film + 3 * i, 12);
            if (moments) std::memcpy(h, &moments[i], 16);
            vr_moments_pixel(a, samples != nullptr, samples ? dn_count(a.dn, samples, x, y) : 1.0f, c, moments ? h : nullptr, rec);
            std::memcpy(&out[i], rec, 16);
        }
}

// ------------------------------------------------------------------ the variance image and the filter: what they share
bool desc_ok(const yk_variance_desc* d) {
    if (!d || d->iterations > DN_MAX_ITERATIONS) return false;
    if (!(d->sigma_variance > 0.0f) || !(d->sigma_normal > 0.0f) || !(d->sigma_plane > 0.0f)) return false;  // <= 0 or NaN
    if (!(d->epsilon >= 0.0f) || !(d->spatial_scale >= 0.0f)) return false;                                  // < 0 or NaN
    return true;
}

VrParams make_params(const yk_variance_desc* d, uint16_t res_x, uint16_t res_y, uint16_t tile_dim) {
    VrParams a{};
    dn_set_grid(a.dn, res_x, res_y, tile_dim);
    a.dn.sigma_color = 0.0f;
    a.dn.den_n = d->sigma_normal * d->sigma_normal;
    a.dn.den_p = d->sigma_plane * d->sigma_plane;
    a.sv2 = d->sigma_variance * d->sigma_variance;
    a.epsilon = d->epsilon;
    a.spatial_scale = d->spatial_scale;
    return a;
}

// ------------------------------------------------------------------ yk_variance
struct VrVarIo {
    const float4* moments;  // may be NULL
    const float* film;
    const uint32_t* samples;  // may be NULL
    const float4* guides;
    const float4* albedo;  // may be NULL
    float* out;
};

__global__ __launch_bounds__(VR_TX* VR_TY) void k_variance(VrVarIo io, VrParams a) {
    constexpr int H = 3, W = (int)VR_TX + 2 * H, ROWS = (int)VR_TY + 2 * H;
    __shared__ float4 lds_a[W * ROWS], lds_b[W * ROWS];
    const uint32_t x0 = blockIdx.x * VR_TX, y0 = blockIdx.y * VR_TY;
    const uint32_t x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inside = x < a.dn.res_x && y < a.dn.res_y;
    const size_t i = inside ? (size_t)y * a.dn.res_x + x : (size_t)0;  // a lane outside the film asks for pixel 0 and drops it
    float var = 0.0f;
    bool have = false;
    if (io.moments) {
        const float4 mv = io.moments[i];
        const float h[4] = {mv.x, mv.y, mv.z, mv.w};
        if (io.albedo) {
            const float4 al = io.albedo[i];
            const float alb[3] = {al.x, al.y, al.z};
            have = vr_temporal(h, alb, var);
        } else {
            have = vr_temporal(h, nullptr, var);
        }
    }
    const int need = inside && !have;
    if (!__syncthreads_or(need)) {  // block-uniform: no lane of this tile needs the window
        if (inside) io.out[i] = vr_sanitise(var);
        return;
    }
    const int bx = (int)x0 - H, by = (int)y0 - H;
    for (int k = (int)(threadIdx.y * VR_TX + threadIdx.x); k < W * ROWS; k += (int)(VR_TX * VR_TY)) {
        const int gx = bx + k % W, gy = by + k / W;
        if (gx < 0 || gy < 0 || gx >= (int)a.dn.res_x || gy >= (int)a.dn.res_y) continue;  // never read: taps outside the film are skipped
        const size_t q = (size_t)gy * a.dn.res_x + (size_t)gx;
        const float l = vr_tap_luminance(a.dn, io.film, io.samples, reinterpret_cast<const float*>(io.albedo), (uint32_t)gx, (uint32_t)gy);
        const float4 gb = io.guides[2 * q + 1];
        lds_a[k] = io.guides[2 * q];
        lds_b[k] = make_float4(gb.x, gb.y, gb.z, l);
    }
    __syncthreads();
    if (!inside) return;
    if (need) {
        var = vr_spatial_pixel(a, x, y, [&](uint32_t qx, uint32_t qy, VrTap& t) {
            const int k = ((int)qy - by) * W + ((int)qx - bx);
            const float4 ga = lds_a[k], gb = lds_b[k];
            t.ns[0] = ga.x;
            t.ns[1] = ga.y;
            t.ns[2] = ga.z;
            t.hit = ga.w;
            t.p[0] = gb.x;
            t.p[1] = gb.y;
            t.p[2] = gb.z;
            t.l = gb.w;
        });
    }
    io.out[i] = vr_sanitise(var);
}

yk_status check_variance(const yk_variance_desc* d, const void* moments, const void* film, const void* guides, bool has_albedo, const void* albedo, uint16_t res_x, uint16_t res_y,
                         uint16_t tile_dim, const void* out) {
    if (!desc_ok(d) || !film || !guides || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * 4, film, n_px * 12) || overlaps(out, n_px * 4, guides, n_px * sizeof(yk_guide))) return YK_ERR_INVALID_ARGUMENT;
    if (moments && overlaps(out, n_px * 4, moments, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
    if (has_albedo && albedo && overlaps(out, n_px * 4, albedo, n_px * sizeof(yk_albedo))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue_variance(yk_context* ctx, hipStream_t st, const yk_variance_desc* d, const void* moments, const float* film, const void* guides, const void* albedo, uint16_t res_x,
                           uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out) {
    const VrParams a = make_params(d, res_x, res_y, tile_dim);
    VrVarIo io{};
    io.moments = reinterpret_cast<const float4*>(moments);
    io.film = film;
    io.guides = reinterpret_cast<const float4*>(guides);
    io.albedo = reinterpret_cast<const float4*>(albedo);
    io.out = out;
    if (samples) {
        yk_status ss = stage_sample_table(ctx, st, samples, res_x, res_y, tile_dim, ctx->denoise.samples);
        if (ss != YK_OK) return ss;
        io.samples = ctx->denoise.samples.as<const uint32_t>();
    }
    const dim3 grid((res_x + VR_TX - 1) / VR_TX, (res_y + VR_TY - 1) / VR_TY), block(VR_TX, VR_TY);
    hipLaunchKernelGGL(k_variance, grid, block, 0, st, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void load_guide(const yk_guide& g, float* ns, float& hit, float* p) {
    std::memcpy(ns, g.ns, 12);
    hit = g.hit;
    std::memcpy(p, g.p, 12);
}

void variance_host(const yk_variance_desc* d, const yk_moments* moments, const float* film, const yk_guide* guides, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y,
                   uint16_t tile_dim, const uint32_t* samples, float* out) {
    const VrParams a = make_params(d, res_x, res_y, tile_dim);
    const size_t n_px = (size_t)res_x * res_y;
    const float* alb = reinterpret_cast<const float*>(albedo);
    std::vector<float> lum(n_px);  // every tap's luminance once: the window reads each 49 times
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) lum[(size_t)y * res_x + x] = vr_tap_luminance(a.dn, film, samples, alb, x, y);
    const auto fetch = [&](uint32_t qx, uint32_t qy, VrTap& t) {
        const size_t q = (size_t)qy * res_x + qx;
        load_guide(guides[q], t.ns, t.hit, t.p);
        t.l = lum[q];
    };
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            float var = 0.0f, h[4];
            if (moments) std::memcpy(h, &moments[i], 16);
            if (!vr_temporal(moments ? h : nullptr, albedo ? albedo[i].a : nullptr, var)) var = vr_spatial_pixel(a, x, y, fetch);
            out[i] = vr_sanitise(var);
        }
}

// ------------------------------------------------------------------ yk_denoise_variance
struct VrIo {
    const float* film;        // the preparing pass: the RGB film ...
    const uint32_t* samples;  // ... its sample table (may be NULL) ...
    const float* variance;    // ... and its variance image
    const float4* in;         // the iterations: the previous iteration's (r, g, b, var) records
    const float4* guides;
    const float4* albedo;  // may be NULL
    float4* out;           // records, or ...
    float* out_rgb;        // ... the last iteration's RGB
};

__device__ __forceinline__ void vr_load_film(const VrParams& a, const VrIo& io, uint32_t i, float* c) {
    const uint32_t y = i / a.dn.res_x, x = i - y * a.dn.res_x;
    c[0] = io.film[3 * (size_t)i];
    c[1] = io.film[3 * (size_t)i + 1];
    c[2] = io.film[3 * (size_t)i + 2];
    dn_normalise(dn_count(a.dn, io.samples, x, y), c);
}

__global__ __launch_bounds__(256) void k_vprep(VrIo io, VrParams a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.dn.res_x * a.dn.res_y) return;
    float c[3];
    vr_load_film(a, io, i, c);
    if (io.albedo) {
        const float4 al = io.albedo[i];
        const float alb[3] = {al.x, al.y, al.z};
        al_demodulate(alb, c);
    }
    io.out[i] = make_float4(c[0], c[1], c[2], vr_sanitise(io.variance[i]));
}

// iterations == 0 with a sample table: the normalised film as RGB (out_rgb may be the film: a lane reads its pixel before it
// writes it and touches no other)
__global__ __launch_bounds__(256) void k_vnormalise(VrIo io, VrParams a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.dn.res_x * a.dn.res_y) return;
    float c[3];
    vr_load_film(a, io, i, c);
    io.out_rgb[3 * (size_t)i] = c[0];
    io.out_rgb[3 * (size_t)i + 1] = c[1];
    io.out_rgb[3 * (size_t)i + 2] = c[2];
}

__device__ __forceinline__ void vr_set_tap(VrFilterTap& t, float4 c, float4 ga, float4 gb) {
    t.t.c[0] = c.x;
    t.t.c[1] = c.y;
    t.t.c[2] = c.z;
    t.var = c.w;
    t.t.ns[0] = ga.x;
    t.t.ns[1] = ga.y;
    t.t.ns[2] = ga.z;
    t.t.hit = ga.w;
    t.t.p[0] = gb.x;
    t.t.p[1] = gb.y;
    t.t.p[2] = gb.z;
}

// The records, the guides, the albedo and the output of one launch never overlap (enqueue sees to it).
template <int S, bool LAST>
__global__ __launch_bounds__(VR_TX* VR_TY) void k_atrous_var(VrIo io, VrParams a, int step) {
    const uint32_t x0 = blockIdx.x * VR_TX, y0 = blockIdx.y * VR_TY;
    const uint32_t x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    const bool inside = x < a.dn.res_x && y < a.dn.res_y;
    float rec[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (S == 0) {
        if (!inside) return;
        vr_pixel(
            a, step, x, y,
            [&](uint32_t qx, uint32_t qy, VrFilterTap& t) {
                const size_t q = (size_t)qy * a.dn.res_x + qx;
                vr_set_tap(t, io.in[q], io.guides[2 * q], io.guides[2 * q + 1]);
            },
            [&](uint32_t qx, uint32_t qy) { return reinterpret_cast<const float*>(io.in)[4 * ((size_t)qy * a.dn.res_x + qx) + 3]; }, rec);
    } else {
        constexpr int H = 2 * S, W = (int)VR_TX + 2 * H, ROWS = (int)VR_TY + 2 * H;
        __shared__ float4 lds_c[W * ROWS], lds_a[W * ROWS], lds_b[W * ROWS];
        const int bx = (int)x0 - H, by = (int)y0 - H;
        for (int k = (int)(threadIdx.y * VR_TX + threadIdx.x); k < W * ROWS; k += (int)(VR_TX * VR_TY)) {
            const int gx = bx + k % W, gy = by + k / W;
            if (gx < 0 || gy < 0 || gx >= (int)a.dn.res_x || gy >= (int)a.dn.res_y) continue;  // never read: taps outside the film are skipped
            const size_t q = (size_t)gy * a.dn.res_x + (size_t)gx;
            lds_c[k] = io.in[q];
            lds_a[k] = io.guides[2 * q];
            lds_b[k] = io.guides[2 * q + 1];
        }
        __syncthreads();
        if (!inside) return;
        vr_pixel(
            a, S, x, y,
            [&](uint32_t qx, uint32_t qy, VrFilterTap& t) {
                const int k = ((int)qy - by) * W + ((int)qx - bx);
                vr_set_tap(t, lds_c[k], lds_a[k], lds_b[k]);
            },
            [&](uint32_t qx, uint32_t qy) { return lds_c[((int)qy - by) * W + ((int)qx - bx)].w; }, rec);
    }
    const size_t i = (size_t)y * a.dn.res_x + x;
    if (LAST) {
        if (io.albedo) {
            const float4 al = io.albedo[i];
            const float alb[3] = {al.x, al.y, al.z};
            al_remodulate(alb, rec);
        }
        io.out_rgb[3 * i] = rec[0];
        io.out_rgb[3 * i + 1] = rec[1];
        io.out_rgb[3 * i + 2] = rec[2];
    } else {
        io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
    }
}

template <bool LAST>
void launch_atrous_var(hipStream_t st, int variant, const VrIo& io, const VrParams& a, int step) {
    const dim3 grid((a.dn.res_x + VR_TX - 1) / VR_TX, (a.dn.res_y + VR_TY - 1) / VR_TY), block(VR_TX, VR_TY);
    if (variant == 1) hipLaunchKernelGGL((k_atrous_var<1, LAST>), grid, block, 0, st, io, a, step);
    else if (variant == 2) hipLaunchKernelGGL((k_atrous_var<2, LAST>), grid, block, 0, st, io, a, step);
    else hipLaunchKernelGGL((k_atrous_var<0, LAST>), grid, block, 0, st, io, a, step);
}

// yk_denoise's check_call with the variance as one more input
yk_status check_filter(const yk_variance_desc* d, const void* film, const void* guides, const void* variance, bool has_albedo, const void* albedo, uint16_t res_x, uint16_t res_y,
                       uint16_t tile_dim, const void* out) {
    if (!desc_ok(d) || !film || !guides || !variance || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(guides, n_px * sizeof(yk_guide), out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (overlaps(variance, n_px * 4, out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (out != film && overlaps(film, n_px * 12, out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (has_albedo && albedo && overlaps(albedo, n_px * sizeof(yk_albedo), out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue_filter(yk_context* ctx, hipStream_t st, const yk_variance_desc* d, const float* film, const void* guides, const float* variance, const void* albedo, uint16_t res_x,
                         uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out) {
    const uint32_t n_px = (uint32_t)res_x * res_y;
    auto& dn = ctx->denoise;
    const VrParams a = make_params(d, res_x, res_y, tile_dim);
    VrIo io{};
    io.film = film;
    io.variance = variance;
    io.guides = reinterpret_cast<const float4*>(guides);
    if (samples) {
        yk_status ss = stage_sample_table(ctx, st, samples, res_x, res_y, tile_dim, dn.samples);
        if (ss != YK_OK) return ss;
        io.samples = dn.samples.as<const uint32_t>();
    }
    const uint32_t n_it = d->iterations;
    if (n_it == 0) {  // the normalised film's bits: no division, no product
        if (samples) {
            io.out_rgb = out;
            hipLaunchKernelGGL(k_vnormalise, dim3((n_px - 1) / 256 + 1), dim3(256), 0, st, io, a);
        } else if (film != out) {
            HIP_TRY(ctx, hipMemcpyAsync(out, film, (size_t)n_px * 12, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(ctx, hipGetLastError());
        return YK_OK;
    }
    io.albedo = reinterpret_cast<const float4*>(albedo);
    HIP_TRY(ctx, dn.ping[0].ensure((size_t)n_px * 16));
    if (n_it > 1) HIP_TRY(ctx, dn.ping[1].ensure((size_t)n_px * 16));
    io.out = dn.ping[0].as<float4>();
    hipLaunchKernelGGL(k_vprep, dim3((n_px - 1) / 256 + 1), dim3(256), 0, st, io, a);
    int src = 0;
    for (uint32_t i = 0; i < n_it; ++i) {
        const int step = 1 << i;
        const int variant = step <= (int)dn.lds_max_step ? step : 0;
        const int dst = src == 0 ? 1 : 0;
        io.in = dn.ping[src].as<const float4>();
        if (i + 1 < n_it) {
            io.out = dn.ping[dst].as<float4>();
            io.out_rgb = nullptr;
            launch_atrous_var<false>(st, variant, io, a, step);
        } else {
            io.out = nullptr;
            io.out_rgb = out;
            launch_atrous_var<true>(st, variant, io, a, step);
        }
        src = dst;
    }
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void filter_host(const yk_variance_desc* d, const float* film, const yk_guide* guides, const float* variance, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y,
                 uint16_t tile_dim, const uint32_t* samples, float* out) {
    const VrParams a = make_params(d, res_x, res_y, tile_dim);
    const size_t n_px = (size_t)res_x * res_y;
    if (d->iterations == 0) albedo = nullptr;
    std::vector<float> cur(4 * n_px), nxt(d->iterations ? 4 * n_px : 0);
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            std::memcpy(&cur[4 * i], film + 3 * i, 12);
            dn_normalise(dn_count(a.dn, samples, x, y), &cur[4 * i]);
            if (albedo) al_demodulate(albedo[i].a, &cur[4 * i]);
            cur[4 * i + 3] = vr_sanitise(variance[i]);
        }
    for (uint32_t it = 0; it < d->iterations; ++it) {
        const auto fetch = [&](uint32_t qx, uint32_t qy, VrFilterTap& t) {
            const size_t q = (size_t)qy * res_x + qx;
            std::memcpy(t.t.c, &cur[4 * q], 12);
            t.var = cur[4 * q + 3];
            load_guide(guides[q], t.t.ns, t.t.hit, t.t.p);
        };
        const auto fetch_var = [&](uint32_t qx, uint32_t qy) { return cur[4 * ((size_t)qy * res_x + qx) + 3]; };
        for (uint32_t y = 0; y < res_y; ++y)
            for (uint32_t x = 0; x < res_x; ++x) vr_pixel(a, 1 << it, x, y, fetch, fetch_var, &nxt[4 * ((size_t)y * res_x + x)]);
        cur.swap(nxt);
    }
    for (size_t i = 0; i < n_px; ++i) {
        if (albedo) al_remodulate(albedo[i].a, &cur[4 * i]);
        std::memcpy(out + 3 * i, &cur[4 * i], 12);
    }
}

}  // namespace

extern "C" {

yk_status yk_moments_blend(yk_context* ctx, const yk_temporal_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                           const yk_moments* moments, yk_moments* out_moments) try {
    if (check_blend(desc, film_rgb, res_x, res_y, tile_dim, moments, out_moments) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend: bad argument");
    if (!ctx) {  // the host instance
        blend_host(desc, film_rgb, res_x, res_y, tile_dim, samples, moments, out_moments);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_moments* d_moments = moments ? sg.upload(moments, n_px) : nullptr;
    yk_moments* d_out = sg.output(out_moments, n_px);
    if (!sg.ok()) return sg.status();
    yk_status s = enqueue_blend(ctx, sg.stream, desc, d_film, res_x, res_y, tile_dim, samples, d_moments, d_out);
    if (s != YK_OK) return s;
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_moments_blend_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                  const void* d_moments, void* d_out_moments, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_blend(desc, d_film_rgb, res_x, res_y, tile_dim, d_moments, d_out_moments) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend_device: bad argument");
    // dword loads of the film, 16-byte loads and stores of the records
    if (misaligned(4, d_film_rgb) || misaligned(16, d_moments, d_out_moments))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend_device: film must be 4-byte aligned, moments 16-byte aligned");
    return enqueue_blend(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, d_moments, d_out_moments);
}

yk_status yk_variance(yk_context* ctx, const yk_variance_desc* desc, const yk_moments* moments, const float* film_rgb, const yk_guide* guides, const yk_albedo* albedo, uint16_t res_x,
                      uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_variance) try {
    if (check_variance(desc, moments, film_rgb, guides, true, albedo, res_x, res_y, tile_dim, out_variance) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_variance: bad argument");
    if (!ctx) {  // the host instance
        variance_host(desc, moments, film_rgb, guides, albedo, res_x, res_y, tile_dim, samples, out_variance);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const yk_moments* d_moments = moments ? sg.upload(moments, n_px) : nullptr;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const yk_albedo* d_albedo = albedo ? sg.upload(albedo, n_px) : nullptr;
    float* d_out = sg.output(out_variance, n_px);
    if (!sg.ok()) return sg.status();
    yk_status s = enqueue_variance(ctx, sg.stream, desc, d_moments, d_film, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out);
    if (s != YK_OK) return s;
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_variance_device(yk_context* ctx, const yk_variance_desc* desc, const void* d_moments, const void* d_film_rgb, const void* d_guides, const void* d_albedo, uint16_t res_x,
                             uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_variance, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_variance(desc, d_moments, d_film_rgb, d_guides, true, d_albedo, res_x, res_y, tile_dim, d_out_variance) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_variance_device: bad argument");
    // dword loads of the film and dword stores of the variance, 16-byte loads of the moments, the guides and the albedo
    if (misaligned(4, d_film_rgb, d_out_variance) || misaligned(16, d_moments, d_guides, d_albedo))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_variance_device: film and variance must be 4-byte aligned, moments, guides and albedo 16-byte aligned");
    return enqueue_variance(ctx, device_call_stream(ctx, stream), desc, d_moments, reinterpret_cast<const float*>(d_film_rgb), d_guides, d_albedo, res_x, res_y, tile_dim, samples,
                            reinterpret_cast<float*>(d_out_variance));
}

yk_status yk_denoise_variance(yk_context* ctx, const yk_variance_desc* desc, const float* film_rgb, const yk_guide* guides, const float* variance, const yk_albedo* albedo,
                              uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb) try {
    if (check_filter(desc, film_rgb, guides, variance, true, albedo, res_x, res_y, tile_dim, out_rgb) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance: bad argument");
    if (!ctx) {  // the host instance
        filter_host(desc, film_rgb, guides, variance, albedo, res_x, res_y, tile_dim, samples, out_rgb);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const float* d_variance = sg.upload(variance, n_px);
    const yk_albedo* d_albedo = albedo ? sg.upload(albedo, n_px) : nullptr;
    float* d_out = sg.output(out_rgb, n_px * 3);
    if (!sg.ok()) return sg.status();
    yk_status s = enqueue_filter(ctx, sg.stream, desc, d_film, d_guides, d_variance, d_albedo, res_x, res_y, tile_dim, samples, d_out);
    if (s != YK_OK) return s;
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_denoise_variance_device(yk_context* ctx, const yk_variance_desc* desc, const void* d_film_rgb, const void* d_guides, const void* d_variance, const void* d_albedo,
                                     uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_filter(desc, d_film_rgb, d_guides, d_variance, true, d_albedo, res_x, res_y, tile_dim, d_out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance_device: bad argument");
    // dword loads and stores of the film, the variance and the output, 16-byte loads of the guides and the albedo
    if (misaligned(4, d_film_rgb, d_variance, d_out_rgb) || misaligned(16, d_guides, d_albedo))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance_device: film, variance and output must be 4-byte aligned, guides and albedo 16-byte aligned");
    return enqueue_filter(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), d_guides, reinterpret_cast<const float*>(d_variance), d_albedo, res_x, res_y,
                          tile_dim, samples, reinterpret_cast<float*>(d_out_rgb));
}

}  // extern "C"
