// yk_variance.hip — what the variance-guided denoise filters by, on gfx950: the carried luminance moments and the variance
// image, behind yk_moments_blend and yk_variance and their _device forms; the per-pixel arithmetic is yk_variance.h's,
// whose host instance these entry points run without a context.  The filter itself, yk_denoise_variance, is one more
// instance of the à-trous kernel and lives with it in yk_denoise.hip.
//
// yk_moments_blend has no kernel of its own: it is the record blend of yk_temporal.hip (k_record_blend, reached through
//   yk_film_call.h) with vr_moments_pixel as its pixel rule, records out and no RGB output.  The output may be the input
//   moments.
// k_variance: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h).  The temporal estimate is one 16-byte load
//   (two with an albedo) and a handful of VALU operations.  Whether the block evaluates the 7 x 7 window at all is decided
//   once per block (__syncthreads_or over "this lane has no temporal estimate"): after the first frames nearly no block
//   does.  A block that does stages the guides and the luminance of its tile plus a halo of 3 in LDS (38 x 14 records of two
//   float4: (ns, hit) and (p, l) — the luminance rides in the slot of the guide's unused t) and only the lanes that need
//   the window walk it.
// The staged sample table of yk_variance is the denoiser's (ctx->denoise), the blend's the temporal pass's: the calls are
// ordered on one stream with those passes and never run beside them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_staging.h"
#include "yk_variance.h"

namespace {

// ------------------------------------------------------------------ yk_variance
struct VrVarIo {
    const float4* moments;  // may be NULL
    const float* film;
    const uint32_t* samples;  // may be NULL
    const float4* guides;
    const float4* albedo;  // may be NULL
    float* out;
};

__global__ __launch_bounds__(FT_TX* FT_TY) void k_variance(VrVarIo io, VrParams a) {
    using Tile = FilmTile<3>;
    __shared__ float4 lds_a[Tile::N], lds_b[Tile::N];
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
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
    const Tile tile;
    tile.stage(a.dn.res_x, a.dn.res_y, [&](int k, uint32_t gx, uint32_t gy) {
        const size_t q = (size_t)gy * a.dn.res_x + gx;
        const float l = vr_tap_luminance(a.dn, io.film, io.samples, reinterpret_cast<const float*>(io.albedo), gx, gy);
        const float4 gb = io.guides[2 * q + 1];
        lds_a[k] = io.guides[2 * q];
        lds_b[k] = make_float4(gb.x, gb.y, gb.z, l);
    });
    if (!inside) return;
    if (need) {
        var = vr_spatial_pixel(a, x, y, [&](uint32_t qx, uint32_t qy, VrTap& t) {
            const int k = tile.index(qx, qy);
            const float4 ga = lds_a[k], gb = lds_b[k];
            dn_guide(&ga.x, &gb.x, t.ns, t.hit, t.p);
            t.l = gb.w;
        });
    }
    io.out[i] = vr_sanitise(var);
}

yk_status check_variance(const yk_variance_desc* d, const void* moments, const void* film, const void* guides, bool has_albedo, const void* albedo, uint16_t res_x, uint16_t res_y,
                         uint16_t tile_dim, const void* out) {
    if (!vr_desc_ok(d) || !film || !guides || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * 4, film, n_px * 12) || overlaps(out, n_px * 4, guides, n_px * sizeof(yk_guide))) return YK_ERR_INVALID_ARGUMENT;
    if (moments && overlaps(out, n_px * 4, moments, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
    if (has_albedo && albedo && overlaps(out, n_px * 4, albedo, n_px * sizeof(yk_albedo))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue_variance(yk_context* ctx, hipStream_t st, const yk_variance_desc* d, const void* moments, const float* film, const void* guides, const void* albedo, uint16_t res_x,
                           uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out) {
    const VrParams a = vr_make_params(d, res_x, res_y, tile_dim);
    VrVarIo io{};
    io.moments = reinterpret_cast<const float4*>(moments);
    io.film = film;
    io.guides = reinterpret_cast<const float4*>(guides);
    io.albedo = reinterpret_cast<const float4*>(albedo);
    io.out = out;
    if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, ctx->denoise.samples, &io.samples)) return ss;
    hipLaunchKernelGGL(k_variance, ft_grid(res_x, res_y), ft_block(), 0, st, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void variance_host(const yk_variance_desc* d, const yk_moments* moments, const float* film, const yk_guide* guides, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y,
                   uint16_t tile_dim, const uint32_t* samples, float* out) {
    const VrParams a = vr_make_params(d, res_x, res_y, tile_dim);
    const size_t n_px = (size_t)res_x * res_y;
    const float* alb = reinterpret_cast<const float*>(albedo);
    std::vector<float> lum(n_px);  // every tap's luminance once: the window reads each 49 times
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) lum[(size_t)y * res_x + x] = vr_tap_luminance(a.dn, film, samples, alb, x, y);
    const auto fetch = [&](uint32_t qx, uint32_t qy, VrTap& t) {
        const size_t q = (size_t)qy * res_x + qx;
        dn_guide(guides[q].ns, guides[q].p, t.ns, t.hit, t.p);
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

}  // namespace

extern "C" {

yk_status yk_moments_blend(yk_context* ctx, const yk_temporal_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                           const yk_moments* moments, yk_moments* out_moments) try {
    if (record_blend_check(desc, film_rgb, res_x, res_y, tile_dim, moments, out_moments, nullptr) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend: bad argument");
    if (!ctx) {  // the host instance
        record_blend_host(BlendRule::MOMENTS, desc, film_rgb, res_x, res_y, tile_dim, samples, moments, out_moments, nullptr);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_moments* d_moments = moments ? sg.upload(moments, n_px) : nullptr;
    yk_moments* d_out = sg.output(out_moments, n_px);
    return sg.run([&] { return record_blend_enqueue(ctx, sg.stream, BlendRule::MOMENTS, desc, d_film, res_x, res_y, tile_dim, samples, d_moments, d_out, nullptr); });
}
YK_CATCH(ctx)

yk_status yk_moments_blend_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                  const void* d_moments, void* d_out_moments, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (record_blend_check(desc, d_film_rgb, res_x, res_y, tile_dim, d_moments, d_out_moments, nullptr) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend_device: bad argument");
    // dword loads of the film, 16-byte loads and stores of the records
    if (misaligned(4, d_film_rgb) || misaligned(16, d_moments, d_out_moments))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_moments_blend_device: film must be 4-byte aligned, moments 16-byte aligned");
    return record_blend_enqueue(ctx, device_call_stream(ctx, stream), BlendRule::MOMENTS, desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, d_moments, d_out_moments,
                                nullptr);
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
    return sg.run([&] { return enqueue_variance(ctx, sg.stream, desc, d_moments, d_film, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out); });
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

}  // extern "C"
