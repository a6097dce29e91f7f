// yk_rectify.hip — history rectification on gfx950, behind yk_history_rectify[_device]; the per-pixel arithmetic is
// yk_rectify.h's, whose host instance these entry points run without a context.
//
// k_rectify: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h).  A lane reads its history record and,
//   with moments, its moments record (one 16-byte load each, both requested before either is looked at).  Whether the block
//   looks at the film at all is decided once per block (__syncthreads_or over "this lane has a history"): before the first
//   blend, and wherever reprojection found nothing, no block does.  A block that does stages the taps of its tile plus a
//   halo of `radius` in LDS — one float4 (r, g, b, m) an entry, normalised as the blend normalises them: three dword loads
//   of the film and, with a table, one of the staged sample table — and every lane with a history walks its window out of
//   LDS twice (mean, then variance).  A wave reads two rows of 32 consecutive 16-byte entries with each ds_read_b128: every
//   16-lane group of that instruction gets 16 different 16-byte slots of the 256-byte bank row, so the walk has no bank
//   conflicts at any window offset.  The radius is a template parameter (FilmTile<1..3>, both window loops unrolled); a
//   build with -DYK_RECTIFY_ONE_INSTANCE has one instance with halo 3 and a run-time radius instead, for the timing that
//   chose between them.
// The staged sample table is the temporal pass's (ctx->temporal.samples): the call is ordered on one stream with the blends
// and never runs beside them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_rectify.h"
#include "yk_staging.h"

namespace {

struct RcIo {
    const float* film;
    const uint32_t* samples;  // may be NULL
    const float4* history;
    const float4* moments;  // may be NULL, with out_moments
    float4* out_history;
    float4* out_moments;
};

// RADIUS > 0: the window's radius, and the halo; RADIUS == 0: a.radius at run time under a halo of RC_MAX_RADIUS
template <int RADIUS>
__global__ __launch_bounds__(FT_TX* FT_TY) void k_rectify(RcIo io, RcParams a) {
    using Tile = FilmTile<(RADIUS > 0 ? RADIUS : (int)RC_MAX_RADIUS)>;
    __shared__ float4 lds[Tile::N];
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    const bool inside = x < a.dn.res_x && y < a.dn.res_y;
    const size_t i = inside ? (size_t)y * a.dn.res_x + x : (size_t)0;  // a lane outside the film asks for pixel 0 and drops it
    const float4 hv = io.history[i];
    float4 mv = hv;
    if (io.moments) mv = io.moments[i];
    const float h[4] = {hv.x, hv.y, hv.z, hv.w};
    if (!__syncthreads_or(inside && rc_present(h))) {  // block-uniform: no lane of this tile has a history to clip
        if (inside) {
            io.out_history[i] = hv;
            if (io.moments) io.out_moments[i] = mv;
        }
        return;
    }
    const Tile tile;
    tile.stage(a.dn.res_x, a.dn.res_y, [&](int k, uint32_t gx, uint32_t gy) {
        float t[4];
        rc_tap(a.dn, io.film, io.samples, gx, gy, t);
        lds[k] = make_float4(t[0], t[1], t[2], t[3]);
    });
    if (!inside) return;
    float out[4], f;
    const bool clipped = rc_pixel<RADIUS>(
        a, x, y, h,
        [&](uint32_t qx, uint32_t qy, float* t) {
            const float4 v = lds[tile.index(qx, qy)];
            t[0] = v.x;
            t[1] = v.y;
            t[2] = v.z;
            t[3] = v.w;
        },
        out, f);
    io.out_history[i] = make_float4(out[0], out[1], out[2], out[3]);
    if (io.moments) {
        const float m[4] = {mv.x, mv.y, mv.z, mv.w};
        float mo[4] = {mv.x, mv.y, mv.z, mv.w};
        if (clipped) rc_moments(m, f, out[3], mo);
        io.out_moments[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
    }
}

// history and out_history are required, the moments come in a pair; an output may BE its own input and overlaps nothing else
yk_status check_rectify(const yk_rectify_desc* d, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* history, const void* moments, const void* out_history,
                        const void* out_moments) {
    if (!rc_desc_ok(d) || !film || !history || !out_history || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    if ((moments == nullptr) != (out_moments == nullptr)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y, rec = n_px * 16;
    if (overlaps(out_history, rec, film, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (out_history != history && overlaps(out_history, rec, history, rec)) return YK_ERR_INVALID_ARGUMENT;
    if (moments) {
        if (overlaps(out_history, rec, moments, rec) || overlaps(out_history, rec, out_moments, rec)) return YK_ERR_INVALID_ARGUMENT;
        if (overlaps(out_moments, rec, film, n_px * 12) || overlaps(out_moments, rec, history, rec)) return YK_ERR_INVALID_ARGUMENT;
        if (out_moments != moments && overlaps(out_moments, rec, moments, rec)) return YK_ERR_INVALID_ARGUMENT;
    }
    return YK_OK;
}

yk_status enqueue_rectify(yk_context* ctx, hipStream_t st, const yk_rectify_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                          const void* history, const void* moments, void* out_history, void* out_moments) {
    const RcParams a = rc_make_params(d, res_x, res_y, tile_dim);
    RcIo io{film, nullptr, reinterpret_cast<const float4*>(history), reinterpret_cast<const float4*>(moments), reinterpret_cast<float4*>(out_history), reinterpret_cast<float4*>(out_moments)};
    if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, ctx->temporal.samples, &io.samples)) return ss;
    const dim3 grid = ft_grid(res_x, res_y), block = ft_block();
#ifdef YK_RECTIFY_ONE_INSTANCE
    hipLaunchKernelGGL(k_rectify<0>, grid, block, 0, st, io, a);
#else
    if (a.radius == 1) hipLaunchKernelGGL(k_rectify<1>, grid, block, 0, st, io, a);
    else if (a.radius == 2) hipLaunchKernelGGL(k_rectify<2>, grid, block, 0, st, io, a);
    else hipLaunchKernelGGL(k_rectify<3>, grid, block, 0, st, io, a);
#endif
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void rectify_host(const yk_rectify_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const yk_history* history, const yk_moments* moments,
                  yk_history* out_history, yk_moments* out_moments) {
    const RcParams a = rc_make_params(d, res_x, res_y, tile_dim);
    const size_t n_px = (size_t)res_x * res_y;
    std::vector<float> taps(4 * n_px);  // every pixel's tap once: the windows read each up to 2 * 49 times
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) rc_tap(a.dn, film, samples, x, y, &taps[4 * ((size_t)y * res_x + x)]);
    const auto fetch = [&](uint32_t qx, uint32_t qy, float* t) { std::memcpy(t, &taps[4 * ((size_t)qy * res_x + qx)], 16); };
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            float h[4], out[4], f;
            std::memcpy(h, &history[i], 16);
            const bool clipped = rc_pixel<0>(a, x, y, h, fetch, out, f);
            if (moments) {
                float m[4], mo[4];
                std::memcpy(m, &moments[i], 16);
                std::memcpy(mo, m, 16);
                if (clipped) rc_moments(m, f, out[3], mo);
                std::memcpy(&out_moments[i], mo, 16);
            }
            std::memcpy(&out_history[i], out, 16);
        }
}

}  // namespace

extern "C" {

yk_status yk_history_rectify(yk_context* ctx, const yk_rectify_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                             const yk_history* history, const yk_moments* moments, yk_history* out_history, yk_moments* out_moments) try {
    if (check_rectify(desc, film_rgb, res_x, res_y, tile_dim, history, moments, out_history, out_moments) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_rectify: bad argument");
    if (!ctx) {  // the host instance
        rectify_host(desc, film_rgb, res_x, res_y, tile_dim, samples, history, moments, out_history, out_moments);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_history* d_history = sg.upload(history, n_px);
    const yk_moments* d_moments = moments ? sg.upload(moments, n_px) : nullptr;
    yk_history* d_out_history = sg.output(out_history, n_px);
    yk_moments* d_out_moments = sg.output(out_moments, n_px);  // NULL with the moments: no slot
    return sg.run([&] { return enqueue_rectify(ctx, sg.stream, desc, d_film, res_x, res_y, tile_dim, samples, d_history, d_moments, d_out_history, d_out_moments); });
}
YK_CATCH(ctx)

yk_status yk_history_rectify_device(yk_context* ctx, const yk_rectify_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                    const void* d_history, const void* d_moments, void* d_out_history, void* d_out_moments, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_rectify(desc, d_film_rgb, res_x, res_y, tile_dim, d_history, d_moments, d_out_history, d_out_moments) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_rectify_device: bad argument");
    // dword loads of the film, 16-byte loads and stores of the records
    if (misaligned(4, d_film_rgb) || misaligned(16, d_history, d_moments, d_out_history, d_out_moments))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_rectify_device: film must be 4-byte aligned, histories and moments 16-byte aligned");
    return enqueue_rectify(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, d_history, d_moments, d_out_history,
                           d_out_moments);
}

}  // extern "C"
