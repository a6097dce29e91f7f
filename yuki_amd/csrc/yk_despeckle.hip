// yk_despeckle.hip — the despeckle pass on gfx950, behind yk_despeckle[_device]; the per-pixel arithmetic is
// yk_despeckle.h's, whose host instance these entry points run without a context.
//
// k_despeckle: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h).  A lane asks for its own three
//   stored floats first (the output keeps their bits wherever the pixel is not touched, and a clamp scales them, not the
//   normalised colour), then the block stages the taps of its tile plus a halo of `radius` in LDS — one float4 (r, g, b, m)
//   an entry, as rc_tap reads a pixel: three dword loads of the film and, with a table, one of the staged sample table —
//   and every lane walks its window out of LDS ONCE: the four largest luminances sink through a compare-and-swap chain in
//   four registers, the count and the three sums for a repair are kept along the way.  A wave reads two rows of 32
//   consecutive 16-byte entries with each ds_read_b128, the conflict-free pattern of k_rectify.  The radius is a template
//   parameter (FilmTile<1..2>, the window loop unrolled).
//   Counts: a wave ballots "clamped" and "repaired", its first lane adds the two popcounts to two LDS words, and after the
//   block has met two lanes add a word each to the caller's two with a 32-bit integer atomic, and none where the word is
//   zero.  Every block adds to the same two addresses, and those atomics are what the counts cost.  No
//   floating-point atomics.
// The staged sample table is the temporal pass's (ctx->temporal.samples), as k_rectify's: the call is ordered on one
// stream with the rectification and the blends and never runs beside them.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_despeckle.h"
#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_staging.h"

namespace {

struct DsIo {
    const float* film;
    const uint32_t* samples;  // may be NULL
    float* out;
    uint8_t* mask;     // may be NULL
    uint32_t* counts;  // may be NULL; two words (clamped, repaired), cleared before the launch
};

template <int RADIUS>
__global__ __launch_bounds__(FT_TX* FT_TY) void k_despeckle(DsIo io, DsParams a) {
    using Tile = FilmTile<RADIUS>;
    __shared__ float4 lds[Tile::N];
    __shared__ uint32_t n_block[2];
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    const bool inside = x < a.dn.res_x && y < a.dn.res_y;
    const size_t i = inside ? (size_t)y * a.dn.res_x + x : (size_t)0;  // a lane outside the film asks for pixel 0 and drops it
    const float stored[3] = {io.film[3 * i], io.film[3 * i + 1], io.film[3 * i + 2]};
    if (io.counts && threadIdx.x < 2 && threadIdx.y == 0) n_block[threadIdx.x] = 0;
    const Tile tile;
    tile.stage(a.dn.res_x, a.dn.res_y, [&](int k, uint32_t gx, uint32_t gy) {
        float t[4];
        rc_tap(a.dn, io.film, io.samples, gx, gy, t);
        lds[k] = make_float4(t[0], t[1], t[2], t[3]);
    });
    uint8_t what = DS_UNTOUCHED;
    if (inside) {
        const float4 pv = lds[tile.index(x, y)];
        const float p[4] = {pv.x, pv.y, pv.z, pv.w};
        float out[3];
        what = ds_pixel<RADIUS>(
            a, io.samples != nullptr, x, y, stored, p,
            [&](uint32_t qx, uint32_t qy, float* t) {
                const float4 v = lds[tile.index(qx, qy)];
                t[0] = v.x;
                t[1] = v.y;
                t[2] = v.z;
                t[3] = v.w;
            },
            out);
        io.out[3 * i] = out[0];
        io.out[3 * i + 1] = out[1];
        io.out[3 * i + 2] = out[2];
        if (io.mask) io.mask[i] = what;
    }
    if (!io.counts) return;  // block-uniform
    const unsigned long long clamped = __ballot(what == DS_CLAMPED), repaired = __ballot(what == DS_REPAIRED);
    if (((threadIdx.y * FT_TX + threadIdx.x) & 63u) == 0) {
        if (clamped) atomicAdd(&n_block[0], (uint32_t)__popcll(clamped));
        if (repaired) atomicAdd(&n_block[1], (uint32_t)__popcll(repaired));
    }
    __syncthreads();
    if (threadIdx.x < 2 && threadIdx.y == 0 && n_block[threadIdx.x]) atomicAdd(&io.counts[threadIdx.x], n_block[threadIdx.x]);
}

// film and out_rgb are required and share no byte (a pixel reads its neighbours' input); mask and counts are optional and
// overlap nothing else
yk_status check_despeckle(const yk_despeckle_desc* d, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* out_rgb, const void* out_mask, const void* out_counts) {
    if (!ds_desc_ok(d) || !film || !out_rgb || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y, rgb = n_px * 12;
    if (overlaps(out_rgb, rgb, film, rgb)) return YK_ERR_INVALID_ARGUMENT;
    if (out_mask && (overlaps(out_mask, n_px, film, rgb) || overlaps(out_mask, n_px, out_rgb, rgb))) return YK_ERR_INVALID_ARGUMENT;
    if (out_counts) {
        if (overlaps(out_counts, 8, film, rgb) || overlaps(out_counts, 8, out_rgb, rgb)) return YK_ERR_INVALID_ARGUMENT;
        if (out_mask && overlaps(out_counts, 8, out_mask, n_px)) return YK_ERR_INVALID_ARGUMENT;
    }
    return YK_OK;
}

yk_status enqueue_despeckle(yk_context* ctx, hipStream_t st, const yk_despeckle_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb,
                            uint8_t* out_mask, uint32_t* out_counts) {
    const DsParams a = ds_make_params(d, res_x, res_y, tile_dim);
    DsIo io{film, nullptr, out_rgb, out_mask, out_counts};
    if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, ctx->temporal.samples, &io.samples)) return ss;
    if (out_counts) HIP_TRY(ctx, hipMemsetAsync(out_counts, 0, 8, st));
    const dim3 grid = ft_grid(res_x, res_y), block = ft_block();
    if (a.radius == 1) hipLaunchKernelGGL(k_despeckle<1>, grid, block, 0, st, io, a);
    else hipLaunchKernelGGL(k_despeckle<2>, grid, block, 0, st, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void despeckle_host(const yk_despeckle_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb, uint8_t* out_mask,
                    uint32_t* out_counts) {
    const DsParams a = ds_make_params(d, res_x, res_y, tile_dim);
    const size_t n_px = (size_t)res_x * res_y;
    std::vector<float> taps(4 * n_px);  // every pixel's tap once: the windows read each up to 24 times
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) rc_tap(a.dn, film, samples, x, y, &taps[4 * ((size_t)y * res_x + x)]);
    const auto fetch = [&](uint32_t qx, uint32_t qy, float* t) { std::memcpy(t, &taps[4 * ((size_t)qy * res_x + qx)], 16); };
    uint32_t counts[2] = {0, 0};
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            float stored[3], out[3];
            std::memcpy(stored, &film[3 * i], 12);
            const uint8_t what = ds_pixel<0>(a, samples != nullptr, x, y, stored, &taps[4 * i], fetch, out);
            std::memcpy(&out_rgb[3 * i], out, 12);
            if (out_mask) out_mask[i] = what;
            counts[0] += what == DS_CLAMPED;
            counts[1] += what == DS_REPAIRED;
        }
    if (out_counts) std::memcpy(out_counts, counts, 8);
}

}  // namespace

extern "C" {

yk_status yk_despeckle(yk_context* ctx, const yk_despeckle_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb,
                       uint8_t* out_mask, uint32_t* out_counts) try {
    if (check_despeckle(desc, film_rgb, res_x, res_y, tile_dim, out_rgb, out_mask, out_counts) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_despeckle: bad argument");
    if (!ctx) {  // the host instance
        despeckle_host(desc, film_rgb, res_x, res_y, tile_dim, samples, out_rgb, out_mask, out_counts);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    float* d_out = sg.output(out_rgb, n_px * 3);
    uint8_t* d_mask = sg.output(out_mask, n_px);  // NULL where the caller wants none: no slot
    uint32_t* d_counts = sg.output(out_counts, 2);
    return sg.run([&] { return enqueue_despeckle(ctx, sg.stream, desc, d_film, res_x, res_y, tile_dim, samples, d_out, d_mask, d_counts); });
}
YK_CATCH(ctx)

yk_status yk_despeckle_device(yk_context* ctx, const yk_despeckle_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb,
                              void* d_out_mask, void* d_out_counts, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_despeckle(desc, d_film_rgb, res_x, res_y, tile_dim, d_out_rgb, d_out_mask, d_out_counts) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_despeckle_device: bad argument");
    // dword loads and stores of the films, 32-bit integer atomics on the counts; the mask is written in bytes
    if (misaligned(4, d_film_rgb, d_out_rgb, d_out_counts)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_despeckle_device: films and counts must be 4-byte aligned");
    return enqueue_despeckle(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, reinterpret_cast<float*>(d_out_rgb),
                             reinterpret_cast<uint8_t*>(d_out_mask), reinterpret_cast<uint32_t*>(d_out_counts));
}

}  // extern "C"
