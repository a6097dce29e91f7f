// yk_upsample.hip — the guided upsample on gfx950, behind yk_upsample and yk_upsample_device; the per-pixel arithmetic is
// yk_upsample.h's, whose host instance these entry points run without a context.
//
// k_upsample<ALBEDO, DIRECT>: one lane per FULL pixel, a block is a 32 x 8 tile of the full film (yk_film_tile.h).  A lane
//   requests its own records first — the full guide (two 16-byte loads) and, with ALBEDO, the full albedo (one), all
//   coalesced — and writes three dwords of RGB as the à-trous OUT_RGB does, and one of weight where the caller asked.
//   The block's 256 lanes ask for 1024 taps of at most (ceil(32/s) + 2) x (ceil(8/s) + 2) low records (340 at s = 1, 108 at
//   s = 2), so the block stages that window in LDS once: colours in one float4 array and guides in two, as k_atrous lays
//   them out, and a tap is three ds_read_b128.  Normalisation by the low sample table and demodulation by the low albedo
//   happen at staging: one division per low record, not per tap — the rule's "once per low pixel", so the same bits.
//   The window is found from the footprints of the block's first and last pixel (up_axis is monotone in x); s is uniform,
//   and the integer divisions by it are two per lane and four per block, none per tap.  A window entry outside the low
//   film is neither written nor read: the rule asks for such a tap at the clamped index, which lies inside the window.
//   DIRECT (a timing build, -DYK_UPSAMPLE_DIRECT): every tap from global memory, normalised and demodulated per tap — the
//   measurement that kept the LDS window (at 1920 x 1080 a call takes 42.3 - 42.7 us with the window and
//   48.3 - 48.5 us without at s = 2, 40.3 - 40.6 against 47.8 - 48.1 us at s = 4, five alternating runs each, same bits).
//   Compiled for gfx950: 68 VGPRs (66 without ALBEDO), 16 320 bytes of LDS, no scratch, 7 waves per SIMD.
// The low film's sample table is staged into ctx->upsample.samples through the pinned copy the tone map and the denoiser
// share; the stream-ordered entry point allocates nothing once the context has seen a table of that size.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_staging.h"
#include "yk_upsample.h"

namespace {

struct UpIo {
    const float* low_rgb;         // the low film ...
    const uint32_t* samples;      // ... and its sample table (may be NULL)
    const float4* low_guides;     // two float4 a low pixel: (ns, hit), (p, t)
    const float4* low_albedo;     // ALBEDO: one float4 a low pixel
    const float4* guides;         // two float4 a full pixel
    const float4* albedo;         // ALBEDO: one float4 a full pixel
    float* out_rgb;
    float* out_weight;            // may be NULL
};

// the widest window: s = 1, where footprints of 32 x 8 pixels span 33 x 9 low pixels; one spare column and row
constexpr int UP_W = (int)FT_TX + 2, UP_ROWS = (int)FT_TY + 2, UP_N = UP_W * UP_ROWS;

// c_Q of low pixel q = (gx, gy) with its guide halves
template <bool ALBEDO>
__device__ __forceinline__ float4 up_low_record(const UpIo& io, const UpParams& a, size_t q, uint32_t gx, uint32_t gy) {
    float4 al = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ALBEDO) al = io.low_albedo[q];  // requested before the film is waited for
    float c[3] = {io.low_rgb[3 * q], io.low_rgb[3 * q + 1], io.low_rgb[3 * q + 2]};
    const float alb[3] = {al.x, al.y, al.z};
    up_low_colour(dn_count(a.dn, io.samples, gx, gy), ALBEDO ? alb : nullptr, c);
    return make_float4(c[0], c[1], c[2], 0.0f);
}

__device__ __forceinline__ void up_set_tap(DnTap& t, const float4& c, const float4& ga, const float4& gb) {
    t.c[0] = c.x;
    t.c[1] = c.y;
    t.c[2] = c.z;
    dn_guide(&ga.x, &gb.x, t.ns, t.hit, t.p);
}

template <bool ALBEDO, bool DIRECT>
__global__ __launch_bounds__(FT_TX* FT_TY) void k_upsample(UpIo io, UpParams a) {
    const uint32_t bx = blockIdx.x * FT_TX, by = blockIdx.y * FT_TY;
    const uint32_t x = bx + threadIdx.x, y = by + threadIdx.y;
    const bool inside = x < a.full_x && y < a.full_y;
    const size_t i = (size_t)y * a.full_x + x;
    float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gb = ga, al = ga;
    if (inside) {  // the lane's own records, in flight while the window is staged
        ga = io.guides[2 * i];
        gb = io.guides[2 * i + 1];
        if (ALBEDO) al = io.albedo[i];
    }
    const uint32_t X = x / a.s, Y = y / a.s;
    const uint32_t pi = x - a.s * X, pj = y - a.s * Y;
    float rec[4];
    const float nsP[3] = {ga.x, ga.y, ga.z}, pP[3] = {gb.x, gb.y, gb.z}, albP[3] = {al.x, al.y, al.z};
    if constexpr (DIRECT) {
        if (!inside) return;
        up_pixel(a, X, pi, Y, pj, nsP, ga.w, pP, ALBEDO ? albP : nullptr,
                 [&](uint32_t qx, uint32_t qy, DnTap& t) {
                     const size_t q = (size_t)qy * a.dn.res_x + qx;
                     const float4 qa = io.low_guides[2 * q], qb = io.low_guides[2 * q + 1];
                     up_set_tap(t, up_low_record<ALBEDO>(io, a, q, qx, qy), qa, qb);
                 },
                 rec);
    } else {
        __shared__ float4 lds_c[UP_N], lds_a[UP_N], lds_b[UP_N];
        // the window: from the first tap of the block's first pixel to the second tap of its last pixel inside the film
        const uint32_t xl = min(bx + FT_TX - 1u, a.full_x - 1u), yl = min(by + FT_TY - 1u, a.full_y - 1u);
        const uint32_t Xf = bx / a.s, Yf = by / a.s, Xl = xl / a.s, Yl = yl / a.s;
        int wx0, wy0, wx1, wy1;
        float unused;
        up_axis(Xf, bx - a.s * Xf, a.s, wx0, unused);
        up_axis(Yf, by - a.s * Yf, a.s, wy0, unused);
        up_axis(Xl, xl - a.s * Xl, a.s, wx1, unused);
        up_axis(Yl, yl - a.s * Yl, a.s, wy1, unused);
        // The window fits the arrays for every s >= 1: up_axis gives x0(x) = floor((2x + 1 - s) / (2s)), so over the block's
        // FT_TX columns x0 grows by at most ceil((FT_TX - 1) / s) <= FT_TX - 1, and with the second tap of the last pixel the
        // window is at most FT_TX + 1 wide (33) and FT_TY + 1 high (9).
        static_assert(UP_W >= (int)FT_TX + 1 && UP_ROWS >= (int)FT_TY + 1, "the LDS arrays hold the widest window (s = 1)");
        const int w_w = wx1 + 2 - wx0, w_h = wy1 + 2 - wy0;
        for (int ry = (int)threadIdx.y; ry < w_h; ry += (int)FT_TY)
            for (int rx = (int)threadIdx.x; rx < w_w; rx += (int)FT_TX) {
                const int gx = wx0 + rx, gy = wy0 + ry;
                if (gx < 0 || gy < 0 || gx >= (int)a.dn.res_x || gy >= (int)a.dn.res_y) continue;
                const size_t q = (size_t)gy * a.dn.res_x + (size_t)gx;
                const int k = ry * UP_W + rx;
                lds_c[k] = up_low_record<ALBEDO>(io, a, q, (uint32_t)gx, (uint32_t)gy);
                lds_a[k] = io.low_guides[2 * q];
                lds_b[k] = io.low_guides[2 * q + 1];
            }
        __syncthreads();
        if (!inside) return;
        up_pixel(a, X, pi, Y, pj, nsP, ga.w, pP, ALBEDO ? albP : nullptr,
                 [&](uint32_t qx, uint32_t qy, DnTap& t) {
                     const int k = ((int)qy - wy0) * UP_W + ((int)qx - wx0);
                     up_set_tap(t, lds_c[k], lds_a[k], lds_b[k]);
                 },
                 rec);
    }
    io.out_rgb[3 * i] = rec[0];
    io.out_rgb[3 * i + 1] = rec[1];
    io.out_rgb[3 * i + 2] = rec[2];
    if (io.out_weight) io.out_weight[i] = rec[3];  // a uniform branch on a kernel argument
}

#ifdef YK_UPSAMPLE_DIRECT
constexpr bool UP_DIRECT = true;
#else
constexpr bool UP_DIRECT = false;
#endif

// What both entry points refuse alike; n_lo and n_full pixels.
yk_status check_call(const yk_upsample_desc* d, const void* low_rgb, const void* low_guides, const void* low_albedo, uint16_t low_res_x, uint16_t low_res_y, uint16_t tile_dim,
                     const void* guides, const void* albedo, const void* out_rgb, const void* out_weight) {
    if (!low_rgb || !low_guides || !guides || !out_rgb || low_res_x == 0 || low_res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    if (!up_desc_ok(d, low_res_x, low_res_y)) return YK_ERR_INVALID_ARGUMENT;
    if ((low_albedo == nullptr) != (albedo == nullptr)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_lo = (size_t)low_res_x * low_res_y, n_full = n_lo * d->s * d->s;
    const struct {
        const void* p;
        size_t bytes;
    } in[5] = {{low_rgb, n_lo * 12}, {low_guides, n_lo * sizeof(yk_guide)}, {low_albedo, n_lo * sizeof(yk_albedo)}, {guides, n_full * sizeof(yk_guide)}, {albedo, n_full * sizeof(yk_albedo)}};
    for (const auto& v : in) {
        if (!v.p) continue;
        if (overlaps(out_rgb, n_full * 12, v.p, v.bytes)) return YK_ERR_INVALID_ARGUMENT;
        if (out_weight && overlaps(out_weight, n_full * 4, v.p, v.bytes)) return YK_ERR_INVALID_ARGUMENT;
    }
    if (out_weight && overlaps(out_weight, n_full * 4, out_rgb, n_full * 12)) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

// One launch on `st`, the sample table staged before it; nothing checked.
yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_upsample_desc* d, const float* low_rgb, const void* low_guides, const void* low_albedo, uint16_t low_res_x, uint16_t low_res_y,
                  uint16_t tile_dim, const uint32_t* samples, const void* guides, const void* albedo, float* out_rgb, float* out_weight) {
    const UpParams a = up_make_params(d, low_res_x, low_res_y, tile_dim);
    UpIo io{low_rgb,  nullptr, reinterpret_cast<const float4*>(low_guides), reinterpret_cast<const float4*>(low_albedo), reinterpret_cast<const float4*>(guides), reinterpret_cast<const float4*>(albedo),
            out_rgb, out_weight};
    if (yk_status ss = stage_samples(ctx, st, samples, low_res_x, low_res_y, tile_dim, ctx->upsample.samples, &io.samples)) return ss;
    if (albedo) hipLaunchKernelGGL((k_upsample<true, UP_DIRECT>), ft_grid(a.full_x, a.full_y), ft_block(), 0, st, io, a);
    else hipLaunchKernelGGL((k_upsample<false, UP_DIRECT>), ft_grid(a.full_x, a.full_y), ft_block(), 0, st, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// The host instance: c_Q of every low pixel once, then every full pixel.
void upsample_host(const yk_upsample_desc* d, const float* low_rgb, const yk_guide* low_guides, const yk_albedo* low_albedo, uint16_t low_res_x, uint16_t low_res_y, uint16_t tile_dim,
                   const uint32_t* samples, const yk_guide* guides, const yk_albedo* albedo, float* out_rgb, float* out_weight) {
    const UpParams a = up_make_params(d, low_res_x, low_res_y, tile_dim);
    std::vector<float> c((size_t)3 * low_res_x * low_res_y);
    for (uint32_t gy = 0; gy < low_res_y; ++gy)
        for (uint32_t gx = 0; gx < low_res_x; ++gx) {
            const size_t q = (size_t)gy * low_res_x + gx;
            std::memcpy(&c[3 * q], low_rgb + 3 * q, 12);
            up_low_colour(dn_count(a.dn, samples, gx, gy), low_albedo ? low_albedo[q].a : nullptr, &c[3 * q]);
        }
    const auto fetch = [&](uint32_t qx, uint32_t qy, DnTap& t) {
        const size_t q = (size_t)qy * low_res_x + qx;
        std::memcpy(t.c, &c[3 * q], 12);
        dn_guide(low_guides[q].ns, low_guides[q].p, t.ns, t.hit, t.p);
    };
    for (uint32_t y = 0; y < a.full_y; ++y)
        for (uint32_t x = 0; x < a.full_x; ++x) {
            const size_t i = (size_t)y * a.full_x + x;
            const uint32_t X = x / a.s, Y = y / a.s;
            float rec[4];
            up_pixel(a, X, x - a.s * X, Y, y - a.s * Y, guides[i].ns, guides[i].hit, guides[i].p, albedo ? albedo[i].a : nullptr, fetch, rec);
            std::memcpy(out_rgb + 3 * i, rec, 12);
            if (out_weight) out_weight[i] = rec[3];
        }
}

}  // namespace

extern "C" {

yk_status yk_upsample(yk_context* ctx, const yk_upsample_desc* desc, const float* low_rgb, const yk_guide* low_guides, const yk_albedo* low_albedo, uint16_t low_res_x, uint16_t low_res_y,
                      uint16_t tile_dim, const uint32_t* samples, const yk_guide* guides, const yk_albedo* albedo, float* out_rgb, float* out_weight) try {
    if (check_call(desc, low_rgb, low_guides, low_albedo, low_res_x, low_res_y, tile_dim, guides, albedo, out_rgb, out_weight) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_upsample: bad argument");
    if (!ctx) {  // the host instance
        upsample_host(desc, low_rgb, low_guides, low_albedo, low_res_x, low_res_y, tile_dim, samples, guides, albedo, out_rgb, out_weight);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_lo = (size_t)low_res_x * low_res_y, n_full = n_lo * desc->s * desc->s;
    const float* d_low_rgb = sg.upload(low_rgb, n_lo * 3);
    const yk_guide* d_low_guides = sg.upload(low_guides, n_lo);
    const yk_albedo* d_low_albedo = low_albedo ? sg.upload(low_albedo, n_lo) : nullptr;
    const yk_guide* d_guides = sg.upload(guides, n_full);
    const yk_albedo* d_albedo = albedo ? sg.upload(albedo, n_full) : nullptr;
    float* d_out_rgb = sg.output(out_rgb, n_full * 3);
    float* d_out_weight = sg.output(out_weight, n_full);  // an output the caller left out takes no slot and stays NULL
    return sg.run([&] { return enqueue(ctx, sg.stream, desc, d_low_rgb, d_low_guides, d_low_albedo, low_res_x, low_res_y, tile_dim, samples, d_guides, d_albedo, d_out_rgb, d_out_weight); });
}
YK_CATCH(ctx)

yk_status yk_upsample_device(yk_context* ctx, const yk_upsample_desc* desc, const void* d_low_rgb, const void* d_low_guides, const void* d_low_albedo, uint16_t low_res_x, uint16_t low_res_y,
                             uint16_t tile_dim, const uint32_t* samples, const void* d_guides, const void* d_albedo, void* d_out_rgb, void* d_out_weight, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(desc, d_low_rgb, d_low_guides, d_low_albedo, low_res_x, low_res_y, tile_dim, d_guides, d_albedo, d_out_rgb, d_out_weight) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_upsample_device: bad argument");
    // dword loads and stores of the low film, the RGB output and the weight, 16-byte loads of the guides and the albedo
    if (misaligned(4, d_low_rgb, d_out_rgb, d_out_weight) || misaligned(16, d_low_guides, d_low_albedo, d_guides, d_albedo))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_upsample_device: film, RGB output and weight must be 4-byte aligned, guides and albedo 16-byte aligned");
    return enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_low_rgb), d_low_guides, d_low_albedo, low_res_x, low_res_y, tile_dim, samples, d_guides, d_albedo,
                   reinterpret_cast<float*>(d_out_rgb), reinterpret_cast<float*>(d_out_weight));
}

}  // extern "C"
