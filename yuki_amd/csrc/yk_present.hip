// yk_present.hip — ScaleOutput::draw (app/renderpasses/scale_output.rs) on gfx950, behind yk_present, yk_present_device and
// yk_present_target_rect; the per-pixel arithmetic is yk_present.h's, whose host instance these entry points run without a
// context.
//
// One launch writes the whole window, letterbox included, so the frame needs no memset:
//   - k_present: one lane per window pixel, a block is PR_BLOCK consecutive pixels of ONE row (grid.y = the row), so the
//     row's tap j0 and weight b are uniform over the block and a wave covers 64 consecutive pixels.  A lane reads up to
//     2 x 2 texels of 12 bytes with dword loads (the film needs 4-byte alignment only; neighbouring lanes share texels, so
//     the taps come out of L1 / L2 when the film is magnified) and stores one 32-bit RGBA8 word, or three floats.
// No work buffer, no allocation, no host synchronisation in the stream-ordered entry point.
#include <hip/hip_runtime.h>

#include <cstring>

#include "yk_film_call.h"
#include "yk_present.h"
#include "yk_staging.h"

namespace {

constexpr unsigned PR_BLOCK = 256;  // 4 waves of 64

// film and out never overlap (checked by the entry points).
__global__ __launch_bounds__(PR_BLOCK) void k_present(const float* __restrict__ film, void* __restrict__ out, PresentArgs p) {
    const uint32_t y = blockIdx.y;
    const uint32_t x = blockIdx.x * PR_BLOCK + threadIdx.x;
    int32_t j0 = 0;
    float b = 0.0f;
    const bool row_inside = pr_axis(y, p.rect.y0, p.rect.height, p.h, j0, b);
    if (x >= p.W) return;
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    const bool inside = pr_pixel(p, film, x, row_inside, j0, b, rgb);
    const size_t px = (size_t)y * p.W + x;
    if (p.format == PR_RGBA8) {
        reinterpret_cast<uint32_t*>(out)[px] = inside ? pr_pack(rgb[0], rgb[1], rgb[2]) : 0xff000000u;
    } else {
        float* o = reinterpret_cast<float*>(out) + 3 * px;
        o[0] = rgb[0];
        o[1] = rgb[1];
        o[2] = rgb[2];
    }
}

size_t out_bytes(const yk_present_desc* d) { return (size_t)d->window_x * d->window_y * (d->format == YK_PRESENT_RGBA8 ? 4 : 12); }

yk_status check_call(const yk_present_desc* d, const void* film, uint16_t res_x, uint16_t res_y, const void* out) {
    if (!d || !film || !out || res_x == 0 || res_y == 0 || d->window_x == 0 || d->window_y == 0) return YK_ERR_INVALID_ARGUMENT;
    if (d->encode > YK_PRESENT_ENCODE_SRGB || d->format > YK_PRESENT_RGB32F) return YK_ERR_INVALID_ARGUMENT;
    if (overlaps(film, (size_t)res_x * res_y * 12, out, out_bytes(d))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

PresentArgs make_args(const yk_present_desc* d, uint16_t res_x, uint16_t res_y) {
    PresentArgs p;
    p.w = res_x;
    p.h = res_y;
    p.W = d->window_x;
    p.H = d->window_y;
    p.rect = pr_target_rect(p.w, p.h, p.W, p.H);
    p.encode = d->encode;
    p.format = d->format;
    return p;
}

yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_present_desc* d, const float* film, uint16_t res_x, uint16_t res_y, void* out) {
    const PresentArgs p = make_args(d, res_x, res_y);
    hipLaunchKernelGGL(k_present, dim3((p.W + PR_BLOCK - 1) / PR_BLOCK, p.H), dim3(PR_BLOCK), 0, st, film, out, p);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void present_host(const yk_present_desc* d, const float* film, uint16_t res_x, uint16_t res_y, void* out) {
    const PresentArgs p = make_args(d, res_x, res_y);
    uint8_t* o = reinterpret_cast<uint8_t*>(out);  // bytes: a host frame needs no alignment
    for (uint32_t y = 0; y < p.H; ++y) {
        int32_t j0 = 0;
        float b = 0.0f;
        const bool row_inside = pr_axis(y, p.rect.y0, p.rect.height, p.h, j0, b);
        for (uint32_t x = 0; x < p.W; ++x) {
            float rgb[3] = {0.0f, 0.0f, 0.0f};
            const bool inside = pr_pixel(p, film, x, row_inside, j0, b, rgb);
            const size_t px = (size_t)y * p.W + x;
            if (p.format == PR_RGBA8) {
                const uint32_t v = inside ? pr_pack(rgb[0], rgb[1], rgb[2]) : 0xff000000u;
                o[4 * px] = (uint8_t)v;
                o[4 * px + 1] = (uint8_t)(v >> 8);
                o[4 * px + 2] = (uint8_t)(v >> 16);
                o[4 * px + 3] = (uint8_t)(v >> 24);
            } else {
                std::memcpy(o + 12 * px, rgb, 12);
            }
        }
    }
}

}  // namespace

extern "C" {

yk_status yk_present_target_rect(uint16_t res_x, uint16_t res_y, uint16_t window_x, uint16_t window_y, yk_present_rect* out) {
    if (!out || res_x == 0 || res_y == 0 || window_x == 0 || window_y == 0) return YK_ERR_INVALID_ARGUMENT;
    const PresentRect r = pr_target_rect(res_x, res_y, window_x, window_y);
    out->x0 = r.x0;
    out->y0 = r.y0;
    out->width = r.width;
    out->height = r.height;
    return YK_OK;
}

yk_status yk_present(yk_context* ctx, const yk_present_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, void* out) try {
    if (check_call(desc, film_rgb, res_x, res_y, out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_present: bad argument");
    if (!ctx) {  // the host instance
        present_host(desc, film_rgb, res_x, res_y, out);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const float* d_film = sg.upload(film_rgb, (size_t)res_x * res_y * 3);
    void* d_out = sg.output(reinterpret_cast<uint8_t*>(out), out_bytes(desc));
    return sg.run([&] { return enqueue(ctx, sg.stream, desc, d_film, res_x, res_y, d_out); });
} YK_CATCH(ctx)

yk_status yk_present_device(yk_context* ctx, const yk_present_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, void* d_out, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(desc, d_film_rgb, res_x, res_y, d_out) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_present_device: bad argument");
    // dword loads of the film, one 32-bit store a pixel (RGBA8) or float stores (RGB32F)
    if (misaligned(4, d_film_rgb, d_out)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_present_device: film and frame must be 4-byte aligned");
    return enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, d_out);
}

}  // extern "C"
