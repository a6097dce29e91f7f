// yk_present.h — the last pass of the reference's frame (app/window.rs:246-270): ScaleOutput::draw
// (app/renderpasses/scale_output.rs) per window pixel, on the host and on gfx950.
//
// The reference draws the tone-mapped film as a textured quad into the window's back buffer: stretched with bilinear
// filtering, the aspect ratio kept, sRGB-encoded, 8 bits a channel.  GL fixes no bit-level result for a textured quad,
// so this file fixes one rule:
//   - IEEE-754 binary32, round to nearest; every operation separate (the library is built with -ffp-contract=off, so
//     nothing below is fused); divisions correctly rounded; texture coordinates exact, in integers.
//   - IEEE leaves the sign and payload of a NaN that an operation PRODUCES to the implementation (x86 and gfx950 differ),
//     so every arithmetic result that is a NaN is the quiet NaN 0x7fc00000 (pr_canon).  A value that is only copied — the
//     identity scale, a tap with weight one — keeps its bits, NaN payloads and -0 included.
// One text, two instances (the yk_tonemap.h pattern): the host instance (yk_present with no context) is what the CPU suite
// pins against an independent restatement; the device instance (yk_present.hip) is compared with the host one bit for bit.
#pragma once
#include "yk_libm.h"
#include "yk_math.h"
#include "yk_tonemap.h"

namespace yk {

enum : uint32_t { PR_ENCODE_NONE = 0, PR_ENCODE_SHADER = 1, PR_ENCODE_SRGB = 2 };
enum : uint32_t { PR_RGBA8 = 0, PR_RGB32F = 1 };

struct PresentRect {
    int32_t x0, y0;          // top-down window coordinates of the rectangle's first column and row
    uint32_t width, height;  // either may be 0: the rectangle covers nothing
};

// The target rectangle (scale_output.rs:64-84), in the reference's own u32 arithmetic.  Film w x h, window W x H, all
// non-zero and below 2^16, so W*h and H*w fit in u32.  The aspects are compared in binary32 (:66-68).
//   frame_aspect < texture_aspect (:69-75): scaled_height = (W*h)/w, left = 0, width = W,
//     bottom = (H saturating_sub scaled_height)/2 + scaled_height;
//   otherwise (:77-83): scaled_width = (H*w)/h, left = (W saturating_sub scaled_width)/2, bottom = H, height = H.
// `bottom` counts from the window's LOWER edge and the quad's height is negative (:74, :82: the flip that puts film row 0
// at the top), so in top-down rows the rectangle starts at y0 = H - bottom: when H - scaled_height is odd the larger
// margin is above.  The float NDC round trip (:86-89) moves an edge by far less than half a pixel and pixel centres sit
// at .5, so coverage is exactly this integer rectangle, clipped to the window (pr_axis tests 0 <= i - x0 < width for
// window pixels only).  The rectangle never exceeds the window: the binary32 comparison separates aspects that differ
// by a whole pixel of scaled size.
YK_HD PresentRect pr_target_rect(uint32_t w, uint32_t h, uint32_t W, uint32_t H) {
    const float frame_aspect = (float)W / (float)H;
    const float texture_aspect = (float)w / (float)h;
    PresentRect r;
    if (frame_aspect < texture_aspect) {
        const uint32_t sh = (W * h) / w;
        const uint32_t bottom = (H > sh ? H - sh : 0u) / 2u + sh;
        r.x0 = 0;
        r.y0 = (int32_t)H - (int32_t)bottom;
        r.width = W;
        r.height = sh;
    } else {
        const uint32_t sw = (H * w) / h;
        r.x0 = (int32_t)((W > sw ? W - sw : 0u) / 2u);
        r.y0 = 0;
        r.width = sw;
        r.height = H;
    }
    return r;
}

// One axis of the texture coordinate.  Output pixel i (a window column or row) against the rectangle's start x0 and
// extent `extent` over `texels` texels.  The quad interpolates uv linearly from 0 to 1 across the rectangle (:14-30), the
// pixel centre sits at .5 and texel centres at .5 (GL LINEAR), so the first tap and its neighbour's weight are
//   n = (2*(i - x0) + 1)*texels - extent,  d = 2*extent,  i0 = floor_div(n, d),  r = n - i0*d,  a = (float)r / (float)d
// exactly: magnification by an integer factor and the identity (a == 0 everywhere) have exact taps.  n needs 34 bits;
// with k = i - x0 and k*texels = q*extent + m (u32), n = d*q + (2*m + texels - extent), whose second term fits in int32,
// so the same i0 and r come from 32-bit divisions.  r < d <= 131070: both conversions and the division are exact /
// correctly rounded.  Returns false when pixel i is outside the rectangle.
YK_HD bool pr_axis(uint32_t i, int32_t x0, uint32_t extent, uint32_t texels, int32_t& i0, float& a) {
    const int32_t ks = (int32_t)i - x0;
    if (ks < 0 || (uint32_t)ks >= extent) return false;
    const uint32_t kt = (uint32_t)ks * texels;
    const uint32_t q = kt / extent;
    const uint32_t m = kt - q * extent;
    const int32_t d = (int32_t)(2u * extent);
    int32_t t = (int32_t)(2u * m + texels) - (int32_t)extent;  // in (-extent, 2*extent + texels)
    int32_t f = t / d;                                         // truncates; floor for t < 0 is one less unless exact
    int32_t r = t - f * d;
    if (r < 0) {
        r += d;
        f -= 1;
    }
    i0 = (int32_t)q + f;
    a = (float)r / (float)d;
    return true;
}

YK_HD float pr_canon(float v) { return v != v ? gl_from_bits(0x7fc00000u) : v; }

// GLSL mix(x, y, a) = x*(1 - a) + y*a, every operation separate; a == 0 returns x itself (bits kept).  The caller does
// not read y when a == 0, so a tap of weight zero cannot leak a NaN.  a < 1 always: x always has weight.
YK_HD float pr_mix(float x, float y, float a) {
    if (a == 0.0f) return x;
    const float w = 1.0f - a;
    const float p = x * w;
    const float q = y * a;
    return pr_canon(p + q);
}

// One texel for the filter: MinifySamplerFilter::Linear / MagnifySamplerFilter::Linear (:58-62: 2 x 2 taps, no mip
// levels) under SamplerWrapFunction::BorderClamp (:60) — a tap outside [0, w) x [0, h) is GL's default border colour
// (0, 0, 0), which gives the rectangle a dark half-texel fringe when the film is magnified.  Reproduced.
YK_HD void pr_texel(const float* film, uint32_t w, uint32_t h, int32_t i, int32_t j, float* c) {
    if (i < 0 || j < 0 || (uint32_t)i >= w || (uint32_t)j >= h) {
        c[0] = c[1] = c[2] = 0.0f;
        return;
    }
    const float* p = film + 3 * ((size_t)j * w + (size_t)i);
    c[0] = p[0];
    c[1] = p[1];
    c[2] = p[2];
}

// texture(input_texture, frag_uv).rgb (:165): the two horizontal mixes first, then the vertical one.  The taps at i0 + 1
// and in row j0 + 1 are read only when their weight is not zero.
YK_HD void pr_sample(const float* film, uint32_t w, uint32_t h, int32_t i0, float a, int32_t j0, float b, float* rgb) {
    float t00[3], t10[3] = {0.0f, 0.0f, 0.0f};
    pr_texel(film, w, h, i0, j0, t00);
    if (a != 0.0f) pr_texel(film, w, h, i0 + 1, j0, t10);
    for (int k = 0; k < 3; ++k) rgb[k] = pr_mix(t00[k], t10[k], a);
    if (b == 0.0f) return;
    float t01[3], t11[3] = {0.0f, 0.0f, 0.0f};
    pr_texel(film, w, h, i0, j0 + 1, t01);
    if (a != 0.0f) pr_texel(film, w, h, i0 + 1, j0 + 1, t11);
    for (int k = 0; k < 3; ++k) rgb[k] = pr_mix(rgb[k], pr_mix(t01[k], t11[k], a), b);
}

// pow(x, y) = exp(y * log(x)) with yk_libm.h's functions; only ever called with x > 0.0031308.
YK_HD float pr_pow(float x, float y) {
    const float l = det_logf(x);
    const float e = y * l;
    return det_expf(e);
}

// PR_ENCODE_SHADER: the shader's linearToSRGB (:154-158) under gamma_before_output != 0:
//   x <= 0.0031308 ? 12.92*x : 1.055*pow(x, 1/gamma) - 0.055 with gamma = 2.2.  A NaN fails the comparison and stays a NaN.
// PR_ENCODE_SRGB: what an sRGB back buffer stores when the shader writes linear values, the reference's default
//   (window.rs:94-127) — the OpenGL sRGB conversion: 0 for x <= 0 or NaN, 12.92*x below 0.0031308,
//   1.055*pow(x, 0.41666) - 0.055 below 1, 1 otherwise.
YK_HD float pr_encode(uint32_t encode, float x) {
    if (encode == PR_ENCODE_SHADER) {
        if (x != x) return pr_canon(x);
        if (x <= 0.0031308f) return 12.92f * x;
        const float p = pr_pow(x, 1.0f / 2.2f);
        const float s = 1.055f * p;
        return s - 0.055f;
    }
    if (encode == PR_ENCODE_SRGB) {
        if (!(x > 0.0f)) return 0.0f;
        if (x < 0.0031308f) return 12.92f * x;
        if (x < 1.0f) {
            const float p = pr_pow(x, 0.41666f);
            const float s = 1.055f * p;
            return s - 0.055f;
        }
        return 1.0f;
    }
    return x;
}

// One channel of the 8-bit frame buffer: (uint8_t)(saturate(x)*255 + 0.5), saturate as the tone map's (NaN -> 0).
YK_HD uint32_t pr_quantise(float x) {
    const float s = tm_saturate(x) * 255.0f;
    return (uint32_t)(s + 0.5f);
}

// R, G, B, A = 255 in byte order, as one little-endian word.  The clear colour (0, 0, 0, 1) of window.rs:247 is
// pr_pack(0, 0, 0).
YK_HD uint32_t pr_pack(float r, float g, float b) { return pr_quantise(r) | (pr_quantise(g) << 8) | (pr_quantise(b) << 16) | 0xff000000u; }

// Everything about a present that does not depend on the pixel.
struct PresentArgs {
    uint32_t w, h, W, H;  // film, window
    PresentRect rect;
    uint32_t encode, format;
};

// Window pixel (x, y) given its row's (inside, j0, b): the encoded colour, or false for the clear colour.
YK_HD bool pr_pixel(const PresentArgs& p, const float* film, uint32_t x, bool row_inside, int32_t j0, float b, float* rgb) {
    int32_t i0;
    float a;
    if (!row_inside || !pr_axis(x, p.rect.x0, p.rect.width, p.w, i0, a)) return false;
    pr_sample(film, p.w, p.h, i0, a, j0, b, rgb);
    for (int k = 0; k < 3; ++k) rgb[k] = pr_encode(p.encode, rgb[k]);
    return true;
}

}  // namespace yk
