// yk_denoise.h — the guided denoiser between the film and the tone map: the edge-avoiding à-trous wavelet transform
// (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding À-Trous Wavelet Transform for fast Global Illumination Filtering",
// HPG 2010) with a colour stop, a normal stop and a plane-distance stop, per pixel, on the host and on gfx950.
//
// The reference has no denoiser, so this file is the rule:
//   - IEEE-754 binary32, round to nearest; every operation separate (the library is built with -ffp-contract=off, so
//     nothing below is fused); divisions correctly rounded; exp is det_expf (yk_libm.h).
//   - IEEE leaves the sign and payload of a NaN that an operation PRODUCES to the implementation (x86 and gfx950 differ),
//     so every value this pass computes and stores goes through dn_canon: a NaN is the quiet NaN 0x7fc00000.  A value
//     that is only copied (the film without a sample table, iterations == 0) keeps its bits.
// One text, two instances (the yk_tonemap.h pattern): the host instance (yk_denoise with no context) is what the CPU suite
// pins against an independent restatement; the device instance (yk_denoise.hip) is compared with the host one bit for bit.
#pragma once
#include "yk_libm.h"
#include "yk_math.h"
#include "yk_tonemap.h"

namespace yk {

enum : uint32_t { DN_MAX_ITERATIONS = 8 };

YK_HD float dn_canon(float v) { return v != v ? gl_from_bits(0x7fc00000u) : v; }

// Everything about a denoise that depends on neither the pixel nor the iteration.
struct DnParams {
    uint32_t res_x, res_y;
    uint32_t tile_dim, x_tile_count;  // the sample table's index rule (tm_sample_index), x_tile_count = res_x / tile_dim (FLOOR)
    float sigma_color;
    float den_n, den_p;  // sigma_normal*sigma_normal and sigma_plane*sigma_plane: the denominators of the normal and plane stops
};
// The tile-grid fields, for every pass that reads a sample table through dn_count (the denoiser, the temporal blend).
inline void dn_set_grid(DnParams& a, uint32_t res_x, uint32_t res_y, uint32_t tile_dim) {
    a.res_x = res_x;
    a.res_y = res_y;
    a.tile_dim = tile_dim;
    a.x_tile_count = res_x / tile_dim;
}

// What a tap reads of a pixel: its colour of the previous iteration and its guide record (yk_guide; t is not used).
struct DnTap {
    float c[3];
    float ns[3];
    float hit;  // != 0: a hit
    float p[3];
};

// A guide record as two halves of four floats, (ns, hit) and (p, t): two 16-byte loads on the device, a yk_guide's ns and p
// on the host.  Copies; t is not read (k_variance keeps a luminance in its slot).
YK_HD void dn_guide(const float* ga, const float* gb, float* ns, float& hit, float* p) {
    ns[0] = ga[0];
    ns[1] = ga[1];
    ns[2] = ga[2];
    hit = ga[3];
    p[0] = gb[0];
    p[1] = gb[1];
    p[2] = gb[2];
}

// What every denoise descriptor must satisfy: at most DN_MAX_ITERATIONS iterations, and the sigma of the colour (or
// variance) stop, of the normal stop and of the plane stop each > 0, which refuses a NaN as well.
inline bool dn_desc_ok(uint32_t iterations, float sigma_first, float sigma_normal, float sigma_plane) {
    return iterations <= DN_MAX_ITERATIONS && sigma_first > 0.0f && sigma_normal > 0.0f && sigma_plane > 0.0f;
}

// Input.  The film's RGB; with a sample table each channel is divided by count = (float)samples[tm_sample_index(x, y)]
// when count > 0 (the Filmic tone map's normalisation, tm_filmic step 1).  Without a table, or where the count is 0, the
// bits are copied.
YK_HD void dn_normalise(float count, float* c) {
    if (count > 0.0f) {
        c[0] = dn_canon(c[0] / count);
        c[1] = dn_canon(c[1] / count);
        c[2] = dn_canon(c[2] / count);
    }
}
YK_HD float dn_count(const DnParams& a, const uint32_t* samples, uint32_t x, uint32_t y) {
    return samples ? (float)samples[tm_sample_index(x, y, a.tile_dim, a.x_tile_count)] : 0.0f;
}

// The B3-spline kernel k = (3/8, 1/4, 1/16) by |offset|; h = k[|dx|] * k[|dy|] is exact (9/64 at the centre).
YK_HD float dn_kernel(int d) {
    const int m = d < 0 ? -d : d;
    return m == 0 ? 0.375f : (m == 1 ? 0.25f : 0.0625f);
}

// The colour scale of iteration i: sigma_color / (float)(1 << i), squared — the denominator of the colour stop.
YK_HD float dn_color_denominator(float sigma_color, uint32_t i) {
    const float s = sigma_color / (float)(1u << i);
    return s * s;
}

// The weight of tap Q for pixel P, both inside the film, Q != P:  w = h * exp(-e),  e = (a_c + a_n) + a_p.
//   a_c = ((dr*dr + dg*dg) + db*db) / den_c over c_P - c_Q;
//   both hits:   a_n = dot(n, n) / den_n with n = ns_P - ns_Q  (the library's dot: ((0 + x*x) + y*y) + z*z),
//                a_p = d*d / den_p with d = dot(ns_P, p_Q - p_P): the distance of Q's hit from P's shading plane;
//   both misses: a_n = a_p = 0;   one of each: w = 0.
// A sigma of +inf makes its denominator +inf and its term 0 for every finite numerator.  The caller skips a tap whose
// weight is 0 or NaN, which happens exactly when: one pixel is a hit and the other a miss; e is NaN or +inf (a channel of
// either colour is NaN or infinite, a difference or its square overflows, a guide is not finite, a denominator is 0 or
// the quotient inf / inf); or exp(-e) underflows to 0 (e above about 103.97).
//
// dn_stops: a_n and a_p of two pixels of one hit class (hit: both are hits), apart — every caller adds them to its
// exponent in its own order (dn_weight and vr_weight: (a_c + a_n) + a_p; the variance window: a_n + a_p).
struct DnStops {
    float a_n, a_p;
};
YK_HD DnStops dn_stops(const DnParams& a, bool hit, const float* nsP, const float* pP, const float* nsQ, const float* pQ) {
    float a_n = 0.0f, a_p = 0.0f;
    if (hit) {
        const V3 nP = V3{nsP[0], nsP[1], nsP[2]};
        const V3 n = nP - V3{nsQ[0], nsQ[1], nsQ[2]};
        const float nn = dot(n, n);
        a_n = nn / a.den_n;
        const V3 v = V3{pQ[0], pQ[1], pQ[2]} - V3{pP[0], pP[1], pP[2]};
        const float d = dot(nP, v);
        const float dd = d * d;
        a_p = dd / a.den_p;
    }
    return DnStops{a_n, a_p};
}
YK_HD float dn_weight(const DnParams& a, float den_c, float h, const DnTap& P, const DnTap& Q) {
    const bool hp = P.hit != 0.0f, hq = Q.hit != 0.0f;
    if (hp != hq) return 0.0f;
    const float dr = P.c[0] - Q.c[0], dg = P.c[1] - Q.c[1], db = P.c[2] - Q.c[2];
    const float rr = dr * dr, gg = dg * dg, bb = db * db;
    const float cs = (rr + gg) + bb;
    const float a_c = cs / den_c;
    const DnStops g = dn_stops(a, hp, P.ns, P.p, Q.ns, Q.p);
    const float e = (a_c + g.a_n) + g.a_p;
    const float x = det_expf(-e);
    return h * x;
}

// One pixel of one iteration with step s = 1 << i.  fetch(qx, qy, tap) reads a pixel inside the film.  Taps: dy = -2..2
// outside, dx = -2..2 inside, accumulated in that order; Q = P + s*(dx, dy), skipped when outside the film.  The centre
// tap has weight h = 9/64 alone and is always taken, so the weight sum is never 0; any other tap is skipped — its colour
// neither multiplied nor added — when its weight is 0 or NaN, so an infinite or NaN pixel does not spread.
// out = sum(w * c_Q) / sum(w) per channel, dn_canon'd: a NaN centre stays NaN, canonical.
template <class Fetch>
YK_HD void dn_pixel(const DnParams& a, float den_c, int s, uint32_t x, uint32_t y, const Fetch& fetch, float* out) {
    DnTap P;
    fetch(x, y, P);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + s * dy;
        if (qy < 0 || qy >= (int)a.res_y) continue;
        const float ky = dn_kernel(dy);
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + s * dx;
            if (qx < 0 || qx >= (int)a.res_x) continue;
            const float h = dn_kernel(dx) * ky;
            float w = h;
            DnTap Q = P;
            if (dx != 0 || dy != 0) {
                fetch((uint32_t)qx, (uint32_t)qy, Q);
                w = dn_weight(a, den_c, h, P, Q);
                if (w == 0.0f || w != w) continue;
            }
            const float pr = w * Q.c[0], pg = w * Q.c[1], pb = w * Q.c[2];
            sr = sr + pr;
            sg = sg + pg;
            sb = sb + pb;
            sw = sw + w;
        }
    }
    out[0] = dn_canon(sr / sw);
    out[1] = dn_canon(sg / sw);
    out[2] = dn_canon(sb / sw);
}

}  // namespace yk
