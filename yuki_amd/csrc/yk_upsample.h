// yk_upsample.h — a film rendered at 1/s resolution rebuilt at full resolution through the first-hit guides of both
// resolutions: a joint-bilateral upsample (Kopf, Cohen, Lischinski, Uyttendaele: "Joint Bilateral Upsampling", SIGGRAPH
// 2007) of demodulated radiance, remodulated with the full-resolution albedo.  It sits between the low-resolution film (or
// its denoiser) and the tone map.  A plain bilinear stretch (what yk_present does to a small film) blurs every texture and
// smears every silhouette; here the texture comes from the full-resolution albedo and a tap across a silhouette has
// weight 0.
//
// The reference has no such pass, so this file is the rule.  Its arithmetic is yk_denoise.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), divisions correctly rounded;
//     exp is det_expf (yk_libm.h);
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and k_upsample of yk_upsample.hip call the functions below and
// agree bit for bit.
//
// Limits:
//   - A low pixel's film value averages its whole footprint while its guide is ONE ray through its centre: full pixels
//     beside a silhouette inherit a mixed value.
//   - A feature no low centre ray hits has no tap of its own class: it falls back to the containing low pixel.
//   - Glass, metal and glossy surfaces are not demodulated (their albedo record is all ones).
//   - yk_multi scenes are not served.  A temporal history at full resolution over upsampled frames is not addressed: the
//     history can be carried at low resolution and upsampled last.
//   - The full albedo of a texture finer than a pixel must be a pixel mean (yk_albedo_mean) for the pass to gain anything.
// Measured (profiles/upsample_quality.json, profiles/upsample_device.json): on the oracle's textured-city
// films, 4 spp at 48 x 27 -> 96 x 54, the error is 0.90 x a bilinear stretch's with pixel-mean albedo records at both
// resolutions and 1.00 x — no gain — with the centre ray's; on textured-cornell (texels larger than a pixel) 0.96 x with
// the centre ray's, all of it from the guides; on untextured city-small the bilinear stretch is better.  On one
// MI355X at 1920 x 1080 k_upsample takes 39.8 us at s = 2 and 37.7 us at s = 4, twice its bytes over the HBM peak.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_albedo.h"
#include "yk_denoise.h"
#include "yk_temporal.h"

namespace yk {

// Everything about a call that does not depend on the pixel.  dn carries the LOW film's resolution, the index rule of its
// sample table (tm_sample_index through dn_count) and the denominators of the normal and the plane stop; its sigma_color
// is not used.  The full film is exactly (s * dn.res_x) x (s * dn.res_y).
struct UpParams {
    DnParams dn;
    uint32_t s;
    uint32_t full_x, full_y;
};
// What yk_upsample asks of its descriptor and of the two resolutions: 1 <= s <= YK_UPSAMPLE_MAX_S, s * low_res <= 65535,
// each sigma > 0 (which refuses a NaN as well; +inf switches its stop off).
inline bool up_desc_ok(const yk_upsample_desc* d, uint32_t low_res_x, uint32_t low_res_y) {
    if (!d || d->s < 1u || d->s > YK_UPSAMPLE_MAX_S) return false;
    if (d->s * low_res_x > 65535u || d->s * low_res_y > 65535u) return false;
    return d->sigma_normal > 0.0f && d->sigma_plane > 0.0f;
}
inline UpParams up_make_params(const yk_upsample_desc* d, uint32_t low_res_x, uint32_t low_res_y, uint32_t tile_dim) {
    UpParams a{};
    dn_set_grid(a.dn, low_res_x, low_res_y, tile_dim);
    a.dn.den_n = d->sigma_normal * d->sigma_normal;
    a.dn.den_p = d->sigma_plane * d->sigma_plane;
    a.s = d->s;
    a.full_x = d->s * low_res_x;
    a.full_y = d->s * low_res_y;
    return a;
}

// Geometry, one axis.  Full pixel x = s*X + i (X = x / s and i = x - s*X in integers) lies in low pixel X — yk_albedo_mean's
// relation.  Its centre sits at t = (2i + 1 - s) / (2s) low pixels from the centre of X: the numerator an exact integer,
// converted, and ONE division by (float)(2s).  t < 0: the footprint starts one pixel earlier, x0 = X - 1, a = t + 1.0f;
// otherwise x0 = X, a = t.  a lies in [0, 1); x0 in [-1, res - 1].  s == 1: t = 0, the pixel itself with weight 1.  An odd
// s has a column i = (s - 1) / 2 with t = 0 exactly, whose second tap has b == 0.
YK_HD void up_axis(uint32_t X, uint32_t i, uint32_t s, int& x0, float& a) {
    const float t = (float)((int)(2u * i + 1u) - (int)s) / (float)(2u * s);
    const bool before = t < 0.0f;
    x0 = before ? (int)X - 1 : (int)X;
    a = before ? t + 1.0f : t;
}

// Low pixel Q, once per pixel: c_Q is the low film's RGB, normalised by the LOW film's sample table where one is given
// (dn_normalise with count = dn_count on the low grid; no table: count 0, the bits are copied), then — with albedo — each
// channel divided by al_divisor of Q's low albedo record (al_demodulate).
YK_HD void up_low_colour(float count, const float* low_albedo, float* c) {
    dn_normalise(count, c);
    if (low_albedo) al_demodulate(low_albedo, c);
}

// One full pixel P = (s*X + i, s*Y + j) whose FULL guide is (nsP, hitP, pP).  fetch(qx, qy, tap) reads low pixel Q inside
// the low film: c = c_Q as above, and Q's LOW guide (a DnTap: yk_denoise.h's).  out = (r, g, b, sw).
//   Taps: (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with b = (1 - ax | ax) * (1 - ay | ay), accumulated in that order.
//   A tap is skipped — its colour neither multiplied nor added — when
//     1. it lies outside the low film;
//     2. b == 0;
//     3. the hit class of P's full guide differs from that of Q's low guide (hit != 0 against hit != 0);
//     4. a channel of c_Q is NaN or infinite;
//     5. its weight w is 0 or NaN.
//   Weight: two hits: (a_n, a_p) = dn_stops(P, Q) under den_n and den_p, e = a_n + a_p, w = b * det_expf(-e);
//           two misses: w = b.
//   All four taps are fetched before the first is consumed: the skip conditions select what is accumulated, not what is
//   requested.  A tap outside the film is requested at the clamped index — the nearest pixel inside, which is another tap
//   of the same footprint — and what comes back is dropped: no load stands under a branch.
//   Output: sw = sum w;  sw != 0: rgb = dn_canon(sum(w * c_Q) / sw) per channel;  sw == 0 (every tap skipped): rgb = c of
//   the containing low pixel (X, Y), as bits — it is always one of the four taps, and always inside.  With albedo each
//   channel is then multiplied by al_divisor of P's FULL albedo record (al_remodulate), the fallback's too.
//   out[3] = sw: 0 exactly where the fallback ran.
template <class Fetch>
YK_HD void up_pixel(const UpParams& a, uint32_t X, uint32_t i, uint32_t Y, uint32_t j, const float* nsP, float hitP, const float* pP, const float* albedoP, const Fetch& fetch, float* out) {
    int x0, y0;
    float ax, ay;
    up_axis(X, i, a.s, x0, ax);
    up_axis(Y, j, a.s, y0, ay);
    const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay};
    DnTap Q[4];
    bool inside[4];
    const int mx = (int)a.dn.res_x - 1, my = (int)a.dn.res_y - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        inside[k] = qx >= 0 && qy >= 0 && qx <= mx && qy <= my;
        fetch((uint32_t)(qx < 0 ? 0 : (qx > mx ? mx : qx)), (uint32_t)(qy < 0 ? 0 : (qy > my ? my : qy)), Q[k]);
    }
    const bool hp = hitP != 0.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float b = wx[k & 1] * wy[k >> 1];
        const bool hq = Q[k].hit != 0.0f;
        const DnStops g = dn_stops(a.dn, hp, nsP, pP, Q[k].ns, Q[k].p);
        const float e = g.a_n + g.a_p;
        const float x = det_expf(-e);
        const float bx = b * x;
        const float w = hp ? bx : b;
        const bool finite = tp_finite(Q[k].c[0]) && tp_finite(Q[k].c[1]) && tp_finite(Q[k].c[2]);
        if (!inside[k] || b == 0.0f || hp != hq || !finite || w == 0.0f || w != w) continue;
        const float pr = w * Q[k].c[0], pg = w * Q[k].c[1], pb = w * Q[k].c[2];
        sr = sr + pr;
        sg = sg + pg;
        sb = sb + pb;
        sw = sw + w;
    }
    const int own = (x0 == (int)X ? 0 : 1) + (y0 == (int)Y ? 0 : 2);  // the tap that is the containing low pixel
    float c0 = Q[0].c[0], c1 = Q[0].c[1], c2 = Q[0].c[2];
#pragma unroll
    for (int k = 1; k < 4; ++k) {  // a select, not an index: the taps stay in registers
        c0 = own == k ? Q[k].c[0] : c0;
        c1 = own == k ? Q[k].c[1] : c1;
        c2 = own == k ? Q[k].c[2] : c2;
    }
    if (sw != 0.0f) {
        c0 = dn_canon(sr / sw);
        c1 = dn_canon(sg / sw);
        c2 = dn_canon(sb / sw);
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    if (albedoP) al_remodulate(albedoP, out);
    out[3] = sw;
}

}  // namespace yk
