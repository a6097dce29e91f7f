// yk_variance.h — variance-guided denoise: per-pixel luminance moments carried beside the temporal history, a variance
// image made from them, and an à-trous filter whose colour stop is scaled by that variance (after Schied et al.,
// "Spatiotemporal Variance-Guided Filtering", HPG 2017).  yk_denoise's colour stop sigma_color / 2^i knows nothing about
// how noisy a pixel is: a film blended from many frames gets the blur of a film of one.  Here the stop closes as the
// carried film converges.
//
// The reference has no denoiser, so this file is the rule.  Its arithmetic is yk_denoise.h's and yk_temporal.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), divisions correctly rounded,
//     exp is det_expf;
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and the gfx950 kernels (yk_variance.hip: the moments and the
// variance image; yk_denoise.hip: the filter) call the functions below and agree bit for bit.
//
// The moments record yk_moments (m1, m2, frames, n) has the layout of yk_history (rgb[3], n) ON PURPOSE: a moments
// buffer is reprojected by yk_history_reproject[_device] and yk_history_reproject_moved[_device] as they are, cast to
// yk_history.  It gets the same taps, the same bilinear weights and the same skip set as the colour history beside it
// (tp_take reads n > 0 and the finiteness of the three other fields, which is what the presence rule below reads too), and
// m1, m2 and frames are interpolated like colours — all three are linear in what they average.
//
// Limits: the variance is that of LUMINANCE only (a pixel noisy in chroma alone looks converged); yk_multi scenes are not
// served; the temporal estimate inherits what lag yk_rectify.h leaves the history on glass and metal (it shrinks the
// moments' count with the history's; m1 and m2 it does not touch).
#pragma once
#include "yk_albedo.h"
#include "yk_denoise.h"
#include "yk_temporal.h"

namespace yk {

// Everything about a call that depends on neither the pixel nor the iteration.  dn carries the film's resolution, the
// sample table's index rule and den_n / den_p; its sigma_color is not used.
struct VrParams {
    DnParams dn;
    float sv2;  // sigma_variance * sigma_variance
    float epsilon, spatial_scale;
};
// What yk_variance and yk_denoise_variance ask of their descriptor, and the parameters it makes.
inline bool vr_desc_ok(const yk_variance_desc* d) {
    if (!d || !dn_desc_ok(d->iterations, d->sigma_variance, d->sigma_normal, d->sigma_plane)) return false;
    return d->epsilon >= 0.0f && d->spatial_scale >= 0.0f;  // < 0 or NaN
}
inline VrParams vr_make_params(const yk_variance_desc* d, uint32_t res_x, uint32_t res_y, uint32_t tile_dim) {
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

// Luminance: fixed Rec. 709 weights as exact float literals, products first, summed left to right.
YK_HD float vr_luminance(const float* c) {
    const float pr = 0.2126f * c[0], pg = 0.7152f * c[1], pb = 0.0722f * c[2];
    return dn_canon((pr + pg) + pb);
}

// ---- moments blend (yk_moments_blend), one pixel: tp_blend_pixel's sibling.
// c: the film's RGB, normalised exactly as tp_blend_pixel normalises it (with a table and m > 0, dn_normalise);
// l = vr_luminance(c), ll = l * l.  h: the reprojected moments, or NULL.  out = (m1, m2, frames, n):
//   history:  n = min(h.n, max_history), a NaN staying a NaN; absent when h is NULL, n is <= 0 or NaN, or one of h.m1, h.m2,
//             h.frames is not finite (tp_blend_pixel's presence rule on the same four words);
//   current:  absent when m == 0 (tp_blend_pixel's rule) — or when ll is NaN or infinite (l is NaN or infinite, or its
//             square overflows).  This is the one case the colour blend does not have: there a non-finite pixel makes the
//             record non-finite and the next blend drops it; here it is dropped at once, so the moments a pixel has are
//             kept and a non-finite sample never enters them;
//   both absent: zeros;   only the history absent: (l, ll, 1, m);
//   only the current view absent: (h.m1, h.m2 as bits, h.frames * r, n) with r = n / h.n, the clamp's scale (1 when it did
//             not clamp);
//   neither:  t = n + m;  m1 = (n*h.m1 + m*l) / t;  m2 = (n*h.m2 + m*ll) / t;  frames = h.frames * r + 1: the clamp scales
//             the effective number of frames as it scales the number of samples.  t is yk_history_blend's count for the
//             same inputs, bit for bit (the same n, the same m, the same sum).
YK_HD void vr_moments_pixel(const TpParams& a, bool has_table, float m, const float* c_in, const float* h, float* out) {
    float c[3] = {c_in[0], c_in[1], c_in[2]};
    if (has_table) dn_normalise(m, c);
    const float l = vr_luminance(c);
    const float ll = dn_canon(l * l);
    const bool cur = m != 0.0f && tp_finite(ll);
    float n = 0.0f, r = 0.0f;
    bool hist = false;
    if (h) {
        n = h[3] > a.max_history ? a.max_history : h[3];
        hist = n > 0.0f && tp_finite(h[0]) && tp_finite(h[1]) && tp_finite(h[2]);
        r = dn_canon(n / h[3]);
    }
    if (!hist) {
        out[0] = cur ? l : 0.0f;
        out[1] = cur ? ll : 0.0f;
        out[2] = cur ? 1.0f : 0.0f;
        out[3] = cur ? m : 0.0f;
        return;
    }
    const float fr = dn_canon(h[2] * r);
    if (!cur) {
        out[0] = h[0];
        out[1] = h[1];
        out[2] = fr;
        out[3] = n;
        return;
    }
    const float t = n + m;
    const float a1 = n * h[0], b1 = m * l;
    const float s1 = a1 + b1;
    const float a2 = n * h[1], b2 = m * ll;
    const float s2 = a2 + b2;
    out[0] = dn_canon(s1 / t);
    out[1] = dn_canon(s2 / t);
    out[2] = dn_canon(fr + 1.0f);
    out[3] = t;
}

// ---- the variance image (yk_variance): one float a pixel, the estimated variance of the luminance of the film that will
// be filtered.
//
// Temporal estimate, where the moments are present (n > 0, the three other fields finite) and frames >= 2.  The moments
// are sample-weighted means over K = frames frames of m_k samples each, t = sum m_k: m1 = sum(m_k l_k) / t and
// m2 = sum(m_k l_k^2) / t, with l_k the frame means, each of variance sigma^2 / m_k around the true mean mu.  Then
//   E[m2] = mu^2 + sigma^2 K / t   and   E[m1^2] = mu^2 + sigma^2 / t,
// so S = max(0, m2 - m1*m1) has expectation sigma^2 (K - 1) / t, and the variance of the blended mean m1 — the film that
// is filtered — is sigma^2 / t.  Hence var = S / (frames - 1).
// With an albedo the filter runs on radiance / divisor, so var is divided by dl*dl, dl = vr_luminance of the pixel's own
// three divisors (al_divisor, the floor included).  That is an APPROXIMATION: luminance(c / d) is dl-proportional to
// luminance(c) only where the three divisors are equal (a grey albedo); on a coloured texel the channels are scaled
// differently and the true variance of the demodulated luminance depends on the covariance of the channels, which the
// moments do not carry.
// Returns false where the temporal estimate does not apply.
YK_HD bool vr_temporal(const float* h, const float* albedo, float& var) {
    if (!h) return false;
    const bool ok = h[3] > 0.0f && tp_finite(h[0]) && tp_finite(h[1]) && tp_finite(h[2]) && h[2] >= 2.0f;
    if (!ok) return false;
    const float sq = h[0] * h[0];
    float S = h[1] - sq;
    S = S > 0.0f ? S : 0.0f;
    const float k = h[2] - 1.0f;
    float v = S / k;
    if (albedo) {
        const float d[3] = {al_divisor(albedo[0]), al_divisor(albedo[1]), al_divisor(albedo[2])};
        const float dl = vr_luminance(d);
        const float dd = dl * dl;
        v = v / dd;
    }
    var = dn_canon(v);
    return true;
}

// What a tap of the spatial window reads of a pixel: its guide record and the luminance l of its colour — the film's RGB
// after dn_normalise and, with an albedo, al_demodulate with the tap's OWN albedo (vr_tap_luminance).
struct VrTap {
    float ns[3];
    float hit;
    float p[3];
    float l;
};
YK_HD float vr_tap_luminance(const DnParams& a, const float* film, const uint32_t* samples, const float* albedo_or_null, uint32_t x, uint32_t y) {
    const size_t i = (size_t)y * a.res_x + x;
    float c[3] = {film[3 * i], film[3 * i + 1], film[3 * i + 2]};
    dn_normalise(dn_count(a, samples, x, y), c);
    if (albedo_or_null) al_demodulate(albedo_or_null + 4 * i, c);
    return vr_luminance(c);
}

// The geometric part of dn_weight's exponent for taps of one hit class: a_n + a_p for two hits, 0 for two misses.
YK_HD float vr_geometry(const DnParams& a, bool hit, const float* nsP, const float* pP, const float* nsQ, const float* pQ) {
    const DnStops g = dn_stops(a, hit, nsP, pP, nsQ, pQ);
    return g.a_n + g.a_p;
}

// Spatial estimate, everywhere else (the first frame, disocclusions, no moments): the weighted variance of l over the
// 7 x 7 window, dy = -3..3 outside, dx = -3..3 inside, accumulated in that order.  The centre has weight 1 and is always
// taken.  Any other tap Q has w = exp(-(a_n + a_p)) — dn_weight's normal and plane stops, the same hit / miss rule, no
// colour stop, no kernel.  The closed set of skipped taps:
//   1. Q lies outside the film (never read);
//   2. one of P, Q is a hit and the other a miss;
//   3. w is 0 or NaN (a guide is not finite, a denominator is 0, the exponent overflows exp to 0);
//   4. l_Q * l_Q is NaN or infinite (l_Q is not finite, or its square overflows).
// s0 = sum w, s1 = sum(w * l), s2 = sum(w * l*l);  mean = s1 / s0;  S = max(0, s2 / s0 - mean*mean);
// var = S * spatial_scale.  (On a constant neighbourhood S is 0 or the rounding of the two quotients, a few ulp of l*l.)  A centre whose luminance is not finite makes S a NaN, which max(0, .) turns into 0.
template <class Fetch>
YK_HD float vr_spatial_pixel(const VrParams& a, uint32_t x, uint32_t y, const Fetch& fetch) {
    VrTap P;
    fetch(x, y, P);
    const bool hp = P.hit != 0.0f;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)a.dn.res_y) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)a.dn.res_x) continue;
            float w = 1.0f;
            VrTap Q = P;
            if (dx != 0 || dy != 0) {
                fetch((uint32_t)qx, (uint32_t)qy, Q);
                if ((Q.hit != 0.0f) != hp) continue;
                const float e = vr_geometry(a.dn, hp, P.ns, P.p, Q.ns, Q.p);
                w = det_expf(-e);
                if (w == 0.0f || w != w) continue;
            }
            const float ll = Q.l * Q.l;
            if ((dx != 0 || dy != 0) && !tp_finite(ll)) continue;
            const float p1 = w * Q.l, p2 = w * ll;
            s0 = s0 + w;
            s1 = s1 + p1;
            s2 = s2 + p2;
        }
    }
    const float mean = s1 / s0, m2 = s2 / s0;
    const float sq = mean * mean;
    float S = m2 - sq;
    S = S > 0.0f ? S : 0.0f;  // a NaN as well
    return dn_canon(S * a.spatial_scale);
}

// What yk_variance stores and what yk_denoise_variance reads of a variance: NaN or negative becomes 0; +inf stays +inf
// and switches the colour stop off for that pixel.
YK_HD float vr_sanitise(float v) { return v >= 0.0f ? v : 0.0f; }

// ---- the filter (yk_denoise_variance): dn_pixel with a variance-scaled colour stop and a propagated variance.
// A colour record is (r, g, b, var).  What a tap reads of a pixel:
struct VrFilterTap {
    DnTap t;
    float var;
};

// The 3 x 3 Gaussian k = (1/2, 1/4) by |offset| (weights 1/4, 1/8, 1/16) of the previous iteration's variance around P at
// UNIT spacing whatever the step, over the taps inside the film whose variance is finite, renormalised by their weights:
// g = sum(k * var) / sum(k), dy = -1..1 outside, dx = -1..1 inside.  var_P not finite (+inf; the records hold no NaN):
// g = +inf without looking at the neighbours — an infinite variance opens the colour stop of ITS pixel and of no other.
// fetch_var(qx, qy) reads the variance of a pixel inside the film.
template <class FetchVar>
YK_HD float vr_gauss(const DnParams& a, uint32_t x, uint32_t y, float var_p, const FetchVar& fetch_var) {
    if (!tp_finite(var_p)) return __builtin_inff();
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)a.res_y) continue;
        const float ky = dy == 0 ? 0.5f : 0.25f;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)a.res_x) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * ky;
            const float v = (dx == 0 && dy == 0) ? var_p : fetch_var((uint32_t)qx, (uint32_t)qy);
            if (!tp_finite(v)) continue;
            const float kv = k * v;
            gs = gs + kv;
            gw = gw + k;
        }
    }
    return dn_canon(gs / gw);  // the centre is finite here: gw >= 1/4
}

// The denominator of the colour stop of pixel P: sigma_variance^2 * g + epsilon, two operations; +inf when sigma_variance
// is +inf (the stop is off whatever g is, a g of 0 included).  There is no / 2^i: the propagated variance shrinks instead.
YK_HD float vr_color_denominator(const VrParams& a, float g) {
    if (a.sv2 == __builtin_inff()) return a.sv2;
    const float sg = a.sv2 * g;
    return dn_canon(sg + a.epsilon);
}

// The weight of tap Q for pixel P: dn_weight with a_c = (dl*dl) / den_c, dl = l_P - l_Q the difference of the luminances of
// the two colours of the previous iteration.  Everything else is dn_weight's, its skip set included: the caller skips a
// weight of 0 or NaN — a hit against a miss; e NaN or +inf (a luminance is NaN or infinite or dl*dl overflows, a guide is not
// finite, a denominator is 0, inf / inf); exp(-e) underflows to 0.
YK_HD float vr_weight(const DnParams& a, float den_c, float h, const DnTap& P, float lP, const DnTap& Q, float lQ) {
    const bool hp = P.hit != 0.0f, hq = Q.hit != 0.0f;
    if (hp != hq) return 0.0f;
    const float dl = lP - lQ;
    const float d2 = dl * dl;
    const float a_c = d2 / den_c;
    const DnStops g = dn_stops(a, hp, P.ns, P.p, Q.ns, Q.p);
    const float e = (a_c + g.a_n) + g.a_p;
    const float x = det_expf(-e);
    return h * x;
}

// One pixel of one iteration with step s.  fetch(qx, qy, tap) reads a pixel inside the film, fetch_var its variance alone.
// Taps, order, the B3 kernel h, the always-taken centre of weight h and the skip of a weight that is 0 or NaN are
// dn_pixel's.  out = (sum(w * c_Q) / sum(w) per channel, var'), each through dn_canon, with
//   var' = sum(w*w * var_Q) / (sum(w) * sum(w)) over the taken taps whose variance is finite, the sum of weights over ALL
//   taken taps;  var_P not finite: var' = var_P.  So an infinite variance stays where it is and does not spread.
// With every variance +inf (and epsilon, sigma_variance finite or not) this is dn_pixel with sigma_color = +inf, except
// that the tap test reads luminance where dn_weight reads the three channels: the two skip the same taps unless a
// channel difference squares to infinity while the luminance difference does not, or the other way round (finite channel
// values between about 1e18 and 1e20 next to ordinary ones).
template <class Fetch, class FetchVar>
YK_HD void vr_pixel(const VrParams& a, int s, uint32_t x, uint32_t y, const Fetch& fetch, const FetchVar& fetch_var, float* out) {
    VrFilterTap P;
    fetch(x, y, P);
    const float g = vr_gauss(a.dn, x, y, P.var, fetch_var);
    const float den_c = vr_color_denominator(a, g);
    const float lP = vr_luminance(P.t.c);
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + s * dy;
        if (qy < 0 || qy >= (int)a.dn.res_y) continue;
        const float ky = dn_kernel(dy);
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + s * dx;
            if (qx < 0 || qx >= (int)a.dn.res_x) continue;
            const float h = dn_kernel(dx) * ky;
            float w = h;
            VrFilterTap Q = P;
            if (dx != 0 || dy != 0) {
                fetch((uint32_t)qx, (uint32_t)qy, Q);
                w = vr_weight(a.dn, den_c, h, P.t, lP, Q.t, vr_luminance(Q.t.c));
                if (w == 0.0f || w != w) continue;
            }
            const float pr = w * Q.t.c[0], pg = w * Q.t.c[1], pb = w * Q.t.c[2];
            sr = sr + pr;
            sg = sg + pg;
            sb = sb + pb;
            sw = sw + w;
            if (tp_finite(Q.var)) {
                const float ww = w * w;
                const float pv = ww * Q.var;
                sv = sv + pv;
            }
        }
    }
    out[0] = dn_canon(sr / sw);
    out[1] = dn_canon(sg / sw);
    out[2] = dn_canon(sb / sw);
    const float sw2 = sw * sw;
    out[3] = tp_finite(P.var) ? dn_canon(sv / sw2) : P.var;
}

}  // namespace yk
