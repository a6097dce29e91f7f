// yk_rectify.h — history rectification: the carried history of a pixel is clipped to what the CURRENT frame shows around
// it, before yk_history_blend folds that frame in.  Reprojection (yk_temporal.h) carries radiance that was right for the
// previous view, the previous lighting and the previous positions; nothing else in the chain compares it with the frame
// at hand.  Here the (2 radius + 1)^2 pixels of the current film around P give a per-channel box mean +- gamma * sigma; a
// history outside the box is moved to its edge and its count n is scaled by how far it was moved, so the next blend weighs
// the new samples accordingly (the neighbourhood clip of interactive renderers: Karis, "High Quality Temporal
// Supersampling", SIGGRAPH 2014 course; Salvi, "An Excursion in Temporal Supersampling", GDC 2016, for the variance box).
//
// The reference has no temporal pass, so this file is the rule.  Its arithmetic is yk_denoise.h's and yk_temporal.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), division and sqrtf correctly
//     rounded (yk_math.h, at `length`, says why that holds on gfx950);
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and k_rectify (yk_rectify.hip) call rc_pixel below and agree bit
// for bit.
//
// Limits: the box is per channel in RGB (no chroma space); a history that is wrong but lies inside the current frame's
// noise box stays; the moments' m1 and m2 are not rectified — after a clip they describe the old radiance until new frames
// outweigh them (their count and frames shrink with the history's, so that is soon); yk_multi scenes are not served.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_denoise.h"
#include "yk_temporal.h"

namespace yk {

enum : uint32_t { RC_MAX_RADIUS = 3 };

// the window loops unroll where the radius is a compile-time constant: in the kernels, not in the host instance
#if defined(__HIP_DEVICE_COMPILE__)
#define RC_UNROLL _Pragma("unroll")
#else
#define RC_UNROLL
#endif

// Everything about a call that does not depend on the pixel.  dn carries the film's resolution and the sample table's index
// rule; its sigmas are not used.
struct RcParams {
    DnParams dn;
    int radius;
    float gamma;
};
// radius 1 .. 3; gamma >= 0, +inf included (every pixel then passes through), NaN refused.
inline bool rc_desc_ok(const yk_rectify_desc* d) { return d && d->radius >= 1 && d->radius <= RC_MAX_RADIUS && d->gamma >= 0.0f; }
inline RcParams rc_make_params(const yk_rectify_desc* d, uint32_t res_x, uint32_t res_y, uint32_t tile_dim) {
    RcParams a{};
    dn_set_grid(a.dn, res_x, res_y, tile_dim);
    a.radius = (int)d->radius;
    a.gamma = d->gamma;
    return a;
}

// What a tap reads of film pixel (x, y), inside the film: t = (r, g, b, m) as yk_history_blend sees the pixel — m =
// (float)samples[tm_sample_index] with a table and 1 without, the colour through dn_normalise(m, .) with a table and as
// its bits without.
YK_HD void rc_tap(const DnParams& a, const float* film, const uint32_t* samples, uint32_t x, uint32_t y, float* t) {
    const size_t q = (size_t)y * a.res_x + x;
    t[0] = film[3 * q];
    t[1] = film[3 * q + 1];
    t[2] = film[3 * q + 2];
    t[3] = 1.0f;
    if (samples) {
        t[3] = dn_count(a, samples, x, y);
        dn_normalise(t[3], t);
    }
}
// A tap inside the film is taken iff its pixel has samples and a finite colour.  Every test is evaluated, in every window
// that holds the pixel: folding the answer into m once per film pixel, where the tap is made, was measured and is SLOWER on
// gfx950 (69.4 us against 59.2 us at radius 2, 1920 x 1080).
YK_HD bool rc_take(const float* t) { return ((int)(t[3] != 0.0f) & (int)tp_finite(t[0]) & (int)tp_finite(t[1]) & (int)tp_finite(t[2])) != 0; }

// The presence of a record by the blends' own test (tp_blend_pixel, vr_moments_pixel): n > 0 — which a NaN is not — and
// the three other fields finite.  max_history does not enter: the clamp cannot make a positive count absent.
YK_HD bool rc_present(const float* h) { return h[3] > 0.0f && tp_finite(h[0]) && tp_finite(h[1]) && tp_finite(h[2]); }

// One pixel P = (x, y) with history record h.  fetch(qx, qy, t) gives rc_tap of a pixel inside the film; RADIUS > 0 fixes
// the window at compile time (the loops unroll), RADIUS == 0 takes a.radius.  Returns whether the history was clipped; out
// is then the new record and f the factor its count was scaled by, otherwise out is h's 16 bytes and f = 1.
//   taps:   dy = -radius .. radius outside, dx inside; a tap outside the film is never fetched; k counts the taken ones;
//   pass-through: the history absent (rc_present), k < 2, a mu or an e not finite, or no channel outside its box;
//   per channel, over the taken taps in tap order:  S = sum c (sequential), mu = S / (float)k, V = sum (c - mu)(c - mu),
//           sigma = sqrtf(V / (float)k), e = gamma * sigma, lo = mu - e, hi = mu + e;
//   clip:   out_c = h_c < lo ? lo : (h_c > hi ? hi : h_c) — an unclipped channel keeps its bits;  for a clipped channel
//           f_c = e / |h_c - mu|.  The divisor is >= e (rounding is monotonic and h_c lies beyond the rounded edge) and not
//           zero (h_c != mu, and a difference of two floats that differ is not 0), so f_c is in [0, 1];  f = the least f_c;
//   count:  n' = n * f: what the clip threw away of the history.  n' == 0 makes the history absent for the blend.
// gamma = +inf gives e = +inf, or NaN where sigma is 0: not finite, the pixel passes through.
// The window is walked twice, so fetch must be cheap: the host instance reads a table of taps, the kernel LDS.
template <int RADIUS, class Fetch>
YK_HD bool rc_pixel(const RcParams& a, uint32_t x, uint32_t y, const float* h, const Fetch& fetch, float* out, float& f) {
    out[0] = h[0];
    out[1] = h[1];
    out[2] = h[2];
    out[3] = h[3];
    f = 1.0f;
    if (!rc_present(h)) return false;
    const int R = RADIUS > 0 ? RADIUS : a.radius;
    const int mx = (int)a.dn.res_x - 1, my = (int)a.dn.res_y - 1;
    int k = 0;
    float S[3] = {0.0f, 0.0f, 0.0f};
    RC_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = (int)y + dy;
        RC_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qy < 0 || qx > mx || qy > my) continue;
            float t[4];
            fetch((uint32_t)qx, (uint32_t)qy, t);
            if (!rc_take(t)) continue;
            S[0] = S[0] + t[0];
            S[1] = S[1] + t[1];
            S[2] = S[2] + t[2];
            ++k;
        }
    }
    if (k < 2) return false;
    const float kf = (float)k;
    const float mu[3] = {S[0] / kf, S[1] / kf, S[2] / kf};
    float V[3] = {0.0f, 0.0f, 0.0f};
    RC_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = (int)y + dy;
        RC_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qy < 0 || qx > mx || qy > my) continue;
            float t[4];
            fetch((uint32_t)qx, (uint32_t)qy, t);
            if (!rc_take(t)) continue;
            const float dr = t[0] - mu[0], dg = t[1] - mu[1], db = t[2] - mu[2];
            const float rr = dr * dr, gg = dg * dg, bb = db * db;
            V[0] = V[0] + rr;
            V[1] = V[1] + gg;
            V[2] = V[2] + bb;
        }
    }
    float e[3];
    bool finite = true;
    RC_UNROLL
    for (int c = 0; c < 3; ++c) {
        const float var = V[c] / kf;
        const float sigma = sqrtf(var);
        e[c] = a.gamma * sigma;
        finite = finite && tp_finite(mu[c]) && tp_finite(e[c]);
    }
    if (!finite) return false;
    bool clipped = false;
    float fm = 1.0f, o[3];
    RC_UNROLL
    for (int c = 0; c < 3; ++c) {
        const float lo = mu[c] - e[c], hi = mu[c] + e[c];
        const bool below = h[c] < lo, above = h[c] > hi;
        o[c] = below ? lo : (above ? hi : h[c]);
        if (below || above) {
            const float d = h[c] - mu[c];
            const float fc = e[c] / fabsf(d);
            fm = fc < fm ? fc : fm;
            clipped = true;
        }
    }
    if (!clipped) return false;
    out[0] = o[0];
    out[1] = o[1];
    out[2] = o[2];
    out[3] = dn_canon(h[3] * fm);
    f = fm;
    return true;
}

// The moments record beside a history that rc_pixel clipped by f to the count n1: where the record is present (rc_present:
// the rule of vr_moments_pixel) its count becomes n1 — the history's, bit for bit, as yk_moments_blend keeps them — and its
// frames are scaled by f, the scaling vr_moments_pixel applies for its own clamp; m1 and m2 keep their bits.  An absent
// record is copied.
YK_HD void rc_moments(const float* m, float f, float n1, float* out) {
    out[0] = m[0];
    out[1] = m[1];
    out[2] = m[2];
    out[3] = m[3];
    if (!rc_present(m)) return;
    out[2] = dn_canon(m[2] * f);
    out[3] = n1;
}

}  // namespace yk
