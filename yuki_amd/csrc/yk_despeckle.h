// yk_despeckle.h — despeckle: a pixel of the CURRENT frame's film that is far brighter than everything around it is scaled
// down to a bound its neighbourhood sets, before anything else in the film chain reads it.  Such an outlier enters
// yk_history_blend at full weight, widens the box yk_history_rectify clips against, inflates the luminance moments and
// survives the à-trous filter (its own tap always weighs 1, its neighbours' colour stop rejects them); this pass stands
// in front of all of them.  The bound is a rank-conditioned one: the rank-th largest luminance among the other pixels of
// the (2 radius + 1)^2 window, times a gain (the rank-order clamps of interactive path tracers, in front of the temporal
// accumulation).  The window reads the film and nothing else — no guides: windows starved of taps clamp real signal
// (as §7.14 found for the rectify window).
//
// The reference has no such pass, so this file is the rule.  Its arithmetic is yk_denoise.h's and yk_rectify.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), division correctly rounded;
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and k_despeckle (yk_despeckle.hip) call ds_pixel below and agree
// bit for bit.
//
// Limits: biased by design — it removes energy from heavy-tailed light transport and is not for a film meant to converge;
// luminance only (the chromaticity of a clamped pixel is kept, a saturated but dim channel is not seen); a real glint
// narrower than the window's rank is clamped like a firefly; yk_multi scenes are not served.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_denoise.h"
#include "yk_rectify.h"
#include "yk_temporal.h"
#include "yk_variance.h"

namespace yk {

enum : uint32_t { DS_MAX_RADIUS = 2, DS_MAX_RANK = 4 };
enum : uint8_t { DS_UNTOUCHED = 0, DS_CLAMPED = 1, DS_REPAIRED = 2 };  // the mask's values, and ds_pixel's return

// Everything about a call that does not depend on the pixel.  dn carries the film's resolution and the sample table's index
// rule; its sigmas are not used.
struct DsParams {
    DnParams dn;
    int radius;
    int rank;
    int need;  // max(min_taps, rank): fewer taken taps and the pixel passes through
    bool repair;
    float gain, floor;
};
// radius 1 .. 2; rank 1 .. 4; min_taps >= rank; no flag but YK_DESPECKLE_REPAIR; gain >= 0, +inf included, NaN refused;
// floor >= 0 and finite; a gain or a floor of -0 is taken as +0 (ds_make_params)
inline bool ds_desc_ok(const yk_despeckle_desc* d) {
    return d && d->radius >= 1 && d->radius <= DS_MAX_RADIUS && d->rank >= 1 && d->rank <= DS_MAX_RANK && d->min_taps >= d->rank && (d->flags & ~(uint32_t)YK_DESPECKLE_REPAIR) == 0 &&
           d->gain >= 0.0f && d->floor >= 0.0f && tp_finite(d->floor);
}
inline DsParams ds_make_params(const yk_despeckle_desc* d, uint32_t res_x, uint32_t res_y, uint32_t tile_dim) {
    DsParams a{};
    dn_set_grid(a.dn, res_x, res_y, tile_dim);
    a.radius = (int)d->radius;
    a.rank = (int)d->rank;
    a.need = (int)(d->min_taps > (uint32_t)INT32_MAX ? (uint32_t)INT32_MAX : d->min_taps);
    a.repair = (d->flags & YK_DESPECKLE_REPAIR) != 0;
    a.gain = d->gain + 0.0f;  // a -0 counts as +0: the bound, and with it s, never carries a sign
    a.floor = d->floor + 0.0f;
    return a;
}

// The four largest values seen so far, t[0] >= t[1] >= t[2] >= t[3], in four registers: a new value sinks through a
// compare-and-swap chain.  No indexed array, so nothing goes to scratch on the device.
struct DsTop4 {
    float t0, t1, t2, t3;
};
YK_HD DsTop4 ds_top_empty() {
    const float ninf = gl_from_bits(0xff800000u);
    return DsTop4{ninf, ninf, ninf, ninf};
}
YK_HD void ds_top_insert(DsTop4& s, float v) {
    bool g = v > s.t0;
    float hi = g ? v : s.t0;
    v = g ? s.t0 : v;
    s.t0 = hi;
    g = v > s.t1;
    hi = g ? v : s.t1;
    v = g ? s.t1 : v;
    s.t1 = hi;
    g = v > s.t2;
    hi = g ? v : s.t2;
    v = g ? s.t2 : v;
    s.t2 = hi;
    s.t3 = v > s.t3 ? v : s.t3;
}
// the rank-th largest (rank 1 .. 4), by selects
YK_HD float ds_top_rank(const DsTop4& s, int rank) { return rank == 1 ? s.t0 : (rank == 2 ? s.t1 : (rank == 3 ? s.t2 : s.t3)); }

// One pixel P = (x, y).  stored: P's three floats in the film; p = rc_tap of P (the colour normalised where the film is a
// sum, m_P in p[3]); has_table: whether a sample table was given.  fetch(qx, qy, t) gives rc_tap of a pixel inside the film;
// RADIUS > 0 fixes the window at compile time (the loops unroll), RADIUS == 0 takes a.radius.  Returns the mask value; out
// is the pixel of the output film, which uses the input's convention (a sum stays a sum).
//   1. m_P == 0: out = stored.
//   2. taps: the window without P, dy = -radius .. radius outside, dx inside; a tap outside the film is never fetched; a tap
//      is taken by rc_take (m_Q != 0, c_Q finite in all three channels); l_Q = vr_luminance(c_Q); k counts the taken ones.
//      k < max(min_taps, rank): out = stored.
//   3. v = the rank-th largest l_Q as a multiset; a v that is not > 0 counts as +0 (see below); bound = gain * v, then
//      bound = floor where bound < floor.  A NaN bound (+inf * 0) passes P through: out = stored.
//   4. c_P finite in all three channels and l_P = vr_luminance(c_P) > bound: s = bound / l_P, out_c = stored_c * s per
//      channel, the mask is 1.  l_P > bound >= 0, so the divisor is positive; bound < l_P and a correctly rounded quotient
//      of two floats a < b is at most 1 - 2^-24, so s is in [0, 1) (0 where the bound is 0; the luminance of a finite colour is finite: the weights sum to 1).
//      c_P finite and l_P <= bound (or l_P NaN): out = stored.
//   5. c_P not finite: with repair, per channel the sequential sum of the taken taps' colours in tap order, divided by
//      (float)k, through dn_canon, and with a table multiplied by m_P (through dn_canon); the mask is 2.  Without repair
//      out = stored.
// The negative v of step 3: a window whose rank-th largest luminance is negative gives gain * v < 0 <= floor for every
// finite gain > 0, so the bound is `floor` whatever v was, and +0 gives the same.  It differs for gain = +inf, where -inf
// would be raised to the floor and clamp P, while +inf * 0 is the NaN that passes it through — which is what makes
// gain = +inf, floor = 0 the identity on EVERY film — and for gain = 0, where it keeps a -0 out of the bound.
// The window is walked once: the four largest luminances, the count and the three sums are kept along the way.
template <int RADIUS, class Fetch>
YK_HD uint8_t ds_pixel(const DsParams& a, bool has_table, uint32_t x, uint32_t y, const float* stored, const float* p, const Fetch& fetch, float* out) {
    out[0] = stored[0];
    out[1] = stored[1];
    out[2] = stored[2];
    if (p[3] == 0.0f) return DS_UNTOUCHED;
    const int R = RADIUS > 0 ? RADIUS : a.radius;
    const int mx = (int)a.dn.res_x - 1, my = (int)a.dn.res_y - 1;
    int k = 0;
    float S[3] = {0.0f, 0.0f, 0.0f};
    DsTop4 top = ds_top_empty();
    RC_UNROLL
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = (int)y + dy;
        RC_UNROLL
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qx = (int)x + dx;
            if (qx < 0 || qy < 0 || qx > mx || qy > my) continue;
            float t[4];
            fetch((uint32_t)qx, (uint32_t)qy, t);
            if (!rc_take(t)) continue;
            ds_top_insert(top, vr_luminance(t));
            S[0] = S[0] + t[0];
            S[1] = S[1] + t[1];
            S[2] = S[2] + t[2];
            ++k;
        }
    }
    if (k < a.need || k < a.rank) return DS_UNTOUCHED;
    float v = ds_top_rank(top, a.rank);
    v = v > 0.0f ? v : 0.0f;
    float bound = a.gain * v;
    bound = bound < a.floor ? a.floor : bound;
    if (bound != bound) return DS_UNTOUCHED;
    const bool finite = (((int)tp_finite(p[0]) & (int)tp_finite(p[1]) & (int)tp_finite(p[2])) != 0);
    if (finite) {
        const float lp = vr_luminance(p);
        if (!(lp > bound)) return DS_UNTOUCHED;
        const float s = bound / lp;
        out[0] = stored[0] * s;
        out[1] = stored[1] * s;
        out[2] = stored[2] * s;
        return DS_CLAMPED;
    }
    if (!a.repair) return DS_UNTOUCHED;
    const float kf = (float)k;
    RC_UNROLL
    for (int c = 0; c < 3; ++c) {
        float m = dn_canon(S[c] / kf);
        if (has_table) m = dn_canon(m * p[3]);
        out[c] = m;
    }
    return DS_REPAIRED;
}

}  // namespace yk
