// yk_exposure.h — the exposure meter: what a film's luminances say the tone map's exposure should be, on the host and on gfx950.
//
// The reference has no meter (FilmicParams.exposure is a slider, tonemap.rs:12-22); this is the project's own rule, fixed so
// that the host and the device instance cannot differ through scheduling or a libm:
//   - the film becomes INTEGER counts in a 256-bin histogram indexed by the bit pattern of each pixel's luminance — the bit
//     pattern of a binary32 is its log2, piecewise linear, so there is no logf;
//   - the percentile cut and the mean over the kept samples are integer arithmetic (uint32 counts, an int64 sum) up to one
//     division: any order of adding the counts gives the same words;
//   - what follows is two binary64 operations and a handful of binary32 ones, every operation separate (the library is built
//     with -ffp-contract=off), written once here for both instances (the yk_tonemap.h pattern).
// The rule, in the order it is applied:
//   pixel    r, g, b each divided by (float)samples[tm_sample_index(x, y, tile_dim, res_x / tile_dim)] when that count is
//            > 0 — step 1 of tm_filmic, the floor / ceil quirk of the lookup included, so the meter sees what the tone map
//            will map; Y = tm_luminance(r, g, b).
//   skip     Y not finite, or Y <= 0 (a miss on a black background says nothing about exposure): counted in `skipped` and
//            nowhere else.
//   bin      u = bits(Y); bin = clamp((u >> 20) - 888, 0, 255): the exponent and three mantissa bits, eight bins to a stop
//            over 2^-16 <= Y < 2^16.  Below that (subnormals included): bin 0 and `below`; above: bin 255 and `above`.
//   value    v(bin) = ((bin >> 3) - 16) * 65536 + Q[bin & 7], stops in Q16; Q[m] = round(65536 * log2(1 + (m + 0.5) / 8)).
//            v(bin) is at most log2(17/16) = 0.0875 stop from the log2 of any luminance of the bin: the meter's resolution.
//   window   {x0, y0, x1, y1}, half open; pixels outside are neither counted nor skipped.
//   cut      N = sum of the bins; n_lo = (uint64(N) * low_cut) >> 16, n_hi = (uint64(N) * high_cut) >> 16 (cuts in 1/65536,
//            low_cut + high_cut < 65536, so one sample at least is kept when N >= 1).  Kept: the ranks [n_lo, N - n_hi) in
//            bin order; a bin cut by a boundary gives the integer part inside:
//            kept_b = clamp(cum_b, n_lo, N - n_hi) - clamp(cum_{b-1}, n_lo, N - n_hi).
//            S = sum kept_b * v(b) (int64, |S| <= 2^32 * 16 * 65536 = 2^52), K = sum kept_b.
//   metered  log2_metered = (float)((double)S / ((double)K * 65536.0)).
//   adapt    no previous state or prev.frames == 0: log2_adapted = log2_metered.  Else d = log2_metered - prev.log2_adapted,
//            rate = d > 0 ? adapt_up : adapt_down, log2_adapted = prev.log2_adapted + d * rate; frames = prev.frames + 1,
//            saturating.  The caller turns a time step into a rate (1 - e^(-dt/tau)); the library takes no clock.
//   empty    N == 0: the state is carried, log2_metered = log2_adapted = prev.log2_adapted, frames = prev.frames; without
//            history log2_adapted = log2_metered = ev_bias and frames = 0, which gives exposure 1.
//   exposure stops = ev_bias - log2_adapted clamped to [min_ev, max_ev] (NaN -> min_ev, the style of tm_saturate);
//            exposure = ex_exp2(stops).
#pragma once
#include <string.h>

#include "../../include/yuki_hip.h"
#include "yk_tonemap.h"

namespace yk {

constexpr uint32_t EX_BINS = 256;
// the words of a histogram slot: the bins, then skipped, below, above (and one of padding)
enum : uint32_t { EX_SKIPPED = 256, EX_BELOW = 257, EX_ABOVE = 258, EX_SLOT_WORDS = 260 };

YK_HD uint32_t ex_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}
YK_HD float ex_float(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}

// The luminance the meter sees: step 1 of tm_filmic, then tm_luminance.  `count` is (float)samples[flat], 0 without a table.
YK_HD float ex_pixel_luminance(float count, float r, float g, float b) {
    if (count > 0.0f) {
        r = r / count;
        g = g / count;
        b = b / count;
    }
    return tm_luminance(r, g, b);
}

// The pixel's slot word: its bin, or EX_SKIPPED for the skip set; *edge: EX_BELOW / EX_ABOVE when the bin was clamped, else 0.
// Y > 0 is false for NaN, zeros and negatives; 0x7F800000 is +inf.
YK_HD uint32_t ex_bin(float Y, uint32_t* edge) {
    *edge = 0;
    const uint32_t u = ex_bits(Y);
    if (!(Y > 0.0f) || u >= 0x7F800000u) return EX_SKIPPED;
    const int32_t e = (int32_t)(u >> 20) - 888;
    if (e < 0) {
        *edge = EX_BELOW;
        return 0;
    }
    if (e > 255) {
        *edge = EX_ABOVE;
        return 255;
    }
    return (uint32_t)e;
}

// v(bin) in Q16 stops
YK_HD int32_t ex_bin_value(uint32_t bin) {
    const int32_t Q[8] = {5732, 16248, 25711, 34312, 42196, 49472, 56229, 62534};
    return ((int32_t)(bin >> 3) - 16) * 65536 + Q[bin & 7];
}

// the ranks the cut keeps: [*n_lo, *n_top)
YK_HD void ex_cut(uint32_t N, uint32_t low_cut, uint32_t high_cut, uint32_t* n_lo, uint32_t* n_top) {
    *n_lo = (uint32_t)(((uint64_t)N * low_cut) >> 16);
    *n_top = N - (uint32_t)(((uint64_t)N * high_cut) >> 16);
}

// kept_b of a bin whose samples have the ranks [cum_before, cum)
YK_HD uint32_t ex_kept(uint32_t cum_before, uint32_t cum, uint32_t n_lo, uint32_t n_top) {
    const uint32_t a = cum_before < n_lo ? n_lo : (cum_before > n_top ? n_top : cum_before);
    const uint32_t b = cum < n_lo ? n_lo : (cum > n_top ? n_top : cum);
    return b - a;
}

// 2^x for -24 <= x <= 24 (the clamp of the rule guarantees it): i = floor(x), f = x - i in [0, 1), then
//   p(f) = 1 + f*(C1 + f*(C2 + f*(C3 + f*(C4 + f*C5))))   by Horner, every multiply and add separate,
// times the float whose bits are (127 + i) << 23.  The coefficients (binary32, exact as written):
//   C1 = 0x1.62e4bap-1  (0.6931512951850891)     C2 = 0x1.ebdb56p-3  (0.24016444385051727)
//   C3 = 0x1.c91ce6p-5  (0.05579991266131401)    C4 = 0x1.277854p-7  (0.009017029777169228)
//   C5 = 0x1.e974fep-10 (0.0018671302823349833)
// a degree-5 minimax fit of relative error with p(0) = 1 pinned, so that integers are exact.  Its relative error against
// float64 2^x, evaluated in binary32 as here, is 1.8e-7 at most over [-24, 24] (the requirement of use is 1e-5, three orders
// below the meter's own resolution).
YK_HD float ex_exp2(float x) {
    int32_t i = (int32_t)x;
    if ((float)i > x) i = i - 1;
    const float f = x - (float)i;
    float p = 0x1.e974fep-10f;
    p = p * f;
    p = p + 0x1.277854p-7f;
    p = p * f;
    p = p + 0x1.c91ce6p-5f;
    p = p * f;
    p = p + 0x1.ebdb56p-3f;
    p = p * f;
    p = p + 0x1.62e4bap-1f;
    p = p * f;
    p = p + 1.0f;
    return p * ex_float((uint32_t)(127 + i) << 23);
}

// The scalar tail of the rule: from the cut's sums (N samples counted, K kept, S their Q16 sum) and the slot's three side
// counts to the record.  `prev` may be NULL and may be `out`: it is read before `out` is written.
YK_HD void ex_finish(const yk_exposure_desc& d, uint32_t N, uint32_t K, int64_t S, uint32_t skipped, uint32_t below, uint32_t above, const yk_exposure_state* prev, yk_exposure_state* out) {
    const bool has_prev = prev != nullptr && prev->frames != 0;
    const float prev_adapted = prev ? prev->log2_adapted : 0.0f;
    const uint32_t prev_frames = prev ? prev->frames : 0u;
    float metered, adapted;
    uint32_t frames;
    if (N == 0) {
        adapted = has_prev ? prev_adapted : d.ev_bias;
        metered = adapted;
        frames = has_prev ? prev_frames : 0u;
    } else {
        const double den = (double)K * 65536.0;
        metered = (float)((double)S / den);
        if (!has_prev) {
            adapted = metered;
        } else {
            const float dl = metered - prev_adapted;
            const float rate = dl > 0.0f ? d.adapt_up : d.adapt_down;
            const float step = dl * rate;
            adapted = prev_adapted + step;
        }
        frames = prev_frames == 0xFFFFFFFFu ? prev_frames : prev_frames + 1u;
    }
    float stops = d.ev_bias - adapted;
    stops = stops > d.min_ev ? (stops < d.max_ev ? stops : d.max_ev) : d.min_ev;
    yk_exposure_state o;
    o.exposure = ex_exp2(stops);
    o.log2_adapted = adapted;
    o.log2_metered = metered;
    o.frames = frames;
    o.counted = N;
    o.skipped = skipped;
    o.below = below;
    o.above = above;
    *out = o;
}

// What a descriptor is refused for, or NULL: the message's tail, after the entry point's prefix.
inline const char* ex_desc_refusal(const yk_exposure_desc* d, uint16_t res_x, uint16_t res_y) {
    if (!d) return "desc is NULL";
    if ((uint64_t)d->low_cut + (uint64_t)d->high_cut >= 65536u) return "low_cut + high_cut must be below 65536";
    if (!(d->min_ev >= -24.0f && d->min_ev <= d->max_ev && d->max_ev <= 24.0f)) return "needs -24 <= min_ev <= max_ev <= 24";
    if (!(d->adapt_up >= 0.0f && d->adapt_up <= 1.0f && d->adapt_down >= 0.0f && d->adapt_down <= 1.0f)) return "adapt_up and adapt_down are rates in [0, 1]";
    if (!(d->window[0] < d->window[2] && d->window[2] <= res_x && d->window[1] < d->window[3] && d->window[3] <= res_y)) return "window needs x0 < x1 <= res_x and y0 < y1 <= res_y";
    return nullptr;
}

}  // namespace yk
