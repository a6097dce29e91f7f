// yk_adaptive.h — adaptive sampling: per-pixel statistics of the samples a pixel has taken decide which pixels take the
// next ones.  Everything behind the film knows how converged a pixel is (yk_variance.h); this is the same knowledge in
// front of it: a running mean and sum of squared deviations of the LUMINANCE of every sample (Welford), a test of the
// standard error of that mean against a fraction of the mean, and a list of the pixels that fail it, in an order that
// keeps a wave's camera rays together.
//
// The reference has no adaptive sampler, so this file is the rule.  Its arithmetic is yk_variance.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), divisions correctly rounded;
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context; the loops at the end of this file) and the gfx950 kernels of
// yk_adaptive.hip call the functions below and agree bit for bit, the order of the list included.
//
// Records.  yk_pixel_stats (mean, m2, n, drawn), 16 bytes: mean and m2 are the running mean and the sum of squared
// deviations of vr_luminance of the samples taken, n their number, drawn the number of sample indices consumed — the
// pixel's next sample index.  The film beside it is film_sum: row-major RGB float SUMS, the accumulating film.  All zeros is
// the cleared state of both.
//
// Limits: luminance only (a pixel noisy in chroma alone looks converged); yk_multi scenes are not served; choosing where
// to sample by the samples' own variance biases the estimate slightly (a pixel whose first samples happen to agree stops
// early and keeps its too-low value) — the 3 x 3 dilation and the floor on min_samples bound that, they do not remove it.
#pragma once
#include <algorithm>
#include <vector>

#include "yk_variance.h"

namespace yk {

const uint32_t AD_TILE = 16;  // the side of a tile of the list's order: a constant of the rule, not FilmSettings.tile_dim

// Everything about a call that depends on no pixel.
struct AdParams {
    uint32_t res_x, res_y;
    uint32_t min_samples, max_samples, round_passes, dilate;
    float thr2;  // threshold * threshold, computed once
    float epsilon;
};
// What the entry points ask of their descriptor: min_samples >= 2; min_samples <= max_samples <= 2^24 ((float)n stays
// exact); round_passes 1 .. 0xFFFF; dilate 0 or 1; threshold > 0; epsilon >= 0 (NaN fails both).
inline bool ad_desc_ok(const yk_adaptive_desc* d) {
    if (!d) return false;
    if (d->min_samples < 2u || d->max_samples < d->min_samples || d->max_samples > (1u << 24)) return false;
    if (d->round_passes == 0u || d->round_passes > 0xFFFFu || d->dilate > 1u) return false;
    return d->threshold > 0.0f && d->epsilon >= 0.0f;
}
inline AdParams ad_make_params(const yk_adaptive_desc* d, uint32_t res_x, uint32_t res_y) {
    AdParams a{};
    a.res_x = res_x;
    a.res_y = res_y;
    a.min_samples = d->min_samples;
    a.max_samples = d->max_samples;
    a.round_passes = d->round_passes;
    a.dilate = d->dilate;
    a.thr2 = d->threshold * d->threshold;
    a.epsilon = d->epsilon;
    return a;
}
inline uint32_t ad_tiles_x(uint32_t res_x) { return (res_x + AD_TILE - 1) / AD_TILE; }
inline uint32_t ad_tiles_y(uint32_t res_y) { return (res_y + AD_TILE - 1) / AD_TILE; }

// ---- fold of one sample c into the pixel's film sum and statistics.
//   drawn += 1, always;  l = vr_luminance(c), ll = l * l;
//   ll NaN or infinite (l is, or its square overflows): nothing else changes — a non-finite sample never enters the film or
//   the statistics (the moments blend's rule);
//   otherwise film += c (three separate adds), n += 1, d = l - mean, mean' = mean + d / (float)n,
//   m2' = m2 + d * (l - mean')  (Welford, in sample order).
YK_HD void ad_fold_sample(const float* c, float* film, yk_pixel_stats& s) {
    s.drawn += 1u;
    const float l = vr_luminance(c);
    const float ll = dn_canon(l * l);
    if (!tp_finite(ll)) return;
    film[0] = dn_canon(film[0] + c[0]);
    film[1] = dn_canon(film[1] + c[1]);
    film[2] = dn_canon(film[2] + c[2]);
    s.n += 1u;
    const float nf = (float)s.n;
    const float d = l - s.mean;
    const float q = d / nf;
    const float mean = dn_canon(s.mean + q);
    const float e = l - mean;
    const float p = d * e;
    s.m2 = dn_canon(s.m2 + p);
    s.mean = mean;
}

// ---- wants: true when n < min_samples; otherwise m2 > (thr2 * ((nf - 1) * nf)) * (me * me), nf = (float)n,
// me = mean + epsilon: (standard error of the mean) > threshold * (mean + epsilon), squared so that no square root is
// needed.  A NaN on either side compares false.
YK_HD bool ad_wants(const AdParams& a, const yk_pixel_stats& s) {
    if (s.n < a.min_samples) return true;
    const float nf = (float)s.n;
    const float n1 = nf - 1.0f;
    const float nn = n1 * nf;
    const float r = a.thr2 * nn;
    const float me = s.mean + a.epsilon;
    const float mm = me * me;
    const float rhs = r * mm;
    return s.m2 > rhs;
}
// eligible: the round still fits under the cap, drawn + round_passes <= max_samples (no wrap: 64-bit sum)
YK_HD bool ad_eligible(const AdParams& a, const yk_pixel_stats& s) { return (uint64_t)s.drawn + a.round_passes <= (uint64_t)a.max_samples; }

// ---- selected = eligible and (wants or (dilate and some 8-neighbour INSIDE the film wants)); a neighbour's want counts
// whether or not that neighbour is itself eligible.  want(qx, qy) answers for a pixel inside the film.
template <class Want>
YK_HD bool ad_selected(const AdParams& a, uint32_t x, uint32_t y, bool eligible, const Want& want) {
    if (!eligible) return false;
    if (want(x, y)) return true;
    if (!a.dilate) return false;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)a.res_y) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)a.res_x || (dx == 0 && dy == 0)) continue;
            if (want((uint32_t)qx, (uint32_t)qy)) return true;
        }
    }
    return false;
}
// ---- the order of the list: tiles of AD_TILE x AD_TILE over the ceil grid in row-major tile order, row-major inside a
// tile, clipped at the film's edges; the selected pixels keep that order.  Entry = (x | y << 16, drawn).
YK_HD uint32_t ad_entry_xy(uint32_t x, uint32_t y) { return x | (y << 16); }

// ---- resolve: rgb = film_sum / (float)n per component where n > 0, zeros otherwise; the variance of the mean
// m2 / ((nf - 1) * nf) where n >= 2, +inf otherwise; NaN or negative is written as 0 (vr_sanitise).  That is the image
// yk_denoise_variance takes as `variance`: +inf already means "this pixel's colour stop is off".
YK_HD void ad_resolve_pixel(const float* film, const yk_pixel_stats& s, float* rgb, float& var) {
    const float nf = (float)s.n;
    if (s.n > 0u) {
        rgb[0] = dn_canon(film[0] / nf);
        rgb[1] = dn_canon(film[1] / nf);
        rgb[2] = dn_canon(film[2] / nf);
    } else {
        rgb[0] = rgb[1] = rgb[2] = 0.0f;
    }
    if (s.n >= 2u) {
        const float n1 = nf - 1.0f;
        const float nn = n1 * nf;
        var = vr_sanitise(dn_canon(s.m2 / nn));
    } else {
        var = __builtin_inff();
    }
}

// ------------------------------------------------------------------ the host instance
// out_xy / out_sample hold res_x * res_y entries (either may be NULL: count only); returns the number selected.
inline uint32_t ad_select_host(const AdParams& a, const yk_pixel_stats* stats, uint32_t* out_xy, uint32_t* out_sample) {
    std::vector<uint8_t> wants((size_t)a.res_x * a.res_y);
    for (size_t i = 0; i < wants.size(); ++i) wants[i] = ad_wants(a, stats[i]) ? 1 : 0;
    const auto want = [&](uint32_t qx, uint32_t qy) { return wants[(size_t)qy * a.res_x + qx] != 0; };
    uint32_t n = 0;
    for (uint32_t ty = 0; ty < ad_tiles_y(a.res_y); ++ty)
        for (uint32_t tx = 0; tx < ad_tiles_x(a.res_x); ++tx)
            for (uint32_t y = ty * AD_TILE; y < std::min(a.res_y, (ty + 1) * AD_TILE); ++y)
                for (uint32_t x = tx * AD_TILE; x < std::min(a.res_x, (tx + 1) * AD_TILE); ++x) {
                    const yk_pixel_stats& s = stats[(size_t)y * a.res_x + x];
                    if (!ad_selected(a, x, y, ad_eligible(a, s), want)) continue;
                    if (out_xy) out_xy[n] = ad_entry_xy(x, y);
                    if (out_sample) out_sample[n] = s.drawn;
                    ++n;
                }
    return n;
}
// passes: n_passes x n x RGB, pass-major; entry e's values are folded in pass order.  The entries are unique pixels
// inside the film (the callers check).
inline void ad_fold_host(uint32_t res_x, const uint32_t* xy, uint32_t n, const float* passes, uint32_t n_passes, float* film_sum, yk_pixel_stats* stats) {
    for (uint32_t e = 0; e < n; ++e) {
        const size_t i = (size_t)(xy[e] >> 16) * res_x + (xy[e] & 0xFFFFu);
        for (uint32_t k = 0; k < n_passes; ++k) ad_fold_sample(passes + ((size_t)k * n + e) * 3, film_sum + 3 * i, stats[i]);
    }
}
inline void ad_resolve_host(uint32_t res_x, uint32_t res_y, const float* film_sum, const yk_pixel_stats* stats, float* out_rgb, float* out_variance) {
    for (size_t i = 0; i < (size_t)res_x * res_y; ++i) {
        float rgb[3], var;
        ad_resolve_pixel(film_sum + 3 * i, stats[i], rgb, var);
        if (out_rgb) out_rgb[3 * i] = rgb[0], out_rgb[3 * i + 1] = rgb[1], out_rgb[3 * i + 2] = rgb[2];
        if (out_variance) out_variance[i] = var;
    }
}

}  // namespace yk
