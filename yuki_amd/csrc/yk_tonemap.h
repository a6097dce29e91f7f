// yk_tonemap.h — the tone-map pass of the reference (app/renderpasses/tonemap.rs) per pixel, on the host and on gfx950.
//
// The reference runs its film through a GL fragment shader (FILMIC_FS_CODE :318-385, HEATMAP_FS_CODE :387-422) before
// `yuki --out` writes it (app/headless.rs:62-84, apply_tone_map :113-158), and finds the Heatmap's bounds on the CPU
// (find_min_max :447-472).  GLSL fixes no bit-level result, so the reference's own files differ between GL drivers; this
// file fixes one evaluation order:
//   - IEEE-754 binary32, round to nearest; every operation separate and left to right (the library is built with
//     -ffp-contract=off, so nothing below is fused); divisions correctly rounded.
// One text, two instances (the yk_libm.h pattern): the host instance (yk_tone_map with no context) is what the CPU suite
// pins against an independent restatement; the device instance (yk_tonemap.hip) is compared with the host one bit for bit.
#pragma once
#include <float.h>

#include "yk_math.h"

namespace yk {

enum : uint32_t { TM_RAW = 0, TM_FILMIC = 1, TM_HEATMAP = 2 };
enum : uint32_t { TM_RED = 0, TM_GREEN = 1, TM_BLUE = 2, TM_LUMINANCE = 3 };

// `#define saturate(v) clamp(v, 0, 1)` (:330, :401).  GLSL leaves clamp(NaN) undefined; here saturate(x) is
// x > 0 ? (x < 1 ? x : 1) : 0, so NaN -> 0, -0 -> +0, +inf -> 1, with no sign-of-zero freedom (fminf / fmaxf have it).
YK_HD float tm_saturate(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// Luminance, in the order of find_min_max (:457): (0.2126*r + 0.7152*g) + 0.0722*b.  The shader's
// dot(rgb, vec3(0.2126, 0.7152, 0.0722)) (:413) uses the same one.
YK_HD float tm_luminance(float r, float g, float b) {
    float a = 0.2126f * r;
    float c = 0.7152f * g;
    float s = a + c;
    float d = 0.0722f * b;
    return s + d;
}

// The sample-count lookup of FILMIC_FS_CODE main (:372-377): x_tile_count = res.x / tile_dim with FLOOR division (:373),
// flat = (y / tile_dim) * x_tile_count + x / tile_dim.  Film.samples is laid out by FilmTile.index (generate_tiles,
// film.rs:299-331): row-major over the CEIL grid.  When res_x % tile_dim != 0 the shader therefore reads another tile's
// count; that is the reference's arithmetic and is reproduced.  flat < ceil(res_x/td) * ceil(res_y/td) always.
// gl_FragCoord.y is the film row: the texture upload and the read-back both keep the film's row order.
YK_HD uint32_t tm_sample_index(uint32_t x, uint32_t y, uint32_t tile_dim, uint32_t x_tile_count) {
    return (y / tile_dim) * x_tile_count + x / tile_dim;
}

// RRTAndODTFit (:348-353): a = v*(v + 0.0245786) - 0.000090537; b = v*(0.983729*v + 0.4329510) + 0.238081; a / b.
// Once v exceeds about 1.8e19, v*v overflows and a / b = inf / inf = NaN (float32: fit(1e19) = 1.01654, fit(2e19) = NaN);
// saturate then maps that channel to 0 after the output matrix, not to 1.
YK_HD float tm_rrt_odt_fit(float v) {
    float t = v + 0.0245786f;
    float a = v * t;
    a = a - 0.000090537f;
    float u = 0.983729f * v;
    u = u + 0.4329510f;
    float b = v * u;
    b = b + 0.238081f;
    return a / b;
}

// out_i = (m[i][0]*r + m[i][1]*g) + m[i][2]*b: `ACESInputMat * color` with ACESInputMat = transpose(mat3(rows)) (:334-346),
// so the rows as written in the shader are the matrix's rows.
YK_HD float tm_row(float m0, float m1, float m2, float r, float g, float b) {
    float x = m0 * r;
    float y = m1 * g;
    float s = x + y;
    float z = m2 * b;
    return s + z;
}

// FILMIC_FS_CODE (:318-385) for one pixel.  `count` is (float)Film.samples[flat] (tm_sample_index), or 0 without a
// table (the non-accumulating film, tonemap.rs:240-251):
//   1. count > 0: r, g, b each divided by count (:376-377)   2. c *= exposure (:378)
//   3. c = ACESInputMat * c (:358)   4. RRTAndODTFit per component (:361)   5. c = ACESOutputMat * c, then saturate (:363-366)
YK_HD void tm_filmic(float count, float exposure, float& r, float& g, float& b) {
    if (count > 0.0f) {
        r = r / count;
        g = g / count;
        b = b / count;
    }
    r = r * exposure;
    g = g * exposure;
    b = b * exposure;
    float i0 = tm_row(0.59719f, 0.35458f, 0.04823f, r, g, b);
    float i1 = tm_row(0.07600f, 0.90834f, 0.01566f, r, g, b);
    float i2 = tm_row(0.02840f, 0.13383f, 0.83777f, r, g, b);
    i0 = tm_rrt_odt_fit(i0);
    i1 = tm_rrt_odt_fit(i1);
    i2 = tm_rrt_odt_fit(i2);
    float o0 = tm_row(1.60475f, -0.53108f, -0.07367f, i0, i1, i2);
    float o1 = tm_row(-0.10208f, 1.10813f, -0.00605f, i0, i1, i2);
    float o2 = tm_row(-0.00327f, -0.07276f, 1.07602f, i0, i1, i2);
    r = tm_saturate(o0);
    g = tm_saturate(o1);
    b = tm_saturate(o2);
}

// The value HEATMAP_FS_CODE maps (:409-414): texel[channel] for channel 1 (Green) and 2 (Blue) only — the shader tests
// `channel > 0 && channel < 3` — and luminance for BOTH 0 (Red) and 3 (Luminance).  find_min_max reads red for Red
// (tm_bounds_value), so under the default HeatmapParams (Red, no bounds) the bounds come from red while the mapped
// value is luminance.  Reproduced.
YK_HD float tm_heat_value(uint32_t channel, float r, float g, float b) {
    if (channel == TM_GREEN) return g;
    if (channel == TM_BLUE) return b;
    return tm_luminance(r, g, b);
}

// mix(x, y, a) = x*(1 - a) + y*a per component (GLSL).
YK_HD float tm_mix(float x, float y, float a) {
    float w = 1.0f - a;
    float p = x * w;
    float q = y * a;
    return p + q;
}

// HEATMAP_FS_CODE (:387-422) for one pixel: s = (value - min) / (max - min); s1 = saturate(s*2), s2 = saturate(s*2 - 1);
// out = mix(mix(LOW, MID, s1), HIGH, s2) with LOW = (0,0,1), MID = (0,1,0), HIGH = (1,0,0).  No division by sample
// counts (the reference maps raw sums).  min == max or an infinity gives NaN / +-inf in s, which saturate folds:
// a uniform film maps to LOW.
YK_HD void tm_heatmap(uint32_t channel, float lo, float hi, float& r, float& g, float& b) {
    float v = tm_heat_value(channel, r, g, b);
    float num = v - lo;
    float den = hi - lo;
    float s = num / den;
    float s2x = s * 2.0f;
    float s1 = tm_saturate(s2x);
    float s2 = tm_saturate(s2x - 1.0f);
    float m0 = tm_mix(0.0f, 0.0f, s1), m1 = tm_mix(0.0f, 1.0f, s1), m2 = tm_mix(1.0f, 0.0f, s1);
    r = tm_mix(m0, 1.0f, s2);
    g = tm_mix(m1, 0.0f, s2);
    b = tm_mix(m2, 0.0f, s2);
}

// The accessor of find_min_max (:452-458): px[channel] for Red / Green / Blue, luminance for Luminance.
YK_HD float tm_bounds_value(uint32_t channel, float r, float g, float b) {
    if (channel == TM_RED) return r;
    if (channel == TM_GREEN) return g;
    if (channel == TM_BLUE) return b;
    return tm_luminance(r, g, b);
}

// One step of find_min_max's fold (:463-469), which starts from (f32::MAX, f32::MIN) = (FLT_MAX, -FLT_MAX).  Rust's
// f32::min / max return the other operand for a NaN, and the running pair is never NaN, so a NaN pixel leaves it as it
// is and an all-NaN film returns the initial pair.  The sign of a zero result is not specified (either operand may be
// returned for min(+0, -0)); min and max are exact, so any tree of these steps gives the sequential fold's value.
YK_HD void tm_fold(float v, float& lo, float& hi) {
    if (v < lo) lo = v;
    if (v > hi) hi = v;
}

}  // namespace yk
