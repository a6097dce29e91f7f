// yk_overlay.h — the wireframe overlays of the reference (app/renderpasses/ray_visualization.rs, bvh_visualization.rs), drawn
// by draw_visualizations (app/window.rs:1033-1063) into the tone-mapped film: the rule for one segment, on the host and on gfx950.
//
// The reference hands GL a LinesList under DrawParameters::default() (no depth test, no blending, line width 1, one colour
// per line, alpha 1).  GL fixes no bit-level result for a line, so this file fixes one:
//   - IEEE-754 binary32, round to nearest; every operation separate and left to right (the library is built with
//     -ffp-contract=off, so nothing below is fused); divisions correctly rounded.
// One text, two instances (the yk_tonemap.h pattern): the host instance (yk_overlay_draw with no context) is what the CPU
// suite pins against an independent restatement; the device instance (yk_overlay.hip) equals the host one bit for bit.
//
// The rule, per segment (p0, p1) in world space, M = world_to_clip row-major:
//   1. Clip coordinates (the vertex shader, `world_to_clip * vec4(position, 1)`): ov_clip_point.  A box's 8 corners are
//      transformed once and its 12 edges read them (bvh_visualization.rs:41-67: ov_box_corner, ov_edge_ends).
//   2. A segment with a non-finite clip component at either end draws nothing (a miss ray's t_max = inf; GL: undefined).
//   2a. DECISION (direction): the ends are put in a canonical order before clipping — the end whose (x, y, z, w) compares
//      lower, component by component, comes first (ov_clip_less) — so that a segment and its reverse clip, and therefore
//      draw, identically.  Step 5 alone would not give that for a clipped segment: the two directions round differently.
//   3. Clipping to -w <= x, y, z <= w (GL's view volume), parametric with t in [0, 1]: the six boundary values
//      w+x, w-x, w+y, w-y, w+z, w-z of the UNCLIPPED ends, in that order; both negative: reject; d0 negative: t = d0/(d0-d1)
//      raises t0 when t > t0; d1 negative: the same t lowers t1 when t < t1; t0 > t1 after the six: reject.  An end with
//      t0 != 0 (t1 != 1) becomes c0 + (c1-c0)*t per component; otherwise it is used exactly.
//   4. Window coordinates (perspective divide + viewport): xw = ((x/w)*0.5 + 0.5)*res_x, yw likewise with res_y.  Film row
//      r is yw in [r, r+1): the matrix already holds the reference's flip_y.
//   4a. DECISION: a segment with a non-finite window coordinate (w == 0 after clipping, an overflow) draws nothing.
//   5. The major axis is x when |dxw| >= |dyw|; the ends are swapped so that the major coordinate ascends, a to b.
//      a == b (a point) draws nothing.
//   6. One pixel for every integer k with a <= k + 0.5 < b and 0 <= k < res_major (ov_first_center gives both loop
//      bounds): m = m_a + ((k + 0.5) - a) * ((m_b - m_a)/(b - a)), the minor index is floor(m), and the pixel is skipped
//      when m < 0, m >= res_minor or m is NaN (ov_pixel).
//   7. A pixel takes the colour of the LAST primitive in list order that covers it: lines by index, then boxes by index,
//      a box's edges in the reference's edge order.  The ordinal of line i is i, of edge e of box b n_lines + 12*b + e.
//      Pixels no primitive covers are not written.
#pragma once
#include "yk_math.h"

namespace yk {

struct OvClip {
    float x, y, z, w;
};

// The plan of one segment after steps 1-5: pixels k in [k_lo, k_hi) along the major axis.
struct OvSpan {
    int32_t k_lo, k_hi;
    uint32_t x_major;
    float a, m_a, slope;
};

// Step 1.  `m` row-major: each row ((m0*x + m1*y) + m2*z) + m3.
YK_HD float ov_row(const float* r, float x, float y, float z) {
    float p = r[0] * x;
    float q = r[1] * y;
    float s = p + q;
    float t = r[2] * z;
    s = s + t;
    return s + r[3];
}
YK_HD OvClip ov_clip_point(const float* m, float x, float y, float z) {
    return OvClip{ov_row(m, x, y, z), ov_row(m + 4, x, y, z), ov_row(m + 8, x, y, z), ov_row(m + 12, x, y, z)};
}

// bvh_visualization.rs:41-50: corner j of (p_min, p_max) — x from p_max for j in {1, 2, 5, 6}, y for {2, 3, 6, 7}, z for j >= 4.
YK_HD void ov_box_corner(const float* box, uint32_t j, float& x, float& y, float& z) {
    const uint32_t q = j & 3u;
    x = (q == 1u || q == 2u) ? box[3] : box[0];
    y = (q >= 2u) ? box[4] : box[1];
    z = (j >= 4u) ? box[5] : box[2];
}
// bvh_visualization.rs:54-67: the corners of edge e = 0..11: (0,1)(1,2)(2,3)(3,0)(0,4)(1,5)(2,6)(3,7)(4,5)(5,6)(6,7)(7,4), one nibble each.
YK_HD void ov_edge_ends(uint32_t e, uint32_t& i0, uint32_t& i1) {
    i0 = (uint32_t)(0x765432103210ull >> (4u * e)) & 15u;
    i1 = (uint32_t)(0x476576540321ull >> (4u * e)) & 15u;
}
// bvh_visualization.rs:35-39: red for an even array index, green for an odd one.
YK_HD void ov_box_colour(uint32_t box_index, float& r, float& g, float& b) {
    r = (box_index & 1u) ? 0.0f : 1.0f;
    g = (box_index & 1u) ? 1.0f : 0.0f;
    b = 0.0f;
}

YK_HD bool ov_finite(float v) { return fabsf(v) <= 3.40282347e+38f; }  // false for NaN
YK_HD bool ov_finite(const OvClip& c) { return ov_finite(c.x) && ov_finite(c.y) && ov_finite(c.z) && ov_finite(c.w); }

// Step 2a.
YK_HD bool ov_clip_less(const OvClip& p, const OvClip& q) {
    if (p.x != q.x) return p.x < q.x;
    if (p.y != q.y) return p.y < q.y;
    if (p.z != q.z) return p.z < q.z;
    return p.w < q.w;
}

// The outcode of step 3 for one end: bit i set when boundary value i is negative.  A primitive all of whose vertices share
// a set bit has every segment rejected by "both negative" (what yk_overlay.hip uses to drop a whole box).
YK_HD uint32_t ov_outcode(const OvClip& c) {
    return (c.w + c.x < 0.0f ? 1u : 0u) | (c.w - c.x < 0.0f ? 2u : 0u) | (c.w + c.y < 0.0f ? 4u : 0u) | (c.w - c.y < 0.0f ? 8u : 0u) |
           (c.w + c.z < 0.0f ? 16u : 0u) | (c.w - c.z < 0.0f ? 32u : 0u);
}

// One boundary of step 3; false = rejected.
YK_HD bool ov_clip_plane(float d0, float d1, float& t0, float& t1) {
    if (d0 < 0.0f && d1 < 0.0f) return false;
    if (d0 < 0.0f) {
        float den = d0 - d1;
        float t = d0 / den;
        if (t > t0) t0 = t;
    } else if (d1 < 0.0f) {
        float den = d0 - d1;
        float t = d0 / den;
        if (t < t1) t1 = t;
    }
    return true;
}

YK_HD float ov_lerp(float c0, float c1, float t) {
    float d = c1 - c0;
    float s = d * t;
    return c0 + s;
}
YK_HD OvClip ov_lerp(const OvClip& c0, const OvClip& c1, float t) {
    return OvClip{ov_lerp(c0.x, c1.x, t), ov_lerp(c0.y, c1.y, t), ov_lerp(c0.z, c1.z, t), ov_lerp(c0.w, c1.w, t)};
}

// Step 4 for one coordinate.
YK_HD float ov_window(float v, float w, float res) {
    float n = v / w;
    n = n * 0.5f;
    n = n + 0.5f;
    return n * res;
}

// Step 6's loop bounds: the smallest integer k in [0, res] with k + 0.5 >= v (res when there is none below it).  res <= 65535,
// so k + 0.5 is exact and so is every comparison.  A NaN never gets here (step 4a).
YK_HD int32_t ov_first_center(float v, uint32_t res) {
    if (!(v > 0.5f)) return 0;
    if (v >= (float)res) return (int32_t)res;
    int32_t k = (int32_t)v;  // floor: v > 0
    if ((float)k + 0.5f < v) k += 1;
    return k;
}

// Steps 2-5 for clip-space ends; false = the segment draws nothing.
YK_HD bool ov_span(OvClip c0, OvClip c1, uint32_t res_x, uint32_t res_y, OvSpan& s) {
    if (!ov_finite(c0) || !ov_finite(c1)) return false;  // 2
    if (ov_clip_less(c1, c0)) {                          // 2a
        OvClip t = c0;
        c0 = c1;
        c1 = t;
    }
    float t0 = 0.0f, t1 = 1.0f;  // 3
    if (!ov_clip_plane(c0.w + c0.x, c1.w + c1.x, t0, t1)) return false;
    if (!ov_clip_plane(c0.w - c0.x, c1.w - c1.x, t0, t1)) return false;
    if (!ov_clip_plane(c0.w + c0.y, c1.w + c1.y, t0, t1)) return false;
    if (!ov_clip_plane(c0.w - c0.y, c1.w - c1.y, t0, t1)) return false;
    if (!ov_clip_plane(c0.w + c0.z, c1.w + c1.z, t0, t1)) return false;
    if (!ov_clip_plane(c0.w - c0.z, c1.w - c1.z, t0, t1)) return false;
    if (t0 > t1) return false;
    const OvClip e0 = (t0 != 0.0f) ? ov_lerp(c0, c1, t0) : c0;
    const OvClip e1 = (t1 != 1.0f) ? ov_lerp(c0, c1, t1) : c1;
    const float fx = (float)res_x, fy = (float)res_y;  // 4
    const float x0 = ov_window(e0.x, e0.w, fx), y0 = ov_window(e0.y, e0.w, fy);
    const float x1 = ov_window(e1.x, e1.w, fx), y1 = ov_window(e1.y, e1.w, fy);
    if (!ov_finite(x0) || !ov_finite(y0) || !ov_finite(x1) || !ov_finite(y1)) return false;  // 4a
    const float dx = x1 - x0, dy = y1 - y0;  // 5
    s.x_major = fabsf(dx) >= fabsf(dy) ? 1u : 0u;
    float a = s.x_major ? x0 : y0, b = s.x_major ? x1 : y1;
    float m_a = s.x_major ? y0 : x0, m_b = s.x_major ? y1 : x1;
    if (a > b) {
        float t = a;
        a = b;
        b = t;
        t = m_a;
        m_a = m_b;
        m_b = t;
    }
    if (!(a < b)) return false;
    const uint32_t res_major = s.x_major ? res_x : res_y;
    s.k_lo = ov_first_center(a, res_major);
    s.k_hi = ov_first_center(b, res_major);
    s.a = a;
    s.m_a = m_a;
    float dm = m_b - m_a;
    float dl = b - a;
    s.slope = dm / dl;
    return s.k_lo < s.k_hi;
}

// Step 6 for one k in [k_lo, k_hi): the pixel's index in the row-major film, or false when the minor index is off the film.
YK_HD bool ov_pixel(const OvSpan& s, int32_t k, uint32_t res_x, uint32_t res_y, uint32_t& index) {
    float c = (float)k + 0.5f;
    float u = c - s.a;
    float v = u * s.slope;
    float m = s.m_a + v;
    const uint32_t res_minor = s.x_major ? res_y : res_x;
    if (!(m >= 0.0f) || m >= (float)res_minor) return false;
    const uint32_t j = (uint32_t)m;  // floor: m >= 0
    index = s.x_major ? j * res_x + (uint32_t)k : (uint32_t)k * res_x + j;
    return true;
}

// ray_visualization.rs:36-42: the colour of a ray by its type (yk_ray_type); false for an unknown type.
YK_HD bool ov_ray_colour(uint32_t ray_type, float& r, float& g, float& b) {
    switch (ray_type) {
        case 0: r = 1.0f; g = 1.0f; b = 1.0f; return true;  // Direct
        case 1: r = 1.0f; g = 0.0f; b = 0.0f; return true;  // Reflection
        case 2: r = 0.0f; g = 1.0f; b = 0.0f; return true;  // Refraction
        case 3: r = 0.0f; g = 0.0f; b = 1.0f; return true;  // Normal
        case 4: r = 1.0f; g = 1.0f; b = 0.0f; return true;  // Shadow
        default: return false;
    }
}

}  // namespace yk
