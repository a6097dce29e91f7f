// yk_temporal.h — the film across camera moves: "reproject" carries the history of the previous view to the current one
// through the two views' first-hit guides, "blend" folds the current view's film into it.  They sit between the
// accumulating film and the denoiser: while a camera stands every displayed frame is blend(R, film, samples) with R
// reprojected ONCE when the camera moved; the last blend's history output is the next move's H', and the guides of that
// view are its G'.
//
// The reference clears its film when the camera moves, so this file is the rule.  Its arithmetic is yk_denoise.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), divisions correctly rounded;
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and the gfx950 kernels of yk_temporal.hip call the functions
// below and agree bit for bit.
//
// Reprojected radiance is exact for view-independent (diffuse) surfaces only.  On glass and metal the carried mean is the
// radiance towards the PREVIOUS eye: it lags the view.  max_history is the loosest bound on how long — a new sample always
// weighs at least m / (max_history + m) — and yk_rectify.h, run before the blend, the tight one: it clips a history the
// current frame contradicts and shrinks its count.  Geometry that moves: tp_reproject_moved_pixel below, through the motion
// records of yk_motion.h.
#pragma once
#include "yk_denoise.h"
#include "yk_math.h"

namespace yk {

// Everything about a call that does not depend on the pixel.  dn carries the film's resolution and the sample table's
// index rule (tm_sample_index through dn_count); its sigmas are not used.
struct TpParams {
    DnParams dn;
    float plane_tolerance, normal_cos_min, max_history;
};
// What yk_history_reproject, yk_history_blend and yk_moments_blend ask of their descriptor, and the parameters it makes.
inline bool tp_desc_ok(const yk_temporal_desc* d) {
    if (!d) return false;
    if (!(d->plane_tolerance > 0.0f)) return false;                                   // <= 0 or NaN
    if (!(d->normal_cos_min >= -1.0f) || !(d->normal_cos_min <= 1.0f)) return false;  // outside [-1, 1] or NaN
    if (!(d->max_history >= 1.0f)) return false;                                      // < 1 or NaN
    return true;
}
inline TpParams tp_make_params(const yk_temporal_desc* d, uint32_t res_x, uint32_t res_y, uint32_t tile_dim) {
    TpParams a{};
    dn_set_grid(a.dn, res_x, res_y, tile_dim);
    a.plane_tolerance = d->plane_tolerance;
    a.normal_cos_min = d->normal_cos_min;
    a.max_history = d->max_history;
    return a;
}

// What a reprojection tap reads of a pixel of the previous view: its history record and its guide record (t is not used).
struct TpTap {
    float c[3];
    float n;
    float ns[3];
    float hit;  // != 0: a hit
    float p[3];
};

YK_HD bool tp_finite(float v) { return fabsf(v) < gl_from_bits(0x7f800000u); }  // false for NaN and +-inf

// The current pixel's hit point p in the previous view's raster space.
//   p_cam = camera_to_world_inv' . p,  r = raster_to_camera_inv' . p_cam, both by xf_point (the transform Camera::ray uses:
//   row sums left to right, the divide by w only when w != 1).
// xf_point does not return its w, so the w of the SECOND transform is read here, from the expression xf_point evaluates
// for it: w = ((m[12]*x + m[13]*y) + m[14]*z) + m[15] with m = raster_to_camera_inv' and (x, y, z) = p_cam — before
// xf_point runs on the same operands (the compiler shares the work).  w <= 0 or NaN: the point is behind the previous
// camera (w is its camera-space depth for a perspective camera) and the function returns false.
// fx = r.x - 0.5 and fy = r.y - 0.5: pixel centres sit at +0.5, as in yk_render_guides.
YK_HD bool tp_project(const float* c2w_inv, const float* r2c_inv, V3 p, float& fx, float& fy) {
    const V3 pc = xf_point(c2w_inv, p);
    const float w = r2c_inv[12] * pc.x + r2c_inv[13] * pc.y + r2c_inv[14] * pc.z + r2c_inv[15];
    if (!(w > 0.0f)) return false;
    const V3 r = xf_point(r2c_inv, pc);
    fx = r.x - 0.5f;
    fy = r.y - 0.5f;
    return true;
}

// One axis of the bilinear footprint: f NaN, < -1 or >= (float)res gives false (tested on the float, before any
// conversion to an integer); otherwise i0 = floor(f) in [-1, res - 1] and a = f - (float)i0 in [0, 1).
YK_HD bool tp_axis(float f, uint32_t res, int& i0, float& a) {
    if (!(f >= -1.0f) || !(f < (float)res)) return false;
    const float fl = floorf(f);
    i0 = (int)fl;
    a = f - fl;
    return true;
}

// Whether tap Q (inside the film, bilinear weight b) is taken for the current pixel with shading normal nsP and hit point
// pP.  The closed set of skipped taps — a skipped tap's colour is neither multiplied nor added:
//   1. Q lies outside the film (the caller: such a tap is never read);
//   2. b == 0;
//   3. G'[Q] is a miss (hit == 0);
//   4. H'[Q].n is <= 0 or NaN;
//   5. a channel of H'[Q] is NaN or infinite;
//   6. d = dot(nsP, p_Q - pP) — the denoiser's plane-distance expression, the library's dot — has |d| > plane_tolerance,
//      or d is NaN (a tolerance of +inf lets every finite or infinite d pass, a NaN d still not);
//   7. dot(nsP, ns_Q) < normal_cos_min, or it is NaN.
YK_HD bool tp_take(const TpParams& a, V3 nsP, V3 pP, float b, const TpTap& Q) {
    const V3 v = V3{Q.p[0], Q.p[1], Q.p[2]} - pP;
    const float d = dot(nsP, v);
    const float cs = dot(nsP, V3{Q.ns[0], Q.ns[1], Q.ns[2]});
    // every test is evaluated (no early way out): nothing a tap reads is needed on one side of a branch only
    const int ok_tap = (int)(b != 0.0f) & (int)(Q.hit != 0.0f) & (int)(Q.n > 0.0f);
    const int ok_rgb = (int)tp_finite(Q.c[0]) & (int)tp_finite(Q.c[1]) & (int)tp_finite(Q.c[2]);
    const int ok_geo = (int)(fabsf(d) <= a.plane_tolerance) & (int)(cs >= a.normal_cos_min);
    return (ok_tap & ok_rgb & ok_geo) != 0;
}

// Reproject, one current pixel whose guide is (nsP, hitP, pP).  fetch(qx, qy, tap) reads a pixel of the previous view
// inside the film.  out = (rgb, n):
//   a miss, a point behind the previous camera, a footprint off the film, or no tap taken: the all-zero record (a constant
//   background converges with its first sample);
//   otherwise the four taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with b = (1 - ax | ax) * (1 - ay | ay), accumulated
//   in that order: sw = sum b, rgb = sum(b * c_Q) / sw, n = sum(b * n_Q) / sw, each through dn_canon.
// All four taps are fetched before the first is consumed: the skip conditions select what is accumulated, not what is
// requested, and no branch stands between the requests.  A tap outside the film is never read: its request goes to the
// nearest pixel inside (one of the other taps' cache lines) and what comes back is dropped.
template <class Fetch>
YK_HD void tp_reproject_pixel(const TpParams& a, const float* c2w_inv, const float* r2c_inv, V3 nsP, float hitP, V3 pP, const Fetch& fetch, float* out) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (hitP == 0.0f) return;
    float fx, fy, ax, ay;
    int x0, y0;
    if (!tp_project(c2w_inv, r2c_inv, pP, fx, fy)) return;
    if (!tp_axis(fx, a.dn.res_x, x0, ax) || !tp_axis(fy, a.dn.res_y, y0, ay)) return;
    const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay};
    TpTap Q[4];
    bool inside[4];
    const int mx = (int)a.dn.res_x - 1, my = (int)a.dn.res_y - 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        inside[k] = qx >= 0 && qy >= 0 && qx <= mx && qy <= my;
        fetch((uint32_t)(qx < 0 ? 0 : (qx > mx ? mx : qx)), (uint32_t)(qy < 0 ? 0 : (qy > my ? my : qy)), Q[k]);
    }
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!inside[k]) continue;
        const float b = wx[k & 1] * wy[k >> 1];
        if (!tp_take(a, nsP, pP, b, Q[k])) continue;
        const float pr = b * Q[k].c[0], pg = b * Q[k].c[1], pb = b * Q[k].c[2], pn = b * Q[k].n;
        sr = sr + pr;
        sg = sg + pg;
        sb = sb + pb;
        sn = sn + pn;
        sw = sw + b;
    }
    if (sw == 0.0f) return;
    out[0] = dn_canon(sr / sw);
    out[1] = dn_canon(sg / sw);
    out[2] = dn_canon(sb / sw);
    out[3] = dn_canon(sn / sw);
}

// Reproject after the GEOMETRY moved (yk_history_reproject_moved), one current pixel whose guide is (nsP, hitP, .) and whose
// motion record is mv = (p_prev, known): tp_reproject_pixel with pP := p_prev; known == 0 gives the zero record, as a miss
// does.  Nothing else of the rule changes:
//   - the point projected into the previous camera is the previous position of the pixel's surface point;
//   - the plane test d = dot(nsP, p_Q - p_prev) runs entirely in the previous frame's world, where the previous guides live;
//   - nsP is the CURRENT shading normal, in the plane test and in the normal test.  The plane test is therefore exact for
//     a translation and approximate under a rotation: the error is the tap distance times the sine of the turn.  A surface
//     that turns by more than acos(normal_cos_min) between two frames loses its history.
// Carried radiance is the radiance the surface HAD: shadows and reflections of things that moved lag until yk_rectify.h
// clips them to the current frame, or max_history ends them.  A NaN in p_prev makes the projection's w a NaN (0 * NaN included): the zero record.
template <class Fetch>
YK_HD void tp_reproject_moved_pixel(const TpParams& a, const float* c2w_inv, const float* r2c_inv, V3 nsP, float hitP, const float* mv, const Fetch& fetch, float* out) {
    tp_reproject_pixel(a, c2w_inv, r2c_inv, nsP, mv[3] == 0.0f ? 0.0f : hitP, V3{mv[0], mv[1], mv[2]}, fetch, out);
}

// Blend, one pixel.  c: the film's RGB (its bits); m = (float)samples[tm_sample_index] (dn_count, the floor / ceil
// mismatch included) with a table, 1 without; h: the reprojected record, or NULL.  out = (rgb, n):
//   current:  with a table and m > 0, c goes through dn_normalise; m == 0: the current view contributes nothing.
//   history:  n = min(h.n, max_history), written so that a NaN stays a NaN (clamping BEFORE the sum: new samples always
//             weigh at least m / (max_history + m)); absent when h is NULL, n is <= 0 or NaN, or a channel of h is not finite.
//   both absent: zeros;   only the history absent: (c, m), c's bits as they are without a table;
//   only the current view absent: (h.rgb, n), h.rgb's bits;
//   neither:  t = n + m, rgb = (n*h + m*c) / t per channel, each operation separate, through dn_canon; the record is (rgb, t).
YK_HD void tp_blend_pixel(const TpParams& a, bool has_table, float m, const float* c_in, const float* h, float* out) {
    float c[3] = {c_in[0], c_in[1], c_in[2]};
    if (has_table) dn_normalise(m, c);
    const bool cur = m != 0.0f;
    float n = 0.0f;
    bool hist = false;
    if (h) {
        n = h[3] > a.max_history ? a.max_history : h[3];
        hist = n > 0.0f && tp_finite(h[0]) && tp_finite(h[1]) && tp_finite(h[2]);
    }
    if (!hist) {
        out[0] = cur ? c[0] : 0.0f;
        out[1] = cur ? c[1] : 0.0f;
        out[2] = cur ? c[2] : 0.0f;
        out[3] = cur ? m : 0.0f;
        return;
    }
    if (!cur) {
        out[0] = h[0];
        out[1] = h[1];
        out[2] = h[2];
        out[3] = n;
        return;
    }
    const float t = n + m;
    for (int k = 0; k < 3; ++k) {
        const float nh = n * h[k], mc = m * c[k];
        const float s = nh + mc;
        out[k] = dn_canon(s / t);
    }
    out[3] = t;
}

}  // namespace yk
