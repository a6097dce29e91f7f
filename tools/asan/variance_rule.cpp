// The variance rule (yuki_amd/csrc/yk_variance.h: vr_moments_pixel, vr_temporal, vr_spatial_pixel, vr_pixel) over films
// sprinkled with NaN, +-inf, -0 and 1e30, on heap arrays of exactly res_x * res_y records: under AddressSanitizer no tap of
// the 7 x 7 window, of the 3 x 3 variance Gaussian or of an a-trous step up to 128 reads past an array, and under UBSan
// nothing in the arithmetic is undefined.  Checks on the way: no variance is NaN or negative, a finite variance stays
// finite next to infinite ones, zeros stay zeros.  Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tools/asan/variance_rule.cpp -o /tmp/variance_rule && /tmp/variance_rule
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_variance.h"
using namespace yk;

static uint32_t lcg_state = 20261020u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 1e30f, -1e30f, 0.0f};
    return lcg() % 25u == 0u ? pool[lcg() % 7u] : v;
}

static int run(uint32_t w, uint32_t h, bool zeros) {
    const size_t n = (size_t)w * h;
    std::vector<float> film(3 * n), albedo(4 * n), moments(4 * n), var(n), guides(8 * n);
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) film[3 * i + k] = zeros ? 0.0f : sprinkle(0.2f + 0.6f * unit());
        for (int k = 0; k < 4; ++k) albedo[4 * i + k] = sprinkle(unit());
        moments[4 * i] = sprinkle(0.5f);
        moments[4 * i + 1] = sprinkle(0.25f + 0.02f * unit());
        moments[4 * i + 2] = sprinkle((float)(1 + lcg() % 5u));
        moments[4 * i + 3] = sprinkle((float)(lcg() % 40u));
        const bool hit = lcg() % 10u != 0u;
        const float g[8] = {0.0f, 0.0f, hit ? 1.0f : 0.0f, hit ? 1.0f : 0.0f, 0.05f * (float)(i % w), 0.05f * (float)(i / w), sprinkle(0.0f), 1.0f};
        std::memcpy(&guides[8 * i], g, 32);
    }
    VrParams a{};
    dn_set_grid(a.dn, w, h, 16);
    a.dn.den_n = 0.3f * 0.3f;
    a.dn.den_p = 0.06f * 0.06f;
    a.sv2 = 9.0f;
    a.epsilon = 1e-8f;
    a.spatial_scale = 1.0f;
    TpParams tp{};
    tp.dn = a.dn;
    tp.plane_tolerance = 0.05f;
    tp.normal_cos_min = 0.9f;
    tp.max_history = 24.0f;
    int bad = 0;
    // the moments blend, in place
    for (size_t i = 0; i < n; ++i) {
        float rec[4];
        vr_moments_pixel(tp, false, 1.0f, &film[3 * i], &moments[4 * i], rec);
        std::memcpy(&moments[4 * i], rec, 16);
    }
    // the variance image, with and without an albedo
    for (int with_albedo = 0; with_albedo < 2; ++with_albedo) {
        const float* alb = with_albedo ? albedo.data() : nullptr;
        const auto fetch = [&](uint32_t qx, uint32_t qy, VrTap& t) {
            const size_t q = (size_t)qy * w + qx;
            std::memcpy(t.ns, &guides[8 * q], 12);
            t.hit = guides[8 * q + 3];
            std::memcpy(t.p, &guides[8 * q + 4], 12);
            t.l = vr_tap_luminance(a.dn, film.data(), nullptr, alb, qx, qy);
        };
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                float v = 0.0f;
                const bool temporal = vr_temporal(&moments[4 * i], alb ? alb + 4 * i : nullptr, v);
                if (!temporal) v = vr_spatial_pixel(a, x, y, fetch);
                var[i] = vr_sanitise(v);
                if (var[i] != var[i] || var[i] < 0.0f || (zeros && !temporal && var[i] != 0.0f)) ++bad;
            }
    }
    for (size_t i = 0; i < n; i += 7) var[i] = __builtin_inff();
    // the filter, eight iterations
    std::vector<float> cur(4 * n), nxt(4 * n);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&cur[4 * i], &film[3 * i], 12);
        cur[4 * i + 3] = var[i];
    }
    for (int it = 0; it < 8; ++it) {
        const auto fetch = [&](uint32_t qx, uint32_t qy, VrFilterTap& t) {
            const size_t q = (size_t)qy * w + qx;
            std::memcpy(t.t.c, &cur[4 * q], 12);
            t.var = cur[4 * q + 3];
            std::memcpy(t.t.ns, &guides[8 * q], 12);
            t.t.hit = guides[8 * q + 3];
            std::memcpy(t.t.p, &guides[8 * q + 4], 12);
        };
        const auto fetch_var = [&](uint32_t qx, uint32_t qy) { return cur[4 * ((size_t)qy * w + qx) + 3]; };
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) vr_pixel(a, 1 << it, x, y, fetch, fetch_var, &nxt[4 * ((size_t)y * w + x)]);
        cur.swap(nxt);
    }
    for (size_t i = 0; i < n; ++i) {
        const float v = cur[4 * i + 3];
        const bool was_inf = i % 7 == 0;
        if (v != v || v < 0.0f || (v == __builtin_inff()) != was_inf) ++bad;
        if (zeros && (cur[4 * i] != 0.0f || cur[4 * i + 1] != 0.0f || cur[4 * i + 2] != 0.0f)) ++bad;
    }
    std::printf("%u x %u%s: bad = %d\n", w, h, zeros ? " zeros" : "", bad);
    return bad;
}

int main() {
    int bad = 0;
    bad += run(1, 1, false);
    bad += run(5, 3, false);
    bad += run(37, 23, false);
    bad += run(64, 36, false);
    bad += run(37, 23, true);
    std::printf("bad = %d\n", bad);
    return bad;
}
