// The guided upsample's rule (yuki_amd/csrc/yk_upsample.h: up_axis, up_low_colour, up_pixel) over random records — films
// sprinkled with NaN, +-inf, -0 and 1e30, guides of both hit classes, albedos with every special value, sample tables with
// zero counts — on heap arrays of exactly the low and the full film's size: under AddressSanitizer no tap, clamped or not,
// reads past an array, and under UBSan nothing in the arithmetic is undefined.  Checks on the way: a weight sum is never
// NaN or negative, the fallback copies the containing low pixel's bits, x0 and a stay in range for every s and i, and the
// window a block of k_upsample stages is never wider than the block plus one (the bound of its LDS arrays).
// Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tests/cpp/upsample_rule.cpp -o /tmp/upsample_rule && /tmp/upsample_rule
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_upsample.h"
using namespace yk;

static uint32_t lcg_state = 20261020u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 1e30f, -1e30f, 0.0f};
    return lcg() % 25u == 0u ? pool[lcg() % 7u] : v;
}
static void guide(float* g, uint32_t x, uint32_t y, float step) {
    const bool hit = lcg() % 10u != 0u;
    const bool left = lcg() % 3u != 0u;
    const float r[8] = {hit ? (left ? 0.6f : -0.6f) : 0.0f, 0.0f, hit ? 0.8f : 0.0f, hit ? 1.0f : 0.0f, step * (float)x, step * (float)y, sprinkle(0.01f * unit()), 1.0f};
    std::memcpy(g, r, 32);
}

static int run(uint32_t lw, uint32_t lh, uint32_t s, bool with_albedo, bool with_table) {
    const uint32_t W = s * lw, H = s * lh, td = 4;
    const size_t n_lo = (size_t)lw * lh, n = (size_t)W * H;
    std::vector<float> low(3 * n_lo), low_guides(8 * n_lo), low_albedo(4 * n_lo), guides(8 * n), albedo(4 * n), c(3 * n_lo), out(3 * n), weight(n);
    std::vector<uint32_t> samples((size_t)((lw + td - 1) / td) * ((lh + td - 1) / td));
    for (auto& v : samples) v = lcg() % 5u;
    for (size_t q = 0; q < n_lo; ++q) {
        for (int k = 0; k < 3; ++k) low[3 * q + k] = sprinkle(0.2f + 0.6f * unit());
        for (int k = 0; k < 4; ++k) low_albedo[4 * q + k] = sprinkle(unit());
        guide(&low_guides[8 * q], (uint32_t)(q % lw), (uint32_t)(q / lw), 0.05f * (float)s);
    }
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 4; ++k) albedo[4 * i + k] = sprinkle(unit());
        guide(&guides[8 * i], (uint32_t)(i % W), (uint32_t)(i / W), 0.05f);
    }
    yk_upsample_desc d{s, lcg() % 2u ? 0.3f : __builtin_inff(), lcg() % 2u ? 0.06f : __builtin_inff()};
    int bad = up_desc_ok(&d, lw, lh) ? 0 : 1;
    const UpParams a = up_make_params(&d, lw, lh, td);
    for (uint32_t gy = 0; gy < lh; ++gy)
        for (uint32_t gx = 0; gx < lw; ++gx) {
            const size_t q = (size_t)gy * lw + gx;
            std::memcpy(&c[3 * q], &low[3 * q], 12);
            up_low_colour(dn_count(a.dn, with_table ? samples.data() : nullptr, gx, gy), with_albedo ? &low_albedo[4 * q] : nullptr, &c[3 * q]);
        }
    const auto fetch = [&](uint32_t qx, uint32_t qy, DnTap& t) {
        const size_t q = (size_t)qy * lw + qx;
        std::memcpy(t.c, &c[3 * q], 12);
        dn_guide(&low_guides[8 * q], &low_guides[8 * q + 4], t.ns, t.hit, t.p);
    };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const uint32_t X = x / s, Y = y / s;
            int x0;
            float ax;
            up_axis(X, x - s * X, s, x0, ax);
            if (x0 < -1 || x0 > (int)lw - 1 || !(ax >= 0.0f) || !(ax < 1.0f)) ++bad;
            float rec[4];
            up_pixel(a, X, x - s * X, Y, y - s * Y, &guides[8 * i], guides[8 * i + 3], &guides[8 * i + 4], nullptr, fetch, rec);
            if (rec[3] != rec[3] || rec[3] < 0.0f) ++bad;
            if (rec[3] == 0.0f && std::memcmp(rec, &c[3 * ((size_t)Y * lw + X)], 12) != 0) ++bad;  // the fallback: the containing pixel's bits
            float full[4];
            up_pixel(a, X, x - s * X, Y, y - s * Y, &guides[8 * i], guides[8 * i + 3], &guides[8 * i + 4], with_albedo ? &albedo[4 * i] : nullptr, fetch, full);
            if (!with_albedo && std::memcmp(full, rec, 16) != 0) ++bad;
            std::memcpy(&out[3 * i], full, 12);
            weight[i] = full[3];
        }
    std::printf("%u x %u, s = %u%s%s: bad = %d\n", lw, lh, s, with_albedo ? ", albedo" : "", with_table ? ", table" : "", bad);
    return bad;
}

// The window k_upsample stages for a block of `span` full pixels starting at b0 (a multiple of span, inside a film of
// `full` pixels): from the first tap of the first pixel to the second tap of the last pixel inside the film.  It must fit
// span + 2 entries, the size of the kernel's LDS arrays, for every s and every block.
static int window_bound(uint32_t span) {
    int bad = 0, widest = 0;
    for (uint32_t s = 1; s <= YK_UPSAMPLE_MAX_S; ++s)
        for (uint32_t full : {s, 37u * s, 65535u / s * s})
            for (uint32_t b0 = 0; b0 < full; b0 += span) {
                const uint32_t last = b0 + span - 1u < full - 1u ? b0 + span - 1u : full - 1u;
                int x0, x1;
                float a;
                up_axis(b0 / s, b0 % s, s, x0, a);
                up_axis(last / s, last % s, s, x1, a);
                const int w = x1 + 2 - x0;
                if (w > widest) widest = w;
                if (w < 2 || w > (int)span + 1) ++bad;
            }
    std::printf("window of %u pixels: widest %d, bad = %d\n", span, widest, bad);
    return bad;
}

int main() {
    int bad = window_bound(32) + window_bound(8);  // FT_TX and FT_TY of yk_film_tile.h (device code, not included here)
    for (uint32_t s = 1; s <= YK_UPSAMPLE_MAX_S; ++s) {
        bad += run(1, 1, s, s % 2u != 0u, false);
        bad += run(5, 3, s, true, true);
        bad += run(13, 7, s, false, s % 2u == 0u);
    }
    bad += run(37, 23, 2, true, true);
    std::printf("bad = %d\n", bad);
    return bad;
}
