// The rectification rule (yuki_amd/csrc/yk_rectify.h: rc_tap, rc_pixel, rc_moments) over random records — films and
// histories sprinkled with NaN, +-inf, -0 and 1e30, counts of 0, -3, NaN and +inf, sample tables with zero counts — on heap
// arrays of exactly the film's size: under AddressSanitizer no tap reads past an array, and under UBSan nothing in the
// arithmetic is undefined.  Checks on the way: every tap the rule fetches lies inside the film; a pixel fetches none, one
// or two windows' worth of taps, so the number of taken taps k stays within the window; f lies in [0, 1] and is never NaN;
// a pixel that was not clipped keeps its 16 bytes; and every entry k_rectify reads of its LDS tile lies inside the tile, for
// every halo, block and lane.
// Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tests/cpp/rectify_rule.cpp -o /tmp/rectify_rule && /tmp/rectify_rule
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_rectify.h"
using namespace yk;

static uint32_t lcg_state = 20261021u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 1e30f, -1e30f, 0.0f};
    return lcg() % 25u == 0u ? pool[lcg() % 7u] : v;
}
static float count() {
    static const float pool[] = {0.0f, -3.0f, __builtin_nanf(""), __builtin_inff(), -0.0f, 0.5f};
    return lcg() % 12u == 0u ? pool[lcg() % 6u] : (float)(1u + lcg() % 99u);
}

static int run(uint32_t w, uint32_t h, uint32_t radius, float gamma, bool with_table) {
    const uint32_t td = 4;
    const size_t n = (size_t)w * h;
    std::vector<float> film(3 * n), hist(4 * n), mom(4 * n), taps(4 * n), out(4 * n), out_m(4 * n);
    std::vector<uint32_t> samples((size_t)((w + td - 1) / td) * ((h + td - 1) / td));
    for (auto& v : samples) v = lcg() % 5u;
    for (size_t q = 0; q < n; ++q) {
        for (int k = 0; k < 3; ++k) film[3 * q + k] = sprinkle((with_table ? 3.0f : 1.0f) * (0.2f + 0.6f * unit()));
        for (int k = 0; k < 3; ++k) hist[4 * q + k] = sprinkle(1.2f * unit() - 0.1f);
        hist[4 * q + 3] = count();
        for (int k = 0; k < 3; ++k) mom[4 * q + k] = sprinkle(8.0f * unit());
        mom[4 * q + 3] = lcg() % 8u == 0u ? count() : hist[4 * q + 3];
    }
    yk_rectify_desc d{radius, gamma};
    int bad = rc_desc_ok(&d) ? 0 : 1;
    const RcParams a = rc_make_params(&d, w, h, td);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) rc_tap(a.dn, film.data(), with_table ? samples.data() : nullptr, x, y, &taps[4 * ((size_t)y * w + x)]);
    const int R = (int)radius;
    long clipped_pixels = 0;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            const int x0 = (int)x - R < 0 ? 0 : (int)x - R, x1 = (int)x + R > (int)w - 1 ? (int)w - 1 : (int)x + R;
            const int y0 = (int)y - R < 0 ? 0 : (int)y - R, y1 = (int)y + R > (int)h - 1 ? (int)h - 1 : (int)y + R;
            const int window = (x1 - x0 + 1) * (y1 - y0 + 1);  // the taps inside the film: k can be no more
            int fetched = 0, outside = 0;
            const auto fetch = [&](uint32_t qx, uint32_t qy, float* t) {
                if (qx >= w || qy >= h || (int)qx < x0 || (int)qx > x1 || (int)qy < y0 || (int)qy > y1) ++outside;
                ++fetched;
                std::memcpy(t, &taps[4 * ((size_t)qy * w + qx)], 16);
            };
            float f;
            const bool clipped = rc_pixel<0>(a, x, y, &hist[4 * i], fetch, &out[4 * i], f);
            if (outside != 0) ++bad;
            if (fetched != 0 && fetched != window && fetched != 2 * window) ++bad;
            if (!(f >= 0.0f) || !(f <= 1.0f)) ++bad;
            if (!clipped && (f != 1.0f || std::memcmp(&out[4 * i], &hist[4 * i], 16) != 0)) ++bad;
            if (clipped && fetched != 2 * window) ++bad;
            std::memcpy(&out_m[4 * i], &mom[4 * i], 16);
            if (clipped) rc_moments(&mom[4 * i], f, out[4 * i + 3], &out_m[4 * i]);
            if (std::memcmp(&out_m[4 * i], &mom[4 * i], 8) != 0) ++bad;  // m1 and m2 keep their bits
            clipped_pixels += clipped;
        }
    std::printf("%u x %u, radius %u, gamma %g%s: clipped %ld of %zu, bad = %d\n", w, h, radius, (double)gamma, with_table ? ", table" : "", clipped_pixels, n, bad);
    return bad;
}

// Every LDS entry a lane of k_rectify reads, restated from yk_film_tile.h (device code, not included here): a block of
// TX x TY lanes at (bx0, by0) holds (TX + 2 halo) x (TY + 2 halo) entries whose entry 0 is film pixel (bx0 - halo,
// by0 - halo); a lane reads the taps of its window that lie inside the film.
static int tile_bound(int halo, int radius, int w, int h) {
    const int TX = 32, TY = 8, W = TX + 2 * halo, N = W * (TY + 2 * halo);
    int bad = 0;
    for (int by0 = 0; by0 < h; by0 += TY)
        for (int bx0 = 0; bx0 < w; bx0 += TX)
            for (int ty = 0; ty < TY; ++ty)
                for (int tx = 0; tx < TX; ++tx) {
                    const int x = bx0 + tx, y = by0 + ty;
                    if (x >= w || y >= h) continue;
                    for (int dy = -radius; dy <= radius; ++dy)
                        for (int dx = -radius; dx <= radius; ++dx) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                            const int k = (qy - (by0 - halo)) * W + (qx - (bx0 - halo));
                            if (k < 0 || k >= N) ++bad;
                        }
                }
    return bad;
}

int main() {
    int bad = 0;
    for (int r = 1; r <= (int)RC_MAX_RADIUS; ++r) {
        bad += tile_bound(r, r, 37, 23) + tile_bound(r, r, 64, 36) + tile_bound((int)RC_MAX_RADIUS, r, 33, 9) + tile_bound((int)RC_MAX_RADIUS, r, 1, 1);
    }
    std::printf("tile bounds: bad = %d\n", bad);
    const float gammas[] = {0.0f, 0.5f, 1.0f, 2.0f, __builtin_inff()};
    for (uint32_t r = 1; r <= RC_MAX_RADIUS; ++r) {
        bad += run(1, 1, r, 1.0f, false);
        bad += run(5, 70, r, gammas[r], true);
        bad += run(33, 9, r, gammas[r - 1], false);
        bad += run(37, 23, r, 1.0f, r % 2u != 0u);
        bad += run(2, 1, r, 0.0f, false);
    }
    bad += run(64, 36, 2, gammas[4], true);
    std::printf("bad = %d\n", bad);
    return bad;
}
