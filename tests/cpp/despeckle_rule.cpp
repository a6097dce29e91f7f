// The despeckle rule (yuki_amd/csrc/yk_despeckle.h: ds_pixel over rc_tap) over random records — films sprinkled with NaN,
// +-inf, -0, negative channels, 1e30 and 3e38 (the largest finite luminances), sample tables with zero counts — on heap arrays
// of exactly the film's size: under AddressSanitizer no tap reads past an array, and under UBSan nothing in the arithmetic
// is undefined.  Checks on the way: every tap the rule fetches lies inside the film and is not the pixel itself, and the
// window is walked once or not at all; the factor of a clamped pixel, recomputed from the rule's statement with the bound
// from a SORT of the taken luminances, lies in [0, 1) over a divisor that is > 0, and gives the output's bits; the
// compare-and-swap chain of ds_top_insert equals a sort on random and on tied sequences; a pixel that is neither clamped
// nor repaired keeps its 12 bytes; gain = +inf with floor = 0 is the identity; and every entry k_despeckle reads of its LDS
// tile lies inside the tile, for every block and lane.
// Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tests/cpp/despeckle_rule.cpp -o /tmp/despeckle_rule && /tmp/despeckle_rule
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "yk_despeckle.h"
using namespace yk;

static uint32_t lcg_state = 20261021u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 1e30f, 3e38f, 0.0f, -0.4f};
    return lcg() % 25u == 0u ? pool[lcg() % 8u] : v;
}

static int top4_equals_sort() {
    int bad = 0;
    for (int round = 0; round < 4000; ++round) {
        const int n = 1 + (int)(lcg() % 24u);
        std::vector<float> v((size_t)n);
        for (auto& e : v) e = round % 3 == 0 ? (float)(lcg() % 4u) : 4.0f * unit() - 1.0f;  // every third sequence is full of ties
        DsTop4 top = ds_top_empty();
        for (float e : v) ds_top_insert(top, e);
        std::sort(v.begin(), v.end(), std::greater<float>());
        for (int rank = 1; rank <= 4 && rank <= n; ++rank)
            if (ds_top_rank(top, rank) != v[(size_t)rank - 1]) ++bad;
    }
    std::printf("top four against a sort: bad = %d\n", bad);
    return bad;
}

static int run(uint32_t w, uint32_t h, yk_despeckle_desc d, bool with_table) {
    const uint32_t td = 4;
    const size_t n = (size_t)w * h;
    std::vector<float> film(3 * n), taps(4 * n), out(3 * n);
    std::vector<uint32_t> samples((size_t)((w + td - 1) / td) * ((h + td - 1) / td));
    for (auto& v : samples) v = lcg() % 5u;
    for (size_t q = 0; q < n; ++q) {
        const float fly = lcg() % 20u == 0u ? 5.0f + 100.0f * unit() : 1.0f;
        for (int k = 0; k < 3; ++k) film[3 * q + k] = sprinkle(fly * (with_table ? 3.0f : 1.0f) * (0.2f + 0.6f * unit()));
    }
    int bad = ds_desc_ok(&d) ? 0 : 1;
    const DsParams a = ds_make_params(&d, w, h, td);
    const uint32_t* table = with_table ? samples.data() : nullptr;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) rc_tap(a.dn, film.data(), table, x, y, &taps[4 * ((size_t)y * w + x)]);
    const int R = (int)d.radius;
    long n_clamped = 0, n_repaired = 0;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            const int x0 = (int)x - R < 0 ? 0 : (int)x - R, x1 = (int)x + R > (int)w - 1 ? (int)w - 1 : (int)x + R;
            const int y0 = (int)y - R < 0 ? 0 : (int)y - R, y1 = (int)y + R > (int)h - 1 ? (int)h - 1 : (int)y + R;
            const int window = (x1 - x0 + 1) * (y1 - y0 + 1) - 1;  // the taps inside the film, without the pixel
            int fetched = 0, outside = 0;
            std::vector<float> lum;
            const auto fetch = [&](uint32_t qx, uint32_t qy, float* t) {
                if (qx >= w || qy >= h || (int)qx < x0 || (int)qx > x1 || (int)qy < y0 || (int)qy > y1 || (qx == x && qy == y)) ++outside;
                ++fetched;
                std::memcpy(t, &taps[4 * ((size_t)qy * w + qx)], 16);
                if (rc_take(t)) lum.push_back(vr_luminance(t));
            };
            const uint8_t what = ds_pixel<0>(a, with_table, x, y, &film[3 * i], &taps[4 * i], fetch, &out[3 * i]);
            if (outside != 0) ++bad;
            if (fetched != 0 && fetched != window) ++bad;  // the window is walked once
            if (what == DS_UNTOUCHED && std::memcmp(&out[3 * i], &film[3 * i], 12) != 0) ++bad;
            if (what != DS_UNTOUCHED && ((int)lum.size() < (int)d.rank || lum.size() < d.min_taps || taps[4 * i + 3] == 0.0f)) ++bad;
            if (what == DS_CLAMPED) {
                std::sort(lum.begin(), lum.end(), std::greater<float>());
                float v = lum[d.rank - 1];
                v = v > 0.0f ? v : 0.0f;
                float bound = d.gain * v;
                bound = bound < d.floor ? d.floor : bound;
                const float lp = vr_luminance(&taps[4 * i]);
                const float s = bound / lp;
                if (!(lp > 0.0f) || !(bound >= 0.0f) || !(s >= 0.0f) || !(s < 1.0f)) ++bad;
                for (int k = 0; k < 3; ++k) {
                    const float want = film[3 * i + k] * s;
                    if (std::memcmp(&want, &out[3 * i + k], 4) != 0) ++bad;
                }
                ++n_clamped;
            }
            if (what == DS_REPAIRED) {
                if (!(d.flags & YK_DESPECKLE_REPAIR) || (tp_finite(taps[4 * i]) && tp_finite(taps[4 * i + 1]) && tp_finite(taps[4 * i + 2]))) ++bad;
                ++n_repaired;
            }
            if (d.gain == __builtin_inff() && d.floor == 0.0f && what == DS_CLAMPED) ++bad;
        }
    std::printf("%u x %u, radius %u, rank %u, min_taps %u, gain %g, floor %g%s%s: clamped %ld, repaired %ld of %zu, bad = %d\n", w, h, d.radius, d.rank, d.min_taps, (double)d.gain, (double)d.floor,
                d.flags ? ", repair" : "", with_table ? ", table" : "", n_clamped, n_repaired, n, bad);
    return bad;
}

// Every LDS entry a lane of k_despeckle reads, restated from yk_film_tile.h (device code, not included here): a block of
// TX x TY lanes at (bx0, by0) holds (TX + 2 halo) x (TY + 2 halo) entries whose entry 0 is film pixel (bx0 - halo,
// by0 - halo); a lane reads its own entry and the taps of its window that lie inside the film.
static int tile_bound(int halo, int w, int h) {
    const int TX = 32, TY = 8, W = TX + 2 * halo, N = W * (TY + 2 * halo);
    int bad = 0;
    for (int by0 = 0; by0 < h; by0 += TY)
        for (int bx0 = 0; bx0 < w; bx0 += TX)
            for (int ty = 0; ty < TY; ++ty)
                for (int tx = 0; tx < TX; ++tx) {
                    const int x = bx0 + tx, y = by0 + ty;
                    if (x >= w || y >= h) continue;
                    for (int dy = -halo; dy <= halo; ++dy)
                        for (int dx = -halo; dx <= halo; ++dx) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                            const int k = (qy - (by0 - halo)) * W + (qx - (bx0 - halo));
                            if (k < 0 || k >= N) ++bad;
                        }
                }
    return bad;
}

int main() {
    int bad = top4_equals_sort();
    for (int r = 1; r <= (int)DS_MAX_RADIUS; ++r) bad += tile_bound(r, 37, 23) + tile_bound(r, 64, 36) + tile_bound(r, 65, 17) + tile_bound(r, 1, 1);
    std::printf("tile bounds: bad = %d\n", bad);
    const float inf = __builtin_inff();
    const float gains[] = {0.0f, 1.0f, 1.5f, 2.0f, inf};
    for (uint32_t r = 1; r <= DS_MAX_RADIUS; ++r)
        for (uint32_t rank = 1; rank <= DS_MAX_RANK; ++rank) {
            const uint32_t rep = rank % 2u ? YK_DESPECKLE_REPAIR : 0u;
            bad += run(1, 1, yk_despeckle_desc{r, rank, rank, rep, 1.0f, 0.0f}, false);
            bad += run(2, 1, yk_despeckle_desc{r, rank, rank, rep, 1.0f, 0.0f}, true);
            bad += run(5, 70, yk_despeckle_desc{r, rank, 3u < rank ? rank : 3u, rep, gains[rank], 0.0f}, true);
            bad += run(33, 9, yk_despeckle_desc{r, rank, rank, rep ^ 1u, gains[rank - 1], 0.3f}, false);
            bad += run(37, 23, yk_despeckle_desc{r, rank, 5, rep, 2.0f, 0.0f}, (r + rank) % 2u != 0u);
            bad += run(65, 17, yk_despeckle_desc{r, rank, rank, rep, inf, 0.0f}, rank % 2u == 0u);
        }
    std::printf("bad = %d\n", bad);
    return bad;
}
