// The adaptive-sampling rule (yuki_amd/csrc/yk_adaptive.h: ad_select_host, ad_fold_host, ad_resolve_host — the host instance
// itself) over statistics sprinkled with NaN, +-inf, -0, 1e30, n of 0 / 1 / at the cap and drawn at, just below and far above
// the cap, on heap arrays of exactly res_x * res_y records at resolutions that are no multiple of 16: under AddressSanitizer
// neither the 3 x 3 dilation, the clipped tiles of the list's order nor the fold reads or writes past an array, and under
// UBSan nothing in the arithmetic is undefined.  Checks on the way: every entry is inside the film, no pixel twice, the
// list is in the rule's order, a full selection of a cleared film lists every pixel, every selected pixel is eligible, no
// variance is NaN or negative, a non-finite pass advances drawn alone.  Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tools/asan/adaptive_rule.cpp -o /tmp/adaptive_rule && /tmp/adaptive_rule
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_adaptive.h"
using namespace yk;

static uint32_t lcg_state = 20261020u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 1e30f, -1e30f, 0.0f};
    return lcg() % 20u == 0u ? pool[lcg() % 7u] : v;
}
// position of a pixel in the rule's order: tiles row-major, rows inside the clipped tile
static uint64_t order_key(const AdParams& a, uint32_t x, uint32_t y) {
    const uint64_t tile = (uint64_t)(y / AD_TILE) * ad_tiles_x(a.res_x) + x / AD_TILE;
    return (tile << 8) | ((y % AD_TILE) * AD_TILE + x % AD_TILE);
}

static int run(uint32_t w, uint32_t h, uint32_t dilate, bool cleared) {
    const size_t n_px = (size_t)w * h;
    yk_adaptive_desc d = {16u, 128u, 16u, 0u, dilate, 0.1f, 0.01f};
    int bad = ad_desc_ok(&d) ? 0 : 1;
    const AdParams a = ad_make_params(&d, w, h);
    std::vector<yk_pixel_stats> stats(n_px);
    std::vector<float> film(3 * n_px);
    for (size_t i = 0; i < n_px && !cleared; ++i) {
        static const uint32_t ns[] = {0u, 1u, 15u, 16u, 128u, 1u << 24};
        static const uint32_t drawns[] = {0u, 111u, 112u, 113u, 128u, 0xFFFFFFFFu};
        stats[i].n = lcg() % 4u == 0u ? ns[lcg() % 6u] : 16u + lcg() % 100u;
        stats[i].drawn = lcg() % 4u == 0u ? drawns[lcg() % 6u] : stats[i].n;
        stats[i].mean = sprinkle(2.0f * unit());
        stats[i].m2 = sprinkle(40.0f * unit());
        for (int k = 0; k < 3; ++k) film[3 * i + k] = sprinkle(50.0f * unit());
    }
    // select: exactly n_px words each, not one more
    std::vector<uint32_t> xy(n_px), sample(n_px);
    const uint32_t n = ad_select_host(a, stats.data(), xy.data(), sample.data());
    if (n > n_px || n != ad_select_host(a, stats.data(), nullptr, nullptr)) ++bad;
    if (cleared && n != n_px) ++bad;
    std::vector<uint8_t> seen(n_px, 0);
    uint64_t prev = 0;
    for (uint32_t e = 0; e < n; ++e) {
        const uint32_t x = xy[e] & 0xFFFFu, y = xy[e] >> 16;
        if (x >= w || y >= h) {
            ++bad;
            continue;
        }
        const size_t i = (size_t)y * w + x;
        if (seen[i]++) ++bad;
        if (!ad_eligible(a, stats[i]) || sample[e] != stats[i].drawn) ++bad;
        const uint64_t key = order_key(a, x, y);
        if (e && key <= prev) ++bad;
        prev = key;
    }
    // fold: three passes of exactly n entries, some of them not finite
    std::vector<float> passes((size_t)3 * n * 3);
    for (float& v : passes) v = sprinkle(1.5f * unit());
    const std::vector<yk_pixel_stats> before = stats;
    const std::vector<float> film_before = film;
    ad_fold_host(w, xy.data(), n, passes.data(), 3, film.data(), stats.data());
    for (size_t i = 0; i < n_px; ++i) {
        if (stats[i].drawn != before[i].drawn + (seen[i] ? 3u : 0u) || stats[i].n > before[i].n + 3u) ++bad;
        if (!seen[i] && (std::memcmp(&stats[i], &before[i], 16) != 0 || std::memcmp(&film[3 * i], &film_before[3 * i], 12) != 0)) ++bad;
    }
    // a pass whose every value is not finite advances drawn alone
    const std::vector<yk_pixel_stats> mid = stats;
    const std::vector<float> film_mid = film;
    std::vector<float> nans((size_t)n * 3, __builtin_nanf(""));
    ad_fold_host(w, xy.data(), n, nans.data(), 1, film.data(), stats.data());
    for (size_t i = 0; i < n_px; ++i) {
        yk_pixel_stats want = mid[i];
        want.drawn += seen[i] ? 1u : 0u;
        if (std::memcmp(&stats[i], &want, 16) != 0 || std::memcmp(&film[3 * i], &film_mid[3 * i], 12) != 0) ++bad;
    }
    // resolve
    std::vector<float> rgb(3 * n_px), var(n_px);
    ad_resolve_host(w, h, film.data(), stats.data(), rgb.data(), var.data());
    ad_resolve_host(w, h, film.data(), stats.data(), nullptr, var.data());
    ad_resolve_host(w, h, film.data(), stats.data(), rgb.data(), nullptr);
    for (size_t i = 0; i < n_px; ++i) {
        if (var[i] != var[i] || var[i] < 0.0f) ++bad;
        if ((stats[i].n < 2u) != (var[i] == __builtin_inff() && stats[i].n < 2u)) ++bad;
        if (stats[i].n == 0u && (rgb[3 * i] != 0.0f || rgb[3 * i + 1] != 0.0f || rgb[3 * i + 2] != 0.0f)) ++bad;
    }
    std::printf("%u x %u dilate %u%s: %u selected, bad = %d\n", w, h, dilate, cleared ? " cleared" : "", n, bad);
    return bad;
}

int main() {
    int bad = 0;
    for (uint32_t dilate = 0; dilate < 2; ++dilate) {
        bad += run(1, 1, dilate, false);
        bad += run(5, 3, dilate, false);
        bad += run(17, 1, dilate, false);
        bad += run(37, 23, dilate, false);
        bad += run(130, 70, dilate, false);
    }
    bad += run(37, 23, 1, true);
    std::printf("bad = %d\n", bad);
    return bad;
}
