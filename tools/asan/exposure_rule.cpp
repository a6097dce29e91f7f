// The exposure meter's rule (yuki_amd/csrc/yk_exposure.h: ex_pixel_luminance, ex_bin, ex_cut, ex_kept, ex_bin_value,
// ex_finish, ex_exp2) over films sprinkled with NaN, +-inf, +-0, negatives, subnormals and values far outside the bins, on
// heap arrays of exactly the film's and the table's size: under AddressSanitizer no slot word, bin or table entry is
// touched out of bounds, and under UBSan nothing in the integer arithmetic (the cut's products, the int64 sum, the shift
// that makes 2^i, the float -> int conversion of ex_exp2) is undefined — extreme descriptors and a carried NaN included.
// Checks on the way: counted + skipped is the window's area, K >= 1 whenever N >= 1, the exposure is finite and positive.
// Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tools/asan/exposure_rule.cpp -o /tmp/exposure_rule && /tmp/exposure_rule
#include <cmath>
#include <cstdio>
#include <vector>
#include "yk_exposure.h"
using namespace yk;

static uint32_t lcg_state = 20261020u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float sprinkle(float v) {
    static const float pool[] = {__builtin_nanf(""), __builtin_inff(), -__builtin_inff(), -0.0f, 0.0f, -3.0f, 1e-40f, 1e-9f, 1e9f, 3e38f};
    return lcg() % 7u == 0u ? pool[lcg() % 10u] : v;
}

static int run(uint32_t w, uint32_t h, uint32_t td, const yk_exposure_desc& d, const yk_exposure_state* prev) {
    const size_t n = (size_t)w * h;
    std::vector<float> film(3 * n);
    for (float& v : film) v = sprinkle(std::exp2(24.0f * unit() - 12.0f));
    std::vector<uint32_t> samples((size_t)((w + td - 1) / td) * ((h + td - 1) / td));
    for (uint32_t& s : samples) s = lcg() % 6u;
    std::vector<uint32_t> slot(EX_SLOT_WORDS, 0u);
    for (uint32_t y = d.window[1]; y < d.window[3]; ++y)
        for (uint32_t x = d.window[0]; x < d.window[2]; ++x) {
            const float* p = &film[3 * ((size_t)y * w + x)];
            uint32_t edge;
            slot[ex_bin(ex_pixel_luminance((float)samples[tm_sample_index(x, y, td, w / td)], p[0], p[1], p[2]), &edge)] += 1;
            if (edge) slot[edge] += 1;
        }
    uint32_t N = 0, n_lo, n_top, cum = 0, K = 0;
    for (uint32_t b = 0; b < EX_BINS; ++b) N += slot[b];
    ex_cut(N, d.low_cut, d.high_cut, &n_lo, &n_top);
    int64_t S = 0;
    for (uint32_t b = 0; b < EX_BINS; ++b) {
        const uint32_t kept = ex_kept(cum, cum + slot[b], n_lo, n_top);
        cum += slot[b];
        K += kept;
        S += (int64_t)kept * ex_bin_value(b);
    }
    std::vector<yk_exposure_state> out(1);
    ex_finish(d, N, K, S, slot[EX_SKIPPED], slot[EX_BELOW], slot[EX_ABOVE], prev, out.data());
    const uint32_t area = (uint32_t)(d.window[2] - d.window[0]) * (uint32_t)(d.window[3] - d.window[1]);
    int bad = 0;
    if (out[0].counted + out[0].skipped != area) bad |= 1;
    if (N >= 1 && K < 1) bad |= 2;
    if (!(out[0].exposure > 0.0f) || std::isinf(out[0].exposure)) bad |= 4;
    if (bad) std::printf("%u x %u tile %u: check %d failed\n", w, h, td, bad);
    return bad;
}

int main() {
    int bad = 0;
    const uint32_t sizes[][3] = {{37, 23, 16}, {16, 16, 5}, {1, 5, 16}, {1, 1, 7}, {200, 150, 16}};
    for (const auto& s : sizes) {
        const uint16_t w = (uint16_t)s[0], h = (uint16_t)s[1];
        const yk_exposure_desc descs[] = {
            {3277, 1311, -2.47393f, -8.0f, 8.0f, 1.0f, 1.0f, {0, 0, w, h}},
            {0, 0, 0.0f, -24.0f, 24.0f, 0.25f, 0.75f, {0, 0, w, h}},
            {65535, 0, 24.0f, -24.0f, 24.0f, 0.0f, 0.0f, {0, 0, w, h}},
            {0, 65535, -24.0f, 24.0f, 24.0f, 1.0f, 0.0f, {(uint16_t)(w / 2), (uint16_t)(h / 2), w, h}},
        };
        const yk_exposure_state prevs[] = {{1.0f, 0.0f, 0.0f, 0, 0, 0, 0, 0}, {2.0f, -3.5f, -3.0f, 7, 0, 0, 0, 0}, {1.0f, __builtin_nanf(""), 0.0f, 0xFFFFFFFFu, 0, 0, 0, 0}, {1.0f, 3e38f, 0.0f, 1, 0, 0, 0, 0}};
        for (const auto& d : descs) {
            if (ex_desc_refusal(&d, w, h)) {
                std::printf("a descriptor of the sweep was refused: %s\n", ex_desc_refusal(&d, w, h));
                return 1;
            }
            bad |= run(s[0], s[1], s[2], d, nullptr);
            for (const auto& p : prevs) bad |= run(s[0], s[1], s[2], d, &p);
        }
    }
    for (int k = -24000; k <= 24000; ++k) {
        const float x = (float)k * 0.001f, got = ex_exp2(x);
        if (!(std::fabs((double)got / std::exp2((double)x) - 1.0) <= 1e-5)) {
            std::printf("ex_exp2(%g) = %g\n", x, got);
            bad |= 8;
        }
    }
    std::printf(bad ? "FAILED\n" : "exposure rule: clean\n");
    return bad ? 1 : 0;
}
