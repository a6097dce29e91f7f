// sampler_skip_test.cpp — sampler_skip_2d (yuki_amd/csrc/yk_rng.h) makes the state transition of sampler_get_2d: after
// either call the whole SamplerState is the same, field by field, and so are the next three draws (a 2-D, a 1-D and a 2-D
// one, what a light, the roulette and the BSDF sample would take).  Both sampler kinds; Stratified 2x2 and 8x8 with jitter on
// and off; a few pixels, sample indices and starting dimensions.  Host compile of the header (the samplers are
// __host__ __device__).  Built and run by tests/test_sampler_skip.py.
#include <cstdio>
#include <cstring>

#include "../../yuki_amd/csrc/yk_rng.h"

using namespace yk;

static int failures = 0;
static int cases = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool same_state(const SamplerState& a, const SamplerState& b) {
    return a.rng.state == b.rng.state && a.rng.inc == b.rng.inc && a.px == b.px && a.py == b.py && a.sample_index == b.sample_index && a.dimension == b.dimension;
}

static void one(const SamplerCfg& c, unsigned px, unsigned py, unsigned index, unsigned dim) {
    ++cases;
    SamplerState drawn = sampler_start(c, px, py, index, dim);
    if (c.kind == 1) drawn.dimension = dim;  // a path under way: the stratified sampler's own counter has moved on as well
    SamplerState skipped = drawn;
    float ux = -1.0f, uy = -1.0f;
    sampler_get_2d(c, drawn, ux, uy);
    sampler_skip_2d(c, skipped);
    CHECK(ux >= 0.0f && ux < 1.0f && uy >= 0.0f && uy < 1.0f);  // the draw that was skipped is a real one
    CHECK(drawn.dimension == dim + 2);
    CHECK(same_state(drawn, skipped));
    // the next three draws
    float a0, a1, b0, b1;
    sampler_get_2d(c, drawn, a0, a1);
    sampler_get_2d(c, skipped, b0, b1);
    CHECK(same_bits(a0, b0) && same_bits(a1, b1));
    CHECK(same_bits(sampler_get_1d(c, drawn), sampler_get_1d(c, skipped)));
    sampler_get_2d(c, drawn, a0, a1);
    sampler_get_2d(c, skipped, b0, b1);
    CHECK(same_bits(a0, b0) && same_bits(a1, b1));
    CHECK(same_state(drawn, skipped));
    // two skips in a row (two point lights) are two draws in a row
    SamplerState d2 = sampler_start(c, px, py, index, dim), s2 = d2;
    sampler_get_2d(c, d2, a0, a1);
    sampler_get_2d(c, d2, a0, a1);
    sampler_skip_2d(c, s2);
    sampler_skip_2d(c, s2);
    CHECK(same_state(d2, s2));
}

int main() {
    const SamplerCfg cfgs[] = {
        // kind, nx, ny, jitter, seed, spp
        {0u, 0u, 0u, 0u, 0ull, 4u},                       // Uniform 4
        {0u, 0u, 0u, 0u, 0x9e3779b97f4a7c15ull, 16u},     // Uniform 16, another seed
        {1u, 2u, 2u, 1u, 0ull, 4u},                       // Stratified 2x2, jitter
        {1u, 2u, 2u, 0u, 0ull, 4u},                       // Stratified 2x2, no jitter
        {1u, 8u, 8u, 1u, 0ull, 64u},                      // Stratified 8x8, jitter
        {1u, 8u, 8u, 0u, 12345ull, 64u},                  // Stratified 8x8, no jitter
    };
    const unsigned pixels[][2] = {{0u, 0u}, {1u, 0u}, {17u, 5u}, {1919u, 1079u}, {65535u, 65535u}};
    const unsigned dims[] = {0u, 2u, 7u, 40u};
    for (const SamplerCfg& c : cfgs)
        for (const auto& p : pixels)
            for (unsigned index : {0u, 1u, 3u, c.spp - 1u})
                for (unsigned dim : dims) one(c, p[0], p[1], index, dim);
    // without jitter the stratified sampler never touches its PCG: a skip must not either
    {
        const SamplerCfg c = cfgs[3];
        SamplerState s = sampler_start(c, 3u, 4u, 1u, 0u);
        const Pcg before = s.rng;
        sampler_skip_2d(c, s);
        CHECK(s.rng.state == before.state && s.rng.inc == before.inc && s.dimension == 2u);
    }
    if (failures) {
        std::printf("sampler_skip_test: %d failure(s) in %d cases\n", failures, cases);
        return 1;
    }
    std::printf("sampler_skip_test: ok (%d cases)\n", cases);
    return 0;
}
