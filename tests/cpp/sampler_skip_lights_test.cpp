// sampler_skip_lights_test.cpp — the light loop of a vertex under lights that ignore their sample (light_draw_2d, yk_shade.h):
// n calls of sampler_skip_2d, one per light, against n real draws, at every dimension a depth-8 path with 1 to 4 lights
// reaches.  The walk is Path::li_internal's order of draws (path.rs:102-169): after the camera sample's two dimensions,
// per vertex two dimensions per light, two for the BSDF sample and, from the fifth vertex on, one for the roulette.  At every
// vertex the skipped copy must hold the drawn copy's whole SamplerState, and the BSDF and roulette draws that follow must be
// the same bits.  Uniform 4, Stratified 2x2 with and without jitter, Stratified 8x8 (the flagship's).  Host compile of the
// header (the samplers are __host__ __device__).  Built and run by tests/test_sampler_skip_lights.py.
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

static void path(const SamplerCfg& c, unsigned px, unsigned py, unsigned index, unsigned n_lights, unsigned max_depth) {
    float ux, uy;
    SamplerState drawn = sampler_start(c, px, py, index, 0u);
    sampler_get_2d(c, drawn, ux, uy);  // the camera sample
    unsigned expect_dim = 2u;
    for (unsigned vertex = 0; vertex < max_depth; ++vertex) {
        ++cases;
        SamplerState skipped = drawn;
        for (unsigned l = 0; l < n_lights; ++l) {
            ux = uy = -1.0f;
            sampler_get_2d(c, drawn, ux, uy);
            CHECK(ux >= 0.0f && ux < 1.0f && uy >= 0.0f && uy < 1.0f);  // what is skipped is a real draw
            sampler_skip_2d(c, skipped);
        }
        expect_dim += 2u * n_lights;
        CHECK(drawn.dimension == expect_dim);
        CHECK(same_state(drawn, skipped));
        // the BSDF sample and the roulette of the vertex see the same values after either
        float a0, a1, b0, b1;
        sampler_get_2d(c, drawn, a0, a1);
        sampler_get_2d(c, skipped, b0, b1);
        CHECK(same_bits(a0, b0) && same_bits(a1, b1));
        expect_dim += 2u;
        if (vertex > 3u) {  // path.rs:162: bounces > 3
            CHECK(same_bits(sampler_get_1d(c, drawn), sampler_get_1d(c, skipped)));
            expect_dim += 1u;
        }
        CHECK(same_state(drawn, skipped));
        CHECK(drawn.dimension == expect_dim);
    }
}

int main() {
    const SamplerCfg cfgs[] = {
        // kind, nx, ny, jitter, seed, spp
        {0u, 0u, 0u, 0u, 0x73B9642E74AC471Cull, 4u},  // Uniform 4
        {1u, 2u, 2u, 1u, 0x73B9642E74AC471Cull, 4u},  // Stratified 2x2, jitter
        {1u, 2u, 2u, 0u, 0x73B9642E74AC471Cull, 4u},  // Stratified 2x2, no jitter
        {1u, 8u, 8u, 1u, 0ull, 64u},                  // Stratified 8x8, jitter
    };
    const unsigned pixels[][2] = {{0u, 0u}, {17u, 5u}, {63u, 35u}, {1919u, 1079u}};
    for (const SamplerCfg& c : cfgs)
        for (const auto& p : pixels)
            for (unsigned index : {0u, 1u, c.spp - 1u})
                for (unsigned n_lights = 1; n_lights <= 4; ++n_lights) path(c, p[0], p[1], index, n_lights, 8u);
    if (failures) {
        std::printf("sampler_skip_lights_test: %d failure(s) in %d cases\n", failures, cases);
        return 1;
    }
    std::printf("sampler_skip_lights_test: ok (%d cases)\n", cases);
    return 0;
}
