// render_plan_test.cpp — the arithmetic of a render submission (yuki_amd/csrc/yk_render_plan.h) on cases worked out by hand:
// pixel offsets and their refusals, the accumulating film's rules, the chunks under sample_buf_cap, the batch, the HBM clamp
// and the work sets.  Plain host C++: the header includes no HIP.  Built and run by tests/test_render_plan.py.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../yuki_amd/csrc/yk_render_plan.h"

using namespace yk_plan;

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)
static bool says(const char* got, const char* want) { return got && std::string(got) == want; }

// the 40 tiles of a 128 x 72 film at tile_dim 16 in the order of the reference's outward spiral (film.rs:333-376), as
// yk_film_tiles returns them: 32 of 256 pixels, the bottom row's 8 of 128
static const yk_tile SPIRAL[40] = {
    {48, 32, 64, 48},   {64, 32, 80, 48},   {64, 48, 80, 64},   {48, 48, 64, 64},   {32, 48, 48, 64},   {32, 32, 48, 48},   {32, 16, 48, 32},   {48, 16, 64, 32},
    {64, 16, 80, 32},   {80, 16, 96, 32},   {80, 32, 96, 48},   {80, 48, 96, 64},   {80, 64, 96, 72},   {64, 64, 80, 72},   {48, 64, 64, 72},   {32, 64, 48, 72},
    {16, 64, 32, 72},   {16, 48, 32, 64},   {16, 32, 32, 48},   {16, 16, 32, 32},   {16, 0, 32, 16},    {32, 0, 48, 16},    {48, 0, 64, 16},    {64, 0, 80, 16},
    {80, 0, 96, 16},    {96, 0, 112, 16},   {96, 16, 112, 32},  {96, 32, 112, 48},  {96, 48, 112, 64},  {96, 64, 112, 72},  {0, 64, 16, 72},    {0, 48, 16, 64},
    {0, 32, 16, 48},    {0, 16, 16, 32},    {0, 0, 16, 16},     {112, 0, 128, 16},  {112, 16, 128, 32}, {112, 32, 128, 48}, {112, 48, 128, 64}, {112, 64, 128, 72}};

static void offsets() {
    std::vector<uint32_t> off;
    // 65535 * 65535 + 2 * 65535 = 65536^2 - 1 = 0xFFFFFFFF: the last count that fits
    yk_tile t[3] = {{0, 0, 65535, 65535}, {0, 0, 2, 65535}, {7, 7, 8, 8}};
    CHECK(tile_ranges(t, 2, off) == TILES_OK);
    CHECK(off.size() == 3 && off[0] == 0 && off[1] == 0xFFFE0001u && off[2] == 0xFFFFFFFFu);
    CHECK(tile_ranges(t, 3, off) == TILES_TOO_MANY_PIXELS);
    yk_tile flat[2] = {{0, 0, 16, 16}, {5, 0, 5, 16}};  // x0 == x1
    CHECK(tile_ranges(flat, 2, off) == TILE_DEGENERATE);
    yk_tile low = {0, 9, 16, 8};  // y0 > y1
    CHECK(tile_ranges(&low, 1, off) == TILE_DEGENERATE);
    yk_tile edge[2] = {{112, 56, 128, 72}, {113, 0, 129, 16}};  // film 128 x 72: the first touches both edges, the second has x1 == res_x + 1
    CHECK(tile_ranges(edge, 1, off, 128, 72) == TILES_OK && off[1] == 256);
    CHECK(tile_ranges(edge, 2, off, 128, 72) == TILE_OUTSIDE_FILM);
    CHECK(tile_ranges(edge, 2, off) == TILES_OK);  // no film, no limit
    yk_tile tall = {0, 60, 16, 73};
    CHECK(tile_ranges(&tall, 1, off, 128, 72) == TILE_OUTSIDE_FILM);
    CHECK(tile_ranges(SPIRAL, 40, off) == TILES_OK && off[40] == 128 * 72);
}

static void accumulation() {
    const uint16_t samples[3] = {0, 5, 12};
    RenderPlan p;
    // plain film: every sample of the sampler, no table, exactly one pass
    CHECK(p.set_samples(nullptr, 3, -1, 1, 16) == nullptr && !p.accumulating && !p.sample_table && p.spp == 16 && p.sample_base == 0);
    CHECK(says(p.set_samples(nullptr, 3, -1, 2, 16), "bad number of passes"));
    CHECK(says(p.set_samples(nullptr, 3, -1, 0, 16), "bad number of passes"));
    // a table of FilmTile.sample: 12 + 4 == 16 is the last pass there is
    CHECK(p.set_samples(samples, 3, -1, 4, 16) == nullptr && p.accumulating && p.sample_table && p.spp == 4 && p.sample_base == 0);
    CHECK(says(p.set_samples(samples, 3, -1, 5, 16), "FilmTile.sample (+ passes) beyond the sampler's samples per pixel"));
    CHECK(says(p.set_samples(samples, 3, -1, 0, 16), "bad number of passes"));
    CHECK(says(p.set_samples(samples, 3, -1, 0x10000u, 0xFFFFu), "bad number of passes"));
    CHECK(says(p.set_samples(samples, 3, 0, 1, 16), "an accumulating tile list carries its own sample indices"));
    // one first sample for every tile
    CHECK(p.set_samples(nullptr, 3, 3, 13, 16) == nullptr && p.accumulating && !p.sample_table && p.spp == 13 && p.sample_base == 3);
    CHECK(p.set_samples(nullptr, 3, 0, 16, 16) == nullptr && p.spp == 16 && p.sample_base == 0);
    CHECK(says(p.set_samples(nullptr, 3, 3, 14, 16), "first_sample (+ passes) beyond the sampler's samples per pixel"));
    CHECK(says(p.set_samples(nullptr, 3, 16, 1, 16), "first_sample (+ passes) beyond the sampler's samples per pixel"));
    CHECK(p.set_samples(nullptr, 3, 0, 0xFFFFu, 0xFFFFu) == nullptr && p.spp == 0xFFFFu);
}

static void chunks() {
    std::vector<uint32_t> off;
    CHECK(tile_ranges(SPIRAL, 40, off) == TILES_OK);
    RenderPlan p;
    CHECK(p.set_samples(nullptr, 40, -1, 1, 16) == nullptr);
    CHECK(p.set_chunks(off.data(), 40, 1u << 20) == nullptr);
    CHECK(p.total_px == 9216 && p.total_work == 9216 * 16);
    CHECK(p.max_px_chunk == 4096);  // (1 << 20) / (16 bytes * 16 samples)
    CHECK(p.chunks.size() >= 3);
    size_t next = 0;
    for (size_t k = 0; k < p.chunks.size(); ++k) {
        const Chunk& c = p.chunks[k];
        CHECK(c.t_begin == next && c.t_end > c.t_begin && c.t_end <= 40);  // contiguous, never empty
        CHECK(c.px0 == off[c.t_begin] && c.npx == off[c.t_end] - off[c.t_begin]);
        CHECK(c.npx <= 4096);
        if (c.t_end < 40) CHECK(off[c.t_end + 1] - off[c.t_begin] > 4096);  // maximal: the next tile would not have fitted
        next = c.t_end;
    }
    CHECK(next == 40);  // every tile once
    // by hand: 12 x 256 + 5 x 128 + 256 = 3968 (one more 256 would not fit) | 11 x 256 + 2 x 128 + 4 x 256 = 4096 | the rest, 1152
    CHECK(p.chunks.size() == 3 && p.chunks[0].t_end == 18 && p.chunks[0].npx == 3968 && p.chunks[1].t_end == 35 && p.chunks[1].npx == 4096 && p.chunks[2].npx == 1152);

    // sample ids fit u32 whatever the cap: 0xFFFF samples a pixel leave 65536 pixels a chunk
    yk_tile wide[3] = {{0, 0, 65535, 1}, {0, 0, 1, 1}, {0, 0, 1, 1}};
    CHECK(tile_ranges(wide, 3, off) == TILES_OK);
    CHECK(p.set_samples(nullptr, 3, 0, 0xFFFFu, 0xFFFFu) == nullptr);
    CHECK(p.set_chunks(off.data(), 3, ~0ull) == nullptr && p.max_px_chunk == 65536 && p.chunks.size() == 2 && p.chunks[0].t_end == 2);
    for (const Chunk& c : p.chunks) CHECK((uint64_t)c.npx * p.spp <= 0xFFFFFFF0ull);

    // refusals, both known before anything is enqueued
    yk_tile big[3] = {{0, 0, 16, 16}, {16, 0, 32, 16}, {0, 0, 128, 64}};  // the third: 8192 pixels
    CHECK(tile_ranges(big, 3, off) == TILES_OK);
    CHECK(p.set_samples(nullptr, 3, -1, 1, 16) == nullptr);
    CHECK(says(p.set_chunks(off.data(), 3, 1u << 20), "a single tile exceeds sample_buf_cap"));
    CHECK(p.set_chunks(off.data(), 2, 1u << 20) == nullptr && p.chunks.size() == 1);
    CHECK(says(p.set_chunks(off.data(), 2, 16 * 16 - 1), "sample_buf_cap too small for one pixel"));
    CHECK(says(p.set_chunks(off.data(), 2, 16 * 16), "a single tile exceeds sample_buf_cap"));  // one pixel fits, no tile does
}

static void batch_and_work_sets() {
    std::vector<uint32_t> off;
    CHECK(tile_ranges(SPIRAL, 40, off) == TILES_OK);
    RenderPlan p;
    CHECK(p.set_samples(nullptr, 40, -1, 1, 16) == nullptr && p.set_chunks(off.data(), 40, 1u << 20) == nullptr);
    const uint64_t work = 9216 * 16;
    // two work sets iff streams >= 2, Path, no caller stream and more than one batch
    p.set_batch(4096, 2, true, false);
    CHECK(p.batch == 4096 && p.n_ws == 2);
    p.set_batch(4096, 1, true, false);
    CHECK(p.batch == 4096 && p.n_ws == 1);
    p.set_batch(4096, 2, false, false);
    CHECK(p.n_ws == 1);
    p.set_batch(4096, 2, true, true);
    CHECK(p.n_ws == 1);
    p.set_batch(work, 2, true, false);  // total_work <= batch_paths: one batch, one work set
    CHECK(p.batch == work && p.n_ws == 1);
    p.set_batch(128u << 20, 2, true, false);
    CHECK(p.batch == work && p.n_ws == 1);
    p.set_batch(work - 1, 2, true, false);
    CHECK(p.batch == work - 1 && p.n_ws == 2);

    // the HBM clamp: (148 + 53 * 3 + 36) * 1 = 343 bytes a path; half of the free bytes; only when 65536 paths still fit
    p.set_batch(100000, 1, true, false);
    p.clamp_batch_to_hbm(2 * 343 * 65536ull, 3);
    CHECK(p.batch == 65536);
    p.set_batch(100000, 1, true, false);
    p.clamp_batch_to_hbm(2 * 343 * 65536ull - 1, 3);  // fit == 65535: left alone
    CHECK(p.batch == 100000);
    p.set_batch(100000, 2, true, false);  // two work sets: 2 x (148 + 53 * max(1, 0) + 36) = 474 bytes a path
    CHECK(p.n_ws == 2);
    p.clamp_batch_to_hbm(2 * 474 * 70000ull, 0);
    CHECK(p.batch == 70000);
    p.clamp_batch_to_hbm(~0ull, 0);  // plenty: no change
    CHECK(p.batch == 70000);
}

int main() {
    offsets();
    accumulation();
    chunks();
    batch_and_work_sets();
    if (failures) {
        std::printf("render_plan_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("render_plan_test: ok\n");
    return 0;
}
