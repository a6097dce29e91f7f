// pixel_list_plan_test.cpp — the plan of a pixel-list render (yuki_amd/csrc/yk_render_plan.h, RenderPlan::set_pixel_list) on
// cases worked out by hand: the chunks cover [0, n) exactly once under caps that force 1, 2 and many chunks, and the
// refusals.  Plain host C++: the header includes no HIP.  Built and run by tests/test_pixel_list_plan.py.
#include <cstdio>
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

// every pixel of [0, n) in exactly one chunk, in order, none empty, none above the cap
static void covers(const RenderPlan& p, uint64_t n, uint64_t cap_px, size_t want_chunks) {
    uint64_t next = 0;
    for (const Chunk& c : p.chunks) {
        CHECK(c.px0 == next && c.npx > 0 && c.npx <= cap_px);
        CHECK((uint64_t)c.npx * p.spp <= 0xFFFFFFF0ull);
        next += c.npx;
    }
    CHECK(next == n && p.chunks.size() == want_chunks);
    for (size_t k = 0; k + 1 < p.chunks.size(); ++k) CHECK(p.chunks[k].npx == cap_px);  // greedy: only the last one is short
}

static void chunks() {
    RenderPlan p;
    // 1296 entries, 3 of the list's 4 passes, samples end at 16 of 16: 16 bytes x 3 passes = 48 bytes a pixel
    CHECK(p.set_pixel_list(1296, 3, 4, 16, 16, 1296 * 48) == nullptr);
    CHECK(p.accumulating && p.sample_table && p.spp == 3 && p.sample_base == 0 && p.total_px == 1296 && p.total_work == 3888 && p.max_px_chunk == 1296);
    covers(p, 1296, 1296, 1);
    CHECK(p.set_pixel_list(1296, 3, 4, 16, 16, 1296 * 48 - 1) == nullptr && p.max_px_chunk == 1295);
    covers(p, 1296, 1295, 2);
    CHECK(p.chunks[1].px0 == 1295 && p.chunks[1].npx == 1);
    CHECK(p.set_pixel_list(1296, 3, 4, 16, 16, 648 * 48) == nullptr);
    covers(p, 1296, 648, 2);
    CHECK(p.set_pixel_list(1296, 3, 4, 16, 16, 100 * 48 + 47) == nullptr && p.max_px_chunk == 100);
    covers(p, 1296, 100, 13);
    CHECK(p.chunks[12].px0 == 1200 && p.chunks[12].npx == 96);
    CHECK(p.set_pixel_list(1296, 1, 1, 16, 16, 16) == nullptr);  // one pixel a chunk
    covers(p, 1296, 1, 1296);
    CHECK(p.set_pixel_list(1, 1, 1, 1, 1, ~0ull) == nullptr);
    covers(p, 1, 1, 1);
    // an empty list is a plan without chunks
    CHECK(p.set_pixel_list(0, 1, 1, 16, 16, 1u << 20) == nullptr && p.chunks.empty() && p.total_work == 0);
    // sample ids fit u32 whatever the cap: 0xFFFF passes leave 65536 pixels a chunk
    CHECK(p.set_pixel_list(65537, 0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu, ~0ull) == nullptr && p.max_px_chunk == 65536);
    covers(p, 65537, 65536, 2);
    // the batch and the work sets are the tile route's
    CHECK(p.set_pixel_list(1296, 3, 4, 16, 16, 1u << 20) == nullptr);
    p.set_batch(64, 2, true, false);
    CHECK(p.batch == 64 && p.n_ws == 2);
    p.set_batch(1u << 20, 2, true, false);
    CHECK(p.batch == 3888 && p.n_ws == 1);
}

static void refusals() {
    RenderPlan p;
    CHECK(says(p.set_pixel_list(10, 0, 4, 16, 16, 1u << 20), "bad number of passes"));
    CHECK(says(p.set_pixel_list(10, 5, 4, 16, 16, 1u << 20), "bad number of passes"));  // more than the list was made for
    CHECK(says(p.set_pixel_list(10, 0x10000u, 0x10000u, 16, 0xFFFFu, 1u << 20), "bad number of passes"));
    CHECK(p.set_pixel_list(10, 4, 4, 16, 16, 1u << 20) == nullptr);
    CHECK(says(p.set_pixel_list(10, 4, 4, 17, 16, 1u << 20), "pixel list: sample (+ passes) beyond the sampler's samples per pixel"));
    CHECK(says(p.set_pixel_list(10, 1, 4, 17, 16, 1u << 20), "pixel list: sample (+ passes) beyond the sampler's samples per pixel"));  // the bound is the list's, whatever is rendered of it
    CHECK(says(p.set_pixel_list(0, 1, 1, 2, 1, 1u << 20), "pixel list: sample (+ passes) beyond the sampler's samples per pixel"));   // an empty list as well
    CHECK(says(p.set_pixel_list(1ull << 32, 1, 1, 16, 16, ~0ull), "too many pixels in one call"));
    CHECK(says(p.set_pixel_list(10, 4, 4, 16, 16, 63), "sample_buf_cap too small for one pixel"));
    CHECK(p.set_pixel_list(10, 4, 4, 16, 16, 64) == nullptr && p.chunks.size() == 10);
}

int main() {
    chunks();
    refusals();
    if (failures) {
        std::printf("pixel_list_plan_test: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("pixel_list_plan_test: ok\n");
    return 0;
}
