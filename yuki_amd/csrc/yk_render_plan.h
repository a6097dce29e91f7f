// yk_render_plan.h — what a render submission decides before it touches the device (yk_render.cpp), as pure functions
// over plain numbers: tiles -> pixel offsets, the accumulating film's rules, the chunks under sample_buf_cap, the batch
// size and the work sets.  No HIP here: tests/cpp/render_plan_test.cpp compiles this header alone.  Library-private.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/yuki_hip.h"

namespace yk_plan {

// tiles -> off[n_tiles + 1] (assert!(tile_pixels.len() >= tile.bb.area()), integrators/mod.rs:131).  A refusal is a
// reason: each caller says it in its own words.  res_x / res_y: the film the tiles must fit, where there is one.
enum TileRefusal { TILES_OK = 0, TILE_DEGENERATE, TILE_OUTSIDE_FILM, TILES_TOO_MANY_PIXELS };
inline TileRefusal tile_ranges(const yk_tile* tiles, size_t n_tiles, std::vector<uint32_t>& off, uint32_t res_x = ~0u, uint32_t res_y = ~0u) {
    off.assign(n_tiles + 1, 0);
    uint64_t total = 0;
    for (size_t t = 0; t < n_tiles; ++t) {
        if (tiles[t].x0 >= tiles[t].x1 || tiles[t].y0 >= tiles[t].y1) return TILE_DEGENERATE;
        if (tiles[t].x1 > res_x || tiles[t].y1 > res_y) return TILE_OUTSIDE_FILM;
        total += (uint64_t)(tiles[t].x1 - tiles[t].x0) * (uint64_t)(tiles[t].y1 - tiles[t].y0);
        if (total > 0xFFFFFFFFull) return TILES_TOO_MANY_PIXELS;
        off[t + 1] = (uint32_t)total;
    }
    return TILES_OK;
}

struct Chunk {  // tiles [t_begin, t_end): pixels [px0, px0 + npx) of the call
    size_t t_begin, t_end;
    uint32_t px0, npx;
};

// Every refusal below is YK_ERR_INVALID_ARGUMENT with the message returned; NULL accepts.
struct RenderPlan {
    // accumulating film (integrators/mod.rs:146-161): FilmTile.sample per tile (a table), or one index shared by all tiles
    bool accumulating = false, sample_table = false;
    uint32_t spp = 0;          // samples rendered per pixel by this call: the passes, or all of the sampler's
    uint32_t sample_base = 0;  // without a table: the first sample index of every pixel
    uint64_t total_px = 0, total_work = 0;
    uint64_t max_px_chunk = 0;  // sample ids fit u32 and the sample buffer stays under the cap
    std::vector<Chunk> chunks;  // greedy: each takes every tile that still fits
    size_t batch = 0;           // camera samples per batch
    int n_ws = 1;               // work sets that take alternate batches

    // render_manager.rs:135-143 queues samples 0 .. spp-1 of a tile and nothing else; an index beyond that is outside the
    // samplers' domain (the stratified permutation walks cycles of [0, spp) and need not terminate)
    const char* set_samples(const uint16_t* tile_samples, size_t n_tiles, int64_t uniform_first_sample, uint32_t n_passes, uint32_t sampler_spp) {
        sample_table = tile_samples != nullptr;
        accumulating = sample_table || uniform_first_sample >= 0;
        if (sample_table && uniform_first_sample >= 0) return "an accumulating tile list carries its own sample indices";
        if (n_passes == 0 || n_passes > 0xFFFFu || (!accumulating && n_passes != 1)) return "bad number of passes";
        spp = accumulating ? n_passes : sampler_spp;
        for (size_t t = 0; sample_table && t < n_tiles; ++t)
            if ((uint64_t)tile_samples[t] + n_passes > sampler_spp) return "FilmTile.sample (+ passes) beyond the sampler's samples per pixel";
        if (uniform_first_sample >= 0 && (uint64_t)uniform_first_sample + n_passes > sampler_spp)
            return "first_sample (+ passes) beyond the sampler's samples per pixel";
        sample_base = uniform_first_sample >= 0 ? (uint32_t)uniform_first_sample : 0u;
        return nullptr;
    }

    // after set_samples; off: tile_ranges' offsets
    const char* set_chunks(const uint32_t* off, size_t n_tiles, uint64_t sample_buf_cap) {
        total_px = off[n_tiles];
        total_work = total_px * spp;
        max_px_chunk = std::min<uint64_t>(0xFFFFFFF0ull / spp, sample_buf_cap / (16ull * spp));
        if (max_px_chunk == 0) return "sample_buf_cap too small for one pixel";
        chunks.clear();
        for (size_t t_begin = 0, t_end = 0; t_begin < n_tiles; t_begin = t_end) {
            while (t_end < n_tiles && (uint64_t)(off[t_end + 1] - off[t_begin]) <= max_px_chunk) ++t_end;
            if (t_end == t_begin) return "a single tile exceeds sample_buf_cap";
            chunks.push_back(Chunk{t_begin, t_end, off[t_begin], off[t_end] - off[t_begin]});
        }
        return nullptr;
    }

    // A pixel list instead of tiles (set_samples and set_chunks in one): n_pixels entries, each with its own first sample
    // index on the device, n_passes of them rendered; list_passes: the round size the list was made for; sample_end: the
    // host-known bound, sample + list_passes <= sample_end for every entry.  The entries' indices live on the device, so this
    // bound is what keeps a list from asking a sampler for an index outside its domain (the stratified permutation walk
    // need not end there).  Chunks are cut by pixel count — a list has no tile boundaries; t_begin / t_end stay 0.
    const char* set_pixel_list(uint64_t n_pixels, uint32_t n_passes, uint32_t list_passes, uint64_t sample_end, uint32_t sampler_spp, uint64_t sample_buf_cap) {
        accumulating = sample_table = true;
        if (n_passes == 0 || n_passes > 0xFFFFu || n_passes > list_passes) return "bad number of passes";
        if (sample_end > sampler_spp) return "pixel list: sample (+ passes) beyond the sampler's samples per pixel";
        if (n_pixels > 0xFFFFFFFFull) return "too many pixels in one call";
        spp = n_passes;
        sample_base = 0;
        total_px = n_pixels;
        total_work = total_px * spp;
        max_px_chunk = std::min<uint64_t>(0xFFFFFFF0ull / spp, sample_buf_cap / (16ull * spp));
        if (max_px_chunk == 0) return "sample_buf_cap too small for one pixel";
        chunks.clear();
        for (uint64_t px0 = 0; px0 < total_px; px0 += max_px_chunk) chunks.push_back(Chunk{0, 0, (uint32_t)px0, (uint32_t)std::min<uint64_t>(max_px_chunk, total_px - px0)});
        return nullptr;
    }

    // after set_chunks.  Work is cut into batches of <= batch_paths camera samples.  With streams >= 2 batches alternate
    // between two work sets / HIP streams, so the latency-bound tail launches of one batch (late bounces, few rays) run
    // beside the bulk launches of the other.  A job that fits one batch stays on one work set: splitting it gains nothing
    // once the side stream overlaps shadow rays with the next bounce (measured).
    void set_batch(uint64_t batch_paths, int64_t streams, bool is_path, bool caller_stream) {
        batch = (size_t)std::min<uint64_t>(batch_paths, total_work);
        n_ws = (streams >= 2 && is_path && !caller_stream && total_work > batch) ? 2 : 1;
    }

    // keep the per-batch work buffers (148 + 53 * n_lights + 36 bytes per path and work set) within half of the free HBM,
    // unless that leaves less than 65536 paths
    void clamp_batch_to_hbm(uint64_t free_bytes, unsigned n_lights) {
        const uint64_t per_path = (148 + 53 * (uint64_t)std::max(1u, n_lights) + 36) * (uint64_t)n_ws;
        const uint64_t fit = (free_bytes / 2) / per_path;
        if (fit >= 65536 && batch > fit) batch = (size_t)fit;
    }
};

}  // namespace yk_plan
