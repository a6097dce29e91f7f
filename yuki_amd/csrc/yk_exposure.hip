// yk_exposure.hip — the exposure meter (yk_exposure.h) on gfx950, behind yk_film_histogram, yk_exposure_meter and
// yk_exposure_meter_device; without a context these entry points run the header's host instance.
//
// Two passes, stream-ordered, no float atomics and no float reduction:
//   - k_meter_hist: the film (12 bytes a pixel, read as k_tone_map reads it: three 16-byte loads for four pixels a lane
//     where film and table allow, one pixel at a time otherwise and for the tail; grid-stride over at most EX_MAX_BLOCKS
//     blocks) into a histogram of the block in LDS with LDS integer atomics; each block then adds its non-zero words to one of
//     the context's EX_SUB_SLOTS slots (block index modulo) with integer global atomics.  The slots are zeroed on the
//     stream before the pass.  Integer additions commute, so the sums do not depend on the order the blocks arrive in.
//     (Per-block slabs summed by the final kernel would be as exact, but leave one block to read 2048 x 1040 bytes; one slot
//     for all blocks put 2048 atomics in a row on every word, which cost more than reading the film: DESIGN.md §7.12.)
//     A flat wall puts every lane of a wave on one LDS word; with "exposure_wave_combine" (default) a wave that finds all its
//     active lanes on one word adds their number once.
//   - k_meter_final: one block, one bin a thread: the slots summed per bin, a block scan of the counts, the cut's clamp, an int64 block sum (integer,
//     so its order does not matter), and one lane runs ex_finish — reading the previous record before it writes the new
//     one, which may be the same record.
// The slot and the staged sample table belong to the context and are grown on first use; after that
// yk_exposure_meter_device neither allocates nor waits (but for the sample table's pinned staging: yk_tone_map_device's rule).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "yk_exposure.h"
#include "yk_film_call.h"
#include "yk_staging.h"

namespace {

constexpr unsigned EX_BLOCK = 256;        // 4 waves of 64; k_meter_final: one thread a bin
constexpr unsigned EX_MAX_BLOCKS = 2048;  // the tone map's grid cap; the rest is grid-strided
constexpr unsigned EX_SUB_SLOTS = 32;     // slots the blocks' histograms are spread over (one slot serialised 2048 atomics per word)
static_assert(EX_BLOCK == EX_BINS, "k_meter_final has one thread a bin");

struct MeterArgs {
    const uint32_t* samples;  // Film.samples in FilmTile.index order, or nullptr
    uint32_t res_x, tile_dim, x_tile_count;
    uint32_t x0, y0, x1, y1;  // the window
    uint32_t need_xy;         // a table or a window smaller than the film: the pixel's coordinates are needed
};

// One more sample for word `w` of the block's histogram.  COMBINE: the active lanes of the wave that share the first one's
// word (all of them on a flat wall) add once.
template <bool COMBINE> __device__ __forceinline__ void ex_count(uint32_t* h, uint32_t w) {
    if (COMBINE) {
        const unsigned long long active = __ballot(1);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)w);
        if (__ballot(w == first) == active) {
            if ((threadIdx.x & 63u) == (uint32_t)(__ffsll(active) - 1)) atomicAdd(&h[first], (uint32_t)__popcll(active));
            return;
        }
    }
    atomicAdd(&h[w], 1u);
}

template <bool COMBINE> __device__ __forceinline__ void ex_meter_pixel(const MeterArgs& a, uint32_t* h, uint32_t i, float r, float g, float b) {
    float count = 0.0f;
    if (a.need_xy) {
        const uint32_t y = i / a.res_x, x = i - y * a.res_x;
        if (x < a.x0 || x >= a.x1 || y < a.y0 || y >= a.y1) return;
        if (a.samples) count = (float)a.samples[tm_sample_index(x, y, a.tile_dim, a.x_tile_count)];
    }
    uint32_t edge;
    const uint32_t w = ex_bin(ex_pixel_luminance(count, r, g, b), &edge);
    ex_count<COMBINE>(h, w);
    if (edge) atomicAdd(&h[edge], 1u);
}

template <bool COMBINE> __global__ __launch_bounds__(EX_BLOCK) void k_meter_hist(const float* __restrict__ film, uint32_t n_px, int vec, MeterArgs a, uint32_t* __restrict__ slots) {
    __shared__ uint32_t h[EX_SLOT_WORDS];
    for (uint32_t k = threadIdx.x; k < EX_SLOT_WORDS; k += EX_BLOCK) h[k] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_quads = vec ? n_px / 4 : 0;
    for (uint64_t q = tid; q < n_quads; q += stride) {
        const float4* src = reinterpret_cast<const float4*>(film) + 3 * q;
        const float4 v0 = src[0], v1 = src[1], v2 = src[2];
        const uint32_t i = (uint32_t)(4 * q);
        ex_meter_pixel<COMBINE>(a, h, i, v0.x, v0.y, v0.z);
        ex_meter_pixel<COMBINE>(a, h, i + 1, v0.w, v1.x, v1.y);
        ex_meter_pixel<COMBINE>(a, h, i + 2, v1.z, v1.w, v2.x);
        ex_meter_pixel<COMBINE>(a, h, i + 3, v2.y, v2.z, v2.w);
    }
    for (uint64_t i = 4 * n_quads + tid; i < n_px; i += stride) ex_meter_pixel<COMBINE>(a, h, (uint32_t)i, film[3 * i], film[3 * i + 1], film[3 * i + 2]);
    __syncthreads();
    uint32_t* mine = slots + (blockIdx.x % EX_SUB_SLOTS) * EX_SLOT_WORDS;  // blocks b, b + EX_SUB_SLOTS, ... share a slot
    for (uint32_t k = threadIdx.x; k < EX_SLOT_WORDS; k += EX_BLOCK) {
        const uint32_t c = h[k];
        if (c) atomicAdd(&mine[k], c);
    }
}

// One block of EX_BINS threads: the slots -> the record.  prev may be nullptr and may be out.
__global__ __launch_bounds__(EX_BLOCK) void k_meter_final(const uint32_t* slots, yk_exposure_desc d, const yk_exposure_state* prev, yk_exposure_state* out) {
    __shared__ uint32_t wt[EX_BLOCK / 64];
    __shared__ long long wave_s[EX_BLOCK / 64];
    __shared__ uint32_t wave_k[EX_BLOCK / 64];
    __shared__ uint32_t side[3];  // skipped, below, above
    const uint32_t bin = threadIdx.x;
    uint32_t c = 0, sd = 0;
    for (uint32_t k = 0; k < EX_SUB_SLOTS; ++k) {
        c += slots[k * EX_SLOT_WORDS + bin];
        if (bin < 3) sd += slots[k * EX_SLOT_WORDS + EX_SKIPPED + bin];
    }
    if (bin < 3) side[bin] = sd;
    // the block's exclusive scan: inside each wave by shuffles, the four wave sums through LDS
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= (uint32_t)off) inc += o;
    }
    if (lane == 63u) wt[wave] = inc;
    __syncthreads();
    uint32_t before = inc - c, N = 0;
    for (uint32_t w = 0; w < EX_BLOCK / 64; ++w) {
        if (w < wave) before += wt[w];
        N += wt[w];
    }
    uint32_t n_lo, n_top;
    ex_cut(N, d.low_cut, d.high_cut, &n_lo, &n_top);
    uint32_t kept = ex_kept(before, before + c, n_lo, n_top);
    long long s = (long long)kept * (long long)ex_bin_value(bin);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        kept += __shfl_xor(kept, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        wave_s[threadIdx.x >> 6] = s;
        wave_k[threadIdx.x >> 6] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long S = 0;
        uint32_t K = 0;
        for (unsigned w = 0; w < EX_BLOCK / 64; ++w) {
            S += wave_s[w];
            K += wave_k[w];
        }
        ex_finish(d, N, K, (int64_t)S, side[0], side[1], side[2], prev, out);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the whole film as a window
void full_window(uint16_t res_x, uint16_t res_y, uint16_t w[4]) {
    w[0] = 0;
    w[1] = 0;
    w[2] = res_x;
    w[3] = res_y;
}

// What every entry point here refuses about the film and the window, or nullptr.
const char* film_refusal(const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint16_t window[4]) {
    if (!film) return "film is NULL";
    if (res_x == 0 || res_y == 0) return "zero resolution";
    if (tile_dim == 0) return "tile_dim is 0";
    if (!(window[0] < window[2] && window[2] <= res_x && window[1] < window[3] && window[3] <= res_y)) return "window needs x0 < x1 <= res_x and y0 < y1 <= res_y";
    return nullptr;
}

yk_status refuse(yk_context* ctx, const char* name, const char* why) { return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": " + why); }

// The histogram pass on `st` into the context's slots.
yk_status hist_enqueue(yk_context* ctx, hipStream_t st, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const uint16_t window[4]) {
    auto& ex = ctx->exposure;
    const uint32_t n_px = (uint32_t)res_x * res_y;
    MeterArgs a{};
    if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, ex.samples, &a.samples)) return ss;
    a.res_x = res_x;
    a.tile_dim = tile_dim;
    a.x_tile_count = res_x / tile_dim;
    a.x0 = window[0];
    a.y0 = window[1];
    a.x1 = window[2];
    a.y1 = window[3];
    a.need_xy = (a.samples || a.x0 != 0 || a.y0 != 0 || a.x1 != res_x || a.y1 != res_y) ? 1u : 0u;
    HIP_TRY(ctx, ex.slot.ensure(EX_SUB_SLOTS * EX_SLOT_WORDS * 4));
    HIP_TRY(ctx, hipMemsetAsync(ex.slot.p, 0, EX_SUB_SLOTS * EX_SLOT_WORDS * 4, st));
    const bool vec = aligned16(film);
    const uint64_t items = vec ? std::max<uint64_t>(n_px / 4, 1) : n_px;
    const unsigned grid = (unsigned)std::min<uint64_t>((items + EX_BLOCK - 1) / EX_BLOCK, EX_MAX_BLOCKS);
    if (ex.wave_combine) hipLaunchKernelGGL(k_meter_hist<true>, dim3(grid), dim3(EX_BLOCK), 0, st, film, n_px, vec ? 1 : 0, a, ex.slot.as<uint32_t>());
    else hipLaunchKernelGGL(k_meter_hist<false>, dim3(grid), dim3(EX_BLOCK), 0, st, film, n_px, vec ? 1 : 0, a, ex.slot.as<uint32_t>());
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// Both passes on `st`: the film -> *d_out.
yk_status meter_enqueue(yk_context* ctx, hipStream_t st, const yk_exposure_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                        const yk_exposure_state* d_prev, yk_exposure_state* d_out) {
    if (yk_status s = hist_enqueue(ctx, st, film, res_x, res_y, tile_dim, samples, d->window)) return s;
    hipLaunchKernelGGL(k_meter_final, dim3(1), dim3(EX_BLOCK), 0, st, ctx->exposure.slot.as<const uint32_t>(), *d, d_prev, d_out);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// The host instance: the film -> a slot's words ...
void host_histogram(const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const uint16_t window[4], uint32_t slot[EX_SLOT_WORDS]) {
    std::memset(slot, 0, EX_SLOT_WORDS * 4);
    const uint32_t xt = res_x / tile_dim;
    for (uint32_t y = window[1]; y < window[3]; ++y)
        for (uint32_t x = window[0]; x < window[2]; ++x) {
            const float* p = film + 3 * ((size_t)y * res_x + x);
            const float count = samples ? (float)samples[tm_sample_index(x, y, tile_dim, xt)] : 0.0f;
            uint32_t edge;
            slot[ex_bin(ex_pixel_luminance(count, p[0], p[1], p[2]), &edge)] += 1;
            if (edge) slot[edge] += 1;
        }
}

// ... and a slot -> the record
void host_finish(const yk_exposure_desc* d, const uint32_t slot[EX_SLOT_WORDS], const yk_exposure_state* prev, yk_exposure_state* out) {
    uint32_t N = 0;
    for (uint32_t b = 0; b < EX_BINS; ++b) N += slot[b];
    uint32_t n_lo, n_top, cum = 0, K = 0;
    ex_cut(N, d->low_cut, d->high_cut, &n_lo, &n_top);
    int64_t S = 0;
    for (uint32_t b = 0; b < EX_BINS; ++b) {
        const uint32_t kept = ex_kept(cum, cum + slot[b], n_lo, n_top);
        cum += slot[b];
        K += kept;
        S += (int64_t)kept * ex_bin_value(b);
    }
    ex_finish(*d, N, K, S, slot[EX_SKIPPED], slot[EX_BELOW], slot[EX_ABOVE], prev, out);
}

}  // namespace

extern "C" {

yk_status yk_film_histogram(yk_context* ctx, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const uint16_t window[4],
                            uint32_t out_bins[256], uint32_t out_skipped_below_above[3]) try {
    uint16_t win[4];
    if (window) std::memcpy(win, window, 8);
    else full_window(res_x, res_y, win);
    if (const char* why = film_refusal(film_rgb, res_x, res_y, tile_dim, win)) return refuse(ctx, "yk_film_histogram", why);
    if (!out_bins && !out_skipped_below_above) return refuse(ctx, "yk_film_histogram", "no output");
    uint32_t slot[EX_SLOT_WORDS];
    if (!ctx) {
        host_histogram(film_rgb, res_x, res_y, tile_dim, samples, win, slot);
    } else {
        YK_LOCK(ctx);
        Staging sg(ctx);
        const float* d_film = sg.upload(film_rgb, (size_t)res_x * res_y * 3);
        if (!sg.ok()) return sg.status();
        if (yk_status s = hist_enqueue(ctx, sg.stream, d_film, res_x, res_y, tile_dim, samples, win)) return s;
        std::vector<uint32_t> slots(EX_SUB_SLOTS * EX_SLOT_WORDS);
        sg.check(hipMemcpyAsync(slots.data(), ctx->exposure.slot.p, slots.size() * 4, hipMemcpyDeviceToHost, sg.stream));
        if (yk_status s = sg.finish()) return s;
        std::memset(slot, 0, sizeof(slot));
        for (size_t k = 0; k < slots.size(); ++k) slot[k % EX_SLOT_WORDS] += slots[k];
    }
    if (out_bins) std::memcpy(out_bins, slot, EX_BINS * 4);
    if (out_skipped_below_above) std::memcpy(out_skipped_below_above, slot + EX_SKIPPED, 12);
    return YK_OK;
} YK_CATCH(ctx)

yk_status yk_exposure_meter(yk_context* ctx, const yk_exposure_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                            const yk_exposure_state* prev, yk_exposure_state* out) try {
    if (const char* why = ex_desc_refusal(desc, res_x, res_y)) return refuse(ctx, "yk_exposure_meter", why);
    if (const char* why = film_refusal(film_rgb, res_x, res_y, tile_dim, desc->window)) return refuse(ctx, "yk_exposure_meter", why);
    if (!out) return refuse(ctx, "yk_exposure_meter", "out is NULL");
    if (!ctx) {
        uint32_t slot[EX_SLOT_WORDS];
        host_histogram(film_rgb, res_x, res_y, tile_dim, samples, desc->window, slot);
        host_finish(desc, slot, prev, out);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const float* d_film = sg.upload(film_rgb, (size_t)res_x * res_y * 3);
    const yk_exposure_state* d_prev = prev ? sg.upload(prev, 1) : nullptr;
    yk_exposure_state* d_out = sg.output(out, 1);
    return sg.run([&] { return meter_enqueue(ctx, sg.stream, desc, d_film, res_x, res_y, tile_dim, samples, d_prev, d_out); });
} YK_CATCH(ctx)

yk_status yk_exposure_meter_device(yk_context* ctx, const yk_exposure_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                   const void* d_prev, void* d_out_state, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (const char* why = ex_desc_refusal(desc, res_x, res_y)) return refuse(ctx, "yk_exposure_meter_device", why);
    if (const char* why = film_refusal(d_film_rgb, res_x, res_y, tile_dim, desc->window)) return refuse(ctx, "yk_exposure_meter_device", why);
    if (!d_out_state) return refuse(ctx, "yk_exposure_meter_device", "d_out_state is NULL");
    if (misaligned(4, d_film_rgb, d_prev, d_out_state)) return refuse(ctx, "yk_exposure_meter_device", "film and states need 4-byte alignment");
    return meter_enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples,
                         reinterpret_cast<const yk_exposure_state*>(d_prev), reinterpret_cast<yk_exposure_state*>(d_out_state));
}

}  // extern "C"
