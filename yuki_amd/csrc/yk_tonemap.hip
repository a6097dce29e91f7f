// yk_tonemap.hip — the tone map of the film (app/renderpasses/tonemap.rs) on gfx950, behind yk_tone_map, yk_tone_map_device and
// yk_tone_map_metered_device and yk_film_min_max; the per-pixel arithmetic is yk_tonemap.h's, whose host instance these entry points run without a context.
//
// Two memory-bound passes over a row-major RGB film (12 bytes a pixel):
//   - k_tone_map: film -> out (out may be the film).  A lane maps 4 pixels through three 16-byte loads and three 16-byte
//     stores; pixels past the last whole group of 4 (and every pixel of a film or output not 16-byte aligned) go one at a
//     time.  Grid-stride over at most TM_MAX_BLOCKS blocks of TM_BLOCK threads.
//   - Heatmap without bounds: k_min_max_partial folds the film per wave (shuffles), per block (LDS) into one (min, max)
//     pair per block, k_min_max_final folds those pairs in one block into the context's bounds slot, and k_tone_map reads
//     the bounds from there: no host round trip, no float atomics.
// Everything the passes need on the device (partials, bounds slot, staged sample table) is grown in the context on first
// use; after that the stream-ordered entry point does not allocate, and it waits for the device only when it brings a sample
// table while the previous call's upload of one (out of the same pinned staging) has not run yet.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "yk_film_call.h"
#include "yk_staging.h"
#include "yk_tonemap.h"

namespace {

constexpr unsigned TM_BLOCK = 256;       // 4 waves of 64
constexpr unsigned TM_MAX_BLOCKS = 2048; // grid cap (8 blocks on each of 256 CUs); the rest is grid-strided

struct TmArgs {
    uint32_t kind, channel;
    float exposure;
    float lo, hi;              // Heatmap bounds given by the caller ...
    union {
        const float* bounds;              // ... or found on the device (bounds[0], bounds[1]); nullptr = use lo / hi
        const yk_exposure_state* state;   // k_tone_map<true> (Filmic, which has no bounds): the meter's record
    };
    const uint32_t* samples;   // Filmic: Film.samples in FilmTile.index order, or nullptr
    uint32_t res_x, tile_dim, x_tile_count;
};

__device__ __forceinline__ void tm_pixel(const TmArgs& a, float lo, float hi, uint32_t i, float& r, float& g, float& b) {
    if (a.kind == TM_FILMIC) {
        float count = 0.0f;
        if (a.samples) {
            const uint32_t y = i / a.res_x, x = i - y * a.res_x;
            count = (float)a.samples[tm_sample_index(x, y, a.tile_dim, a.x_tile_count)];
        }
        tm_filmic(count, a.exposure, r, g, b);
    } else if (a.kind == TM_HEATMAP) {
        tm_heatmap(a.channel, lo, hi, r, g, b);
    }
}

// film and out are deliberately not __restrict__: out == film (in place) is allowed; each lane reads its pixels before it
// writes them and touches no other lane's.  METERED (Filmic only): the exposure is a.exposure times the exposure of the
// meter's record (yk_exposure.h), read here once per lane as the Heatmap reads its bounds.  The record's pointer shares the
// bounds' place in TmArgs, so the unmetered instance keeps the kernel arguments and the code it had before there was a meter.
template <bool METERED> __global__ __launch_bounds__(TM_BLOCK) void k_tone_map(const float* film, float* out, uint32_t n_px, int vec, TmArgs a) {
    if (METERED) a.exposure = a.exposure * a.state->exposure;
    float lo = a.lo, hi = a.hi;
    if (!METERED && a.bounds) {
        lo = a.bounds[0];
        hi = a.bounds[1];
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_quads = vec ? n_px / 4 : 0;
    for (uint64_t q = tid; q < n_quads; q += stride) {
        const float4* src = reinterpret_cast<const float4*>(film) + 3 * q;
        const float4 v0 = src[0], v1 = src[1], v2 = src[2];
        float c[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) tm_pixel(a, lo, hi, (uint32_t)(4 * q + k), c[3 * k], c[3 * k + 1], c[3 * k + 2]);
        float4* dst = reinterpret_cast<float4*>(out) + 3 * q;
        dst[0] = make_float4(c[0], c[1], c[2], c[3]);
        dst[1] = make_float4(c[4], c[5], c[6], c[7]);
        dst[2] = make_float4(c[8], c[9], c[10], c[11]);
    }
    for (uint64_t i = 4 * n_quads + tid; i < n_px; i += stride) {
        float r = film[3 * i], g = film[3 * i + 1], b = film[3 * i + 2];
        tm_pixel(a, lo, hi, (uint32_t)i, r, g, b);
        out[3 * i] = r;
        out[3 * i + 1] = g;
        out[3 * i + 2] = b;
    }
}

__device__ __forceinline__ void tm_block_fold(float& lo, float& hi, float2* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float olo = __shfl_xor(lo, off, 64), ohi = __shfl_xor(hi, off, 64);
        if (olo < lo) lo = olo;
        if (ohi > hi) hi = ohi;
    }
    const unsigned wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0) lds[wave] = make_float2(lo, hi);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < blockDim.x / 64; ++w) {
            if (lds[w].x < lo) lo = lds[w].x;
            if (lds[w].y > hi) hi = lds[w].y;
        }
    }
}

// One (min, max) pair per block over its grid-strided pixels (find_min_max's fold, tm_fold).
__global__ __launch_bounds__(TM_BLOCK) void k_min_max_partial(const float* film, uint32_t n_px, int vec, uint32_t channel, float2* partials) {
    __shared__ float2 lds[TM_BLOCK / 64];
    float lo = FLT_MAX, hi = -FLT_MAX;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n_quads = vec ? n_px / 4 : 0;
    for (uint64_t q = tid; q < n_quads; q += stride) {
        const float4* src = reinterpret_cast<const float4*>(film) + 3 * q;
        const float4 v0 = src[0], v1 = src[1], v2 = src[2];
        tm_fold(tm_bounds_value(channel, v0.x, v0.y, v0.z), lo, hi);
        tm_fold(tm_bounds_value(channel, v0.w, v1.x, v1.y), lo, hi);
        tm_fold(tm_bounds_value(channel, v1.z, v1.w, v2.x), lo, hi);
        tm_fold(tm_bounds_value(channel, v2.y, v2.z, v2.w), lo, hi);
    }
    for (uint64_t i = 4 * n_quads + tid; i < n_px; i += stride) tm_fold(tm_bounds_value(channel, film[3 * i], film[3 * i + 1], film[3 * i + 2]), lo, hi);
    tm_block_fold(lo, hi, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(lo, hi);
}

// One block: the partial pairs -> bounds[0..1].
__global__ __launch_bounds__(TM_BLOCK) void k_min_max_final(const float2* partials, uint32_t n, float* bounds) {
    __shared__ float2 lds[TM_BLOCK / 64];
    float lo = FLT_MAX, hi = -FLT_MAX;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float2 p = partials[i];
        if (p.x < lo) lo = p.x;
        if (p.y > hi) hi = p.y;
    }
    tm_block_fold(lo, hi, lds);
    if (threadIdx.x == 0) {
        bounds[0] = lo;
        bounds[1] = hi;
    }
}

unsigned tm_grid(uint32_t n_px, bool vec) {
    const uint64_t items = vec ? std::max<uint64_t>(n_px / 4, 1) : n_px;
    return (unsigned)std::min<uint64_t>((items + TM_BLOCK - 1) / TM_BLOCK, TM_MAX_BLOCKS);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

yk_status check_desc(const yk_tone_map_desc* d) {
    if (!d || d->kind > YK_TONE_MAP_HEATMAP) return YK_ERR_INVALID_ARGUMENT;
    if (d->kind == YK_TONE_MAP_HEATMAP && d->channel > YK_HEATMAP_LUMINANCE) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

}  // namespace

// The caller's table is copied into pinned staging, so that the upload is truly asynchronous; the staging is rewritten only
// once the previous call's upload out of it has run (normally long done).
yk_status stage_sample_table(yk_context* ctx, hipStream_t st, const uint32_t* samples, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, DevBuf& dst) {
    const size_t words = (size_t)((res_x + tile_dim - 1) / tile_dim) * (size_t)((res_y + tile_dim - 1) / tile_dim);
    auto& tm = ctx->tonemap;
    HIP_TRY(ctx, dst.ensure(words * 4));
    if (words > tm.staging_words) {
        if (tm.staging) HIP_TRY(ctx, hipHostFree(tm.staging));
        tm.staging = nullptr;
        tm.staging_words = 0;
        HIP_TRY(ctx, hipHostMalloc((void**)&tm.staging, words * 4, hipHostMallocDefault));
        tm.staging_words = words;
    }
    if (!tm.staged) HIP_TRY(ctx, hipEventCreateWithFlags(&tm.staged, hipEventDisableTiming));
    else HIP_TRY(ctx, hipEventSynchronize(tm.staged));
    std::memcpy(tm.staging, samples, words * 4);
    HIP_TRY(ctx, hipMemcpyAsync(dst.p, tm.staging, words * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(tm.staged, st));
    return YK_OK;
}

namespace {

// The device passes on `st`; a Heatmap without bounds leaves the bounds it found in the context's slot (tm.bounds).
yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_tone_map_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                  const uint32_t* samples, float* out, const yk_exposure_state* d_state = nullptr) {
    const uint32_t n_px = (uint32_t)res_x * res_y;
    const bool vec = aligned16(film) && aligned16(out);
    auto& tm = ctx->tonemap;
    TmArgs a{};
    a.kind = d->kind;
    a.channel = d->channel;
    a.exposure = d->exposure;
    a.lo = d->bounds[0];
    a.hi = d->bounds[1];
    a.res_x = res_x;
    a.tile_dim = tile_dim;
    a.x_tile_count = res_x / tile_dim;
    if (d->kind == YK_TONE_MAP_RAW) {
        if (film != out) HIP_TRY(ctx, hipMemcpyAsync(out, film, (size_t)n_px * 12, hipMemcpyDeviceToDevice, st));
        return YK_OK;
    }
    if (d->kind == YK_TONE_MAP_FILMIC)
        if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, tm.samples, &a.samples)) return ss;
    if (d->kind == YK_TONE_MAP_HEATMAP && !d->has_bounds) {
        HIP_TRY(ctx, tm.partials.ensure(TM_MAX_BLOCKS * sizeof(float2)));
        HIP_TRY(ctx, tm.bounds.ensure(256));
        const unsigned g = tm_grid(n_px, vec);
        hipLaunchKernelGGL(k_min_max_partial, dim3(g), dim3(TM_BLOCK), 0, st, film, n_px, vec ? 1 : 0, d->channel, tm.partials.as<float2>());
        hipLaunchKernelGGL(k_min_max_final, dim3(1), dim3(TM_BLOCK), 0, st, tm.partials.as<const float2>(), g, tm.bounds.as<float>());
        a.bounds = tm.bounds.as<const float>();
    }
    if (d_state) {
        a.state = d_state;
        hipLaunchKernelGGL(k_tone_map<true>, dim3(tm_grid(n_px, vec)), dim3(TM_BLOCK), 0, st, film, out, n_px, vec ? 1 : 0, a);
    } else {
        hipLaunchKernelGGL(k_tone_map<false>, dim3(tm_grid(n_px, vec)), dim3(TM_BLOCK), 0, st, film, out, n_px, vec ? 1 : 0, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

yk_status check_call(const yk_tone_map_desc* desc, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* out) {
    if (check_desc(desc) != YK_OK || !film || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

void host_min_max(const float* film, size_t n_px, uint32_t channel, float* lo_hi) {
    float lo = FLT_MAX, hi = -FLT_MAX;
    for (size_t i = 0; i < n_px; ++i) tm_fold(tm_bounds_value(channel, film[3 * i], film[3 * i + 1], film[3 * i + 2]), lo, hi);
    lo_hi[0] = lo;
    lo_hi[1] = hi;
}

}  // namespace

extern "C" {

yk_status yk_tone_map(yk_context* ctx, const yk_tone_map_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                      const uint32_t* samples, float* out_rgb, float* used_bounds) try {
    if (check_call(desc, film_rgb, res_x, res_y, tile_dim, out_rgb) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_tone_map: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    yk_tone_map_desc d = *desc;
    if (!ctx) {  // the host instance
        if (d.kind == YK_TONE_MAP_HEATMAP && !d.has_bounds) {
            host_min_max(film_rgb, n_px, d.channel, d.bounds);
            d.has_bounds = 1;
        }
        const uint32_t xt = res_x / tile_dim;
        for (size_t i = 0; i < n_px; ++i) {
            float r = film_rgb[3 * i], g = film_rgb[3 * i + 1], b = film_rgb[3 * i + 2];
            if (d.kind == YK_TONE_MAP_FILMIC) {
                const uint32_t y = (uint32_t)(i / res_x), x = (uint32_t)(i % res_x);
                tm_filmic(samples ? (float)samples[tm_sample_index(x, y, tile_dim, xt)] : 0.0f, d.exposure, r, g, b);
            } else if (d.kind == YK_TONE_MAP_HEATMAP) {
                tm_heatmap(d.channel, d.bounds[0], d.bounds[1], r, g, b);
            }
            out_rgb[3 * i] = r;
            out_rgb[3 * i + 1] = g;
            out_rgb[3 * i + 2] = b;
        }
        if (used_bounds && d.kind == YK_TONE_MAP_HEATMAP) std::memcpy(used_bounds, d.bounds, 8);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    float* d_out = sg.output(out_rgb, n_px * 3);
    if (!sg.ok()) return sg.status();
    yk_status s = enqueue(ctx, sg.stream, &d, d_film, res_x, res_y, tile_dim, samples, d_out);
    if (s != YK_OK) return s;
    sg.download();
    if (used_bounds && d.kind == YK_TONE_MAP_HEATMAP) {  // the bounds the device found follow the frame
        if (d.has_bounds) std::memcpy(used_bounds, d.bounds, 8);
        else sg.check(hipMemcpyAsync(used_bounds, ctx->tonemap.bounds.p, 8, hipMemcpyDeviceToHost, sg.stream));
    }
    return sg.finish();
} YK_CATCH(ctx)

yk_status yk_tone_map_device(yk_context* ctx, const yk_tone_map_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                             const uint32_t* samples, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(desc, d_film_rgb, res_x, res_y, tile_dim, d_out_rgb) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_tone_map_device: bad argument");
    return enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, reinterpret_cast<float*>(d_out_rgb));
}

yk_status yk_tone_map_metered_device(yk_context* ctx, const yk_tone_map_desc* desc, const void* d_state, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                                     const uint32_t* samples, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(desc, d_film_rgb, res_x, res_y, tile_dim, d_out_rgb) != YK_OK || !d_state) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_tone_map_metered_device: bad argument");
    if (desc->kind != YK_TONE_MAP_FILMIC) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_tone_map_metered_device: only the Filmic tone map has an exposure");
    if (misaligned(4, d_state)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_tone_map_metered_device: d_state needs 4-byte alignment");
    return enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, reinterpret_cast<float*>(d_out_rgb),
                   reinterpret_cast<const yk_exposure_state*>(d_state));
}

yk_status yk_film_min_max(yk_context* ctx, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint32_t channel, float out_min_max[2]) try {
    if (!film_rgb || !out_min_max || res_x == 0 || res_y == 0 || channel > YK_HEATMAP_LUMINANCE)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_film_min_max: bad argument");
    const size_t n_px = (size_t)res_x * res_y;
    if (!ctx) {
        host_min_max(film_rgb, n_px, channel, out_min_max);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    hipStream_t st = sg.stream;
    auto& tm = ctx->tonemap;
    sg.check(tm.partials.ensure(TM_MAX_BLOCKS * sizeof(float2)));
    sg.check(tm.bounds.ensure(256));
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    if (!sg.ok()) return sg.status();
    const unsigned g = tm_grid((uint32_t)n_px, true);
    hipLaunchKernelGGL(k_min_max_partial, dim3(g), dim3(TM_BLOCK), 0, st, d_film, (uint32_t)n_px, 1, channel, tm.partials.as<float2>());
    hipLaunchKernelGGL(k_min_max_final, dim3(1), dim3(TM_BLOCK), 0, st, tm.partials.as<const float2>(), g, tm.bounds.as<float>());
    sg.check(hipGetLastError());
    sg.check(hipMemcpyAsync(out_min_max, tm.bounds.p, 8, hipMemcpyDeviceToHost, st));
    return sg.finish();
} YK_CATCH(ctx)

}  // extern "C"
