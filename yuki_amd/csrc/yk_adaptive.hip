// yk_adaptive.hip — adaptive sampling on gfx950: the selection that writes a pixel list, the fold of rendered samples into
// the film sums and the per-pixel statistics, and the resolve, behind yk_adaptive_select / _accumulate / _resolve, their
// _device forms and yk_pixel_list; the per-pixel arithmetic is yk_adaptive.h's, whose host instance these entry points run
// without a context.  Rendering a list and the driver are yk_render.cpp's.
//
// k_ad_select: one block of 256 lanes per 16 x 16 tile of the rule's order.  The lanes evaluate ad_wants and ad_eligible for
//   the tile plus a halo of one (18 x 18 pixels, one 16-byte load each, two flag bits a pixel in 324 bytes of LDS; outside
//   the film the flags are 0 and nothing is loaded), every lane reaches the barrier, then each dilates its own pixel from
//   LDS and the block scans the 256 flags (scan::block_excl_scan): the rank inside the tile goes to a per-pixel word (~0:
//   not selected), the tile's count to a per-tile word.
// scan::k_scan_sums: the tile counts become tile bases, the total lands behind them.  One block, any number of tiles.
// k_ad_emit: one block per tile again: a selected pixel writes (x | y << 16, drawn) at base + rank.  base + rank < total <=
//   res_x * res_y, the capacity of every list and of the staged arrays.
// k_ad_fold: one lane per list entry, two sources (a pass-major RGB buffer; a chunk's float4 sample buffer), one device
//   function.  Entries are unique pixels, so a lane owns its film triple and its record: no atomics.
// k_ad_resolve: streaming, one lane per pixel.
// The total is read back by the host (4 bytes, one synchronisation per selection): the batch plan of the render that
// follows needs it.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include "yk_adaptive.h"
#include "yk_film_call.h"
#include "yk_scan.h"
#include "yk_staging.h"

namespace {

__device__ inline yk_pixel_stats load_stats(const uint4* stats, size_t i) {
    const uint4 v = stats[i];
    yk_pixel_stats s;
    s.mean = __uint_as_float(v.x);
    s.m2 = __uint_as_float(v.y);
    s.n = v.z;
    s.drawn = v.w;
    return s;
}
__device__ inline void store_stats(uint4* stats, size_t i, const yk_pixel_stats& s) { stats[i] = make_uint4(__float_as_uint(s.mean), __float_as_uint(s.m2), s.n, s.drawn); }

const uint32_t AD_HALO = AD_TILE + 2;
const uint32_t AD_NOT_SELECTED = ~0u;

__global__ __launch_bounds__(AD_TILE* AD_TILE) void k_ad_select(AdParams a, uint32_t tiles_x, const uint4* stats, uint32_t* rank, uint32_t* tile_count) {
    __shared__ uint8_t flags[AD_HALO * AD_HALO];  // bit 0 wants, bit 1 eligible
    __shared__ uint32_t wt[16];
    const uint32_t tile = blockIdx.x;
    const int x0 = (int)((tile % tiles_x) * AD_TILE), y0 = (int)((tile / tiles_x) * AD_TILE);
    for (uint32_t k = threadIdx.x; k < AD_HALO * AD_HALO; k += blockDim.x) {
        const int gx = x0 + (int)(k % AD_HALO) - 1, gy = y0 + (int)(k / AD_HALO) - 1;
        uint8_t f = 0;
        if (gx >= 0 && gy >= 0 && gx < (int)a.res_x && gy < (int)a.res_y) {
            const yk_pixel_stats s = load_stats(stats, (size_t)gy * a.res_x + (size_t)gx);
            f = (uint8_t)((ad_wants(a, s) ? 1u : 0u) | (ad_eligible(a, s) ? 2u : 0u));
        }
        flags[k] = f;
    }
    __syncthreads();  // every lane of the block is here: none has returned
    const uint32_t lx = threadIdx.x % AD_TILE, ly = threadIdx.x / AD_TILE;
    const uint32_t x = (uint32_t)x0 + lx, y = (uint32_t)y0 + ly;
    const bool inside = x < a.res_x && y < a.res_y;
    bool sel = false;
    if (inside) {
        const bool eligible = (flags[(ly + 1) * AD_HALO + lx + 1] & 2u) != 0;
        sel = ad_selected(a, x, y, eligible, [&](uint32_t qx, uint32_t qy) { return (flags[((int)qy - y0 + 1) * (int)AD_HALO + ((int)qx - x0 + 1)] & 1u) != 0; });
    }
    uint32_t total;
    const uint32_t r = scan::block_excl_scan(sel ? 1u : 0u, total, wt);
    if (inside) rank[(size_t)y * a.res_x + x] = sel ? r : AD_NOT_SELECTED;
    if (threadIdx.x == 0) tile_count[tile] = total;
}

__global__ __launch_bounds__(AD_TILE* AD_TILE) void k_ad_emit(uint32_t res_x, uint32_t res_y, uint32_t tiles_x, const uint4* stats, const uint32_t* rank, const uint32_t* tile_base,
                                                              uint32_t* out_xy, uint32_t* out_sample) {
    const uint32_t tile = blockIdx.x;
    const uint32_t x = (tile % tiles_x) * AD_TILE + threadIdx.x % AD_TILE, y = (tile / tiles_x) * AD_TILE + threadIdx.x / AD_TILE;
    if (x >= res_x || y >= res_y) return;
    const size_t i = (size_t)y * res_x + x;
    const uint32_t r = rank[i];
    if (r == AD_NOT_SELECTED) return;
    const uint32_t at = tile_base[tile] + r;
    out_xy[at] = ad_entry_xy(x, y);
    out_sample[at] = reinterpret_cast<const uint32_t*>(stats)[4 * i + 3];  // drawn
}

// where entry e's k-th value comes from
struct FromPasses {  // n_passes x n x RGB, pass-major: k_resolve_passes' output
    const float* p;
    uint32_t n;
    __device__ void get(uint32_t e, uint32_t k, float* c) const {
        const float* q = p + ((size_t)k * n + e) * 3;
        c[0] = q[0];
        c[1] = q[1];
        c[2] = q[2];
    }
};
struct FromSamples {  // a chunk's sample buffer: float4, pixel-major, e * n_passes + k
    const float4* p;
    uint32_t n_passes;
    __device__ void get(uint32_t e, uint32_t k, float* c) const {
        const float4 v = p[(size_t)e * n_passes + k];
        c[0] = v.x;
        c[1] = v.y;
        c[2] = v.z;
    }
};
template <class From>
__device__ inline void ad_fold_entry(const From& from, uint32_t e, uint32_t n_passes, uint32_t xy, uint32_t res_x, float* film_sum, uint4* stats) {
    const size_t i = (size_t)(xy >> 16) * res_x + (xy & 0xFFFFu);
    float f[3] = {film_sum[3 * i], film_sum[3 * i + 1], film_sum[3 * i + 2]};
    yk_pixel_stats s = load_stats(stats, i);
    for (uint32_t k = 0; k < n_passes; ++k) {
        float c[3];
        from.get(e, k, c);
        ad_fold_sample(c, f, s);
    }
    film_sum[3 * i] = f[0];
    film_sum[3 * i + 1] = f[1];
    film_sum[3 * i + 2] = f[2];
    store_stats(stats, i, s);
}
template <class From>
__global__ __launch_bounds__(256) void k_ad_fold(From from, const uint32_t* pixel_xy, uint32_t n, uint32_t n_passes, uint32_t res_x, float* film_sum, uint4* stats) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    ad_fold_entry(from, e, n_passes, pixel_xy[e], res_x, film_sum, stats);
}

__global__ __launch_bounds__(256) void k_ad_resolve(uint32_t n_px, const float* film_sum, const uint4* stats, float* out_rgb, float* out_variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    const float f[3] = {film_sum[3 * (size_t)i], film_sum[3 * (size_t)i + 1], film_sum[3 * (size_t)i + 2]};
    float rgb[3], var;
    ad_resolve_pixel(f, load_stats(stats, i), rgb, var);
    if (out_rgb) {
        out_rgb[3 * (size_t)i] = rgb[0];
        out_rgb[3 * (size_t)i + 1] = rgb[1];
        out_rgb[3 * (size_t)i + 2] = rgb[2];
    }
    if (out_variance) out_variance[i] = var;
}

inline dim3 blocks_of(uint32_t n) { return dim3((n - 1) / 256 + 1); }

// The three launches on `st` into tables of res_x * res_y words, then the count: 4 bytes and one synchronisation.
yk_status enqueue_select(yk_context* ctx, hipStream_t st, const AdParams& a, const void* d_stats, uint32_t* d_xy, uint32_t* d_sample, uint32_t* out_n) {
    const uint32_t tiles_x = ad_tiles_x(a.res_x), n_tiles = tiles_x * ad_tiles_y(a.res_y);
    HIP_TRY(ctx, ctx->adaptive.rank.ensure((size_t)a.res_x * a.res_y * 4));
    HIP_TRY(ctx, ctx->adaptive.tile_count.ensure(((size_t)n_tiles + 1) * 4));
    uint32_t* rank = ctx->adaptive.rank.as<uint32_t>();
    uint32_t* tile_count = ctx->adaptive.tile_count.as<uint32_t>();
    const uint4* stats = reinterpret_cast<const uint4*>(d_stats);
    hipLaunchKernelGGL(k_ad_select, dim3(n_tiles), dim3(AD_TILE * AD_TILE), 0, st, a, tiles_x, stats, rank, tile_count);
    hipLaunchKernelGGL(scan::k_scan_sums, dim3(1), dim3(scan::kScanThreads), 0, st, tile_count, n_tiles, tile_count + n_tiles);
    hipLaunchKernelGGL(k_ad_emit, dim3(n_tiles), dim3(AD_TILE * AD_TILE), 0, st, a.res_x, a.res_y, tiles_x, stats, rank, tile_count, d_xy, d_sample);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, tile_count + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *out_n = total;
    return YK_OK;
}

// every entry inside the film, none twice
bool entries_ok(const uint32_t* xy, uint32_t n, uint32_t res_x, uint32_t res_y) {
    if ((uint64_t)n > (uint64_t)res_x * res_y) return false;
    std::vector<bool> seen((size_t)res_x * res_y, false);
    for (uint32_t e = 0; e < n; ++e) {
        const uint32_t x = xy[e] & 0xFFFFu, y = xy[e] >> 16;
        if (x >= res_x || y >= res_y) return false;
        const size_t i = (size_t)y * res_x + x;
        if (seen[i]) return false;
        seen[i] = true;
    }
    return true;
}

yk_status check_fold(const void* passes, uint32_t n, uint32_t n_passes, uint32_t res_x, uint32_t res_y, const void* film_sum, const void* stats) {
    if (!film_sum || !stats || res_x == 0 || res_y == 0 || n_passes == 0 || n_passes > 0xFFFFu || (n && !passes)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y, pass_bytes = (size_t)n * n_passes * 12;
    if (overlaps(film_sum, n_px * 12, stats, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
    if (pass_bytes && (overlaps(passes, pass_bytes, film_sum, n_px * 12) || overlaps(passes, pass_bytes, stats, n_px * 16))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status check_resolve(const void* film_sum, const void* stats, uint32_t res_x, uint32_t res_y, const void* out_rgb, const void* out_variance) {
    if (!film_sum || !stats || res_x == 0 || res_y == 0 || (!out_rgb && !out_variance)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    const void* outs[2] = {out_rgb, out_variance};
    const size_t out_bytes[2] = {n_px * 12, n_px * 4};
    for (int k = 0; k < 2; ++k)
        if (outs[k] && (overlaps(outs[k], out_bytes[k], film_sum, n_px * 12) || overlaps(outs[k], out_bytes[k], stats, n_px * 16))) return YK_ERR_INVALID_ARGUMENT;
    if (out_rgb && out_variance && overlaps(out_rgb, n_px * 12, out_variance, n_px * 4)) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

}  // namespace

namespace yk {
void launch_ad_fold_samples(hipStream_t s, const uint32_t* pixel_xy, uint32_t n, const float4* sample_buf, uint32_t n_passes, uint32_t res_x, float* film_sum, void* stats) {
    if (!n) return;
    hipLaunchKernelGGL((k_ad_fold<FromSamples>), blocks_of(n), dim3(256), 0, s, FromSamples{sample_buf, n_passes}, pixel_xy, n, n_passes, res_x, film_sum, reinterpret_cast<uint4*>(stats));
}
}  // namespace yk

yk_status adaptive_select_into(yk_context* ctx, hipStream_t st, const yk_adaptive_desc* desc, const void* d_stats, yk_pixel_list* list, uint32_t* out_n) {
    const AdParams a = ad_make_params(desc, list->res_x, list->res_y);
    list->n = 0;  // whatever happens below, the list never claims entries it does not hold
    uint32_t n = 0;
    yk_status s = enqueue_select(ctx, st, a, d_stats, list->pixel_xy.as<uint32_t>(), list->pixel_sample.as<uint32_t>(), &n);
    if (s != YK_OK) return s;
    list->n = n;
    list->passes = desc->round_passes;
    list->sample_end = desc->max_samples;
    *out_n = n;
    return YK_OK;
}

extern "C" {

yk_status yk_pixel_list_create(yk_context* ctx, uint16_t res_x, uint16_t res_y, yk_pixel_list** out) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!out || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_pixel_list_create: bad argument");
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    std::unique_ptr<yk_pixel_list> l(new yk_pixel_list());
    l->ctx = ctx;
    l->res_x = res_x;
    l->res_y = res_y;
    const size_t bytes = (size_t)res_x * res_y * 4;
    hipError_t e = l->pixel_xy.ensure(bytes);
    if (e == hipSuccess) e = l->pixel_sample.ensure(bytes);
    if (e != hipSuccess) {
        l->pixel_xy.release();
        l->pixel_sample.release();
        return fail(ctx, e == hipErrorOutOfMemory ? YK_ERR_OUT_OF_MEMORY : YK_ERR_DEVICE, std::string("yk_pixel_list_create: ") + hipGetErrorString(e));
    }
    *out = l.release();
    return YK_OK;
}
YK_CATCH(ctx)

void yk_pixel_list_destroy(yk_pixel_list* l) {
    if (!l) return;
    if (l->ctx) (void)hipSetDevice(l->ctx->device);
    l->pixel_xy.release();
    l->pixel_sample.release();
    delete l;
}

yk_status yk_pixel_list_set(yk_pixel_list* list, const uint32_t* xy, const uint32_t* sample, uint32_t n, uint32_t passes) try {
    if (!list || !list->ctx) return YK_ERR_INVALID_ARGUMENT;
    yk_context* ctx = list->ctx;
    YK_LOCK(ctx);
    if ((n && (!xy || !sample)) || passes == 0 || passes > 0xFFFFu) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_pixel_list_set: bad argument");
    if (!entries_ok(xy, n, list->res_x, list->res_y)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_pixel_list_set: a pixel outside the list's resolution, or a pixel twice");
    uint32_t end = passes;
    for (uint32_t e = 0; e < n; ++e) {
        if ((uint64_t)sample[e] + passes > (1u << 24)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_pixel_list_set: sample + passes beyond 2^24");
        end = std::max(end, sample[e] + passes);
    }
    (void)hipSetDevice(ctx->device);
    list->n = 0;
    if (n) {
        HIP_TRY(ctx, hipMemcpyAsync(list->pixel_xy.p, xy, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(list->pixel_sample.p, sample, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    list->n = n;
    list->passes = passes;
    list->sample_end = end;
    return YK_OK;
}
YK_CATCH(list ? list->ctx : nullptr)

yk_status yk_pixel_list_read(const yk_pixel_list* list, uint32_t* out_xy, uint32_t* out_sample, uint32_t cap, uint32_t* out_n) {
    if (!list || !list->ctx) return YK_ERR_INVALID_ARGUMENT;
    yk_context* ctx = list->ctx;
    YK_LOCK(ctx);
    if (!out_n) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_pixel_list_read: null out_n");
    *out_n = list->n;
    const size_t take = std::min(cap, list->n);
    if (!take) return YK_OK;
    (void)hipSetDevice(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (out_xy) HIP_TRY(ctx, hipMemcpy(out_xy, list->pixel_xy.p, take * 4, hipMemcpyDeviceToHost));
    if (out_sample) HIP_TRY(ctx, hipMemcpy(out_sample, list->pixel_sample.p, take * 4, hipMemcpyDeviceToHost));
    return YK_OK;
}

yk_status yk_adaptive_select(yk_context* ctx, const yk_adaptive_desc* desc, const yk_pixel_stats* stats, uint16_t res_x, uint16_t res_y, uint32_t* out_xy, uint32_t* out_sample,
                             uint32_t* out_n) try {
    if (!ad_desc_ok(desc) || !stats || !out_n || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_select: bad argument");
    const AdParams a = ad_make_params(desc, res_x, res_y);
    if (!ctx) {  // the host instance
        *out_n = ad_select_host(a, stats, out_xy, out_sample);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const yk_pixel_stats* d_stats = sg.upload(stats, n_px);
    uint32_t* d_xy = sg.temp<uint32_t>(n_px);
    uint32_t* d_sample = sg.temp<uint32_t>(n_px);
    if (!sg.ok()) return sg.status();
    uint32_t n = 0;
    yk_status s = enqueue_select(ctx, sg.stream, a, d_stats, d_xy, d_sample, &n);
    if (s != YK_OK) return s;
    if (n && out_xy) sg.check(hipMemcpyAsync(out_xy, d_xy, (size_t)n * 4, hipMemcpyDeviceToHost, sg.stream));
    if (n && out_sample) sg.check(hipMemcpyAsync(out_sample, d_sample, (size_t)n * 4, hipMemcpyDeviceToHost, sg.stream));
    *out_n = n;
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_adaptive_select_device(yk_context* ctx, const yk_adaptive_desc* desc, const void* d_stats, uint16_t res_x, uint16_t res_y, yk_pixel_list* list, uint32_t* out_n,
                                    void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!ad_desc_ok(desc) || !d_stats || !list || !out_n || res_x == 0 || res_y == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_select_device: bad argument");
    if (list->ctx != ctx || list->res_x != res_x || list->res_y != res_y)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_select_device: the list belongs to another context or has another resolution");
    if (misaligned(16, d_stats)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_select_device: statistics must be 16-byte aligned");
    return adaptive_select_into(ctx, device_call_stream(ctx, stream), desc, d_stats, list, out_n);
}

yk_status yk_adaptive_accumulate(yk_context* ctx, const uint32_t* xy, uint32_t n, const float* passes_rgb, uint32_t n_passes, uint16_t res_x, uint16_t res_y, float* film_sum,
                                 yk_pixel_stats* stats) try {
    if (check_fold(passes_rgb, n, n_passes, res_x, res_y, film_sum, stats) != YK_OK || (n && !xy)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate: bad argument");
    if (!entries_ok(xy, n, res_x, res_y)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate: a pixel outside the film, or a pixel twice");
    if (!ctx) {  // the host instance
        ad_fold_host(res_x, xy, n, passes_rgb, n_passes, film_sum, stats);
        return YK_OK;
    }
    if (n == 0) return YK_OK;
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const uint32_t* d_xy = sg.upload(xy, n);
    const float* d_passes = sg.upload(passes_rgb, (size_t)n * n_passes * 3);
    float* d_film = sg.inout(film_sum, n_px * 3);
    yk_pixel_stats* d_stats = sg.inout(stats, n_px);
    if (!sg.ok()) return sg.status();
    hipLaunchKernelGGL((k_ad_fold<FromPasses>), blocks_of(n), dim3(256), 0, sg.stream, FromPasses{d_passes, n}, d_xy, n, n_passes, (uint32_t)res_x, d_film, reinterpret_cast<uint4*>(d_stats));
    sg.check(hipGetLastError());
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_adaptive_accumulate_device(yk_context* ctx, const yk_pixel_list* list, const void* d_passes_rgb, uint32_t n_passes, uint16_t res_x, uint16_t res_y, void* d_film_sum,
                                        void* d_stats, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!list || check_fold(d_passes_rgb, list->n, n_passes, res_x, res_y, d_film_sum, d_stats) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate_device: bad argument");
    if (list->ctx != ctx || list->res_x != res_x || list->res_y != res_y)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate_device: the list belongs to another context or has another resolution");
    if (n_passes > list->passes) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate_device: more passes than the list was made for");
    if (misaligned(4, d_passes_rgb, d_film_sum) || misaligned(16, d_stats))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_accumulate_device: passes and film must be 4-byte aligned, statistics 16-byte aligned");
    hipStream_t st = device_call_stream(ctx, stream);
    if (list->n == 0) return YK_OK;
    hipLaunchKernelGGL((k_ad_fold<FromPasses>), blocks_of(list->n), dim3(256), 0, st, FromPasses{reinterpret_cast<const float*>(d_passes_rgb), list->n}, list->pixel_xy.as<uint32_t>(), list->n,
                       n_passes, (uint32_t)res_x, reinterpret_cast<float*>(d_film_sum), reinterpret_cast<uint4*>(d_stats));
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

yk_status yk_adaptive_resolve(yk_context* ctx, const float* film_sum, const yk_pixel_stats* stats, uint16_t res_x, uint16_t res_y, float* out_rgb, float* out_variance) try {
    if (check_resolve(film_sum, stats, res_x, res_y, out_rgb, out_variance) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_resolve: bad argument");
    if (!ctx) {  // the host instance
        ad_resolve_host(res_x, res_y, film_sum, stats, out_rgb, out_variance);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_sum, n_px * 3);
    const yk_pixel_stats* d_stats = sg.upload(stats, n_px);
    float* d_rgb = sg.output(out_rgb, n_px * 3);
    float* d_var = sg.output(out_variance, n_px);
    if (!sg.ok()) return sg.status();
    hipLaunchKernelGGL(k_ad_resolve, blocks_of((uint32_t)n_px), dim3(256), 0, sg.stream, (uint32_t)n_px, d_film, reinterpret_cast<const uint4*>(d_stats), d_rgb, d_var);
    sg.check(hipGetLastError());
    return sg.finish();
}
YK_CATCH(ctx)

yk_status yk_adaptive_resolve_device(yk_context* ctx, const void* d_film_sum, const void* d_stats, uint16_t res_x, uint16_t res_y, void* d_out_rgb, void* d_out_variance, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_resolve(d_film_sum, d_stats, res_x, res_y, d_out_rgb, d_out_variance) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_resolve_device: bad argument");
    if (misaligned(4, d_film_sum, d_out_rgb, d_out_variance) || misaligned(16, d_stats))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_adaptive_resolve_device: film, output and variance must be 4-byte aligned, statistics 16-byte aligned");
    const uint32_t n_px = (uint32_t)res_x * res_y;
    hipLaunchKernelGGL(k_ad_resolve, blocks_of(n_px), dim3(256), 0, device_call_stream(ctx, stream), n_px, reinterpret_cast<const float*>(d_film_sum), reinterpret_cast<const uint4*>(d_stats),
                       reinterpret_cast<float*>(d_out_rgb), reinterpret_cast<float*>(d_out_variance));
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

}  // extern "C"
