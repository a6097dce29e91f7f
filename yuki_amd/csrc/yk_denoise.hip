// yk_denoise.hip — the edge-avoiding à-trous filter on gfx950, behind yk_denoise, yk_denoise_albedo and yk_denoise_variance
// and their _device forms; the per-pixel arithmetic is yk_denoise.h's, yk_albedo.h's and yk_variance.h's, whose host
// instance these entry points run without a context.
//
// One kernel template, k_atrous<Rule, IN_RGB, OUT, S>, one driver, enqueue_atrous, and one host loop, atrous_host, serve
// the three denoisers.  One launch per iteration, one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h;
// a wave covers two rows of 32 pixels).  A tap is 48 bytes — a 16-byte colour record and a guide record of two 16-byte
// loads — 25 of them a pixel, nearly all re-read from cache.
//   Rule    DnRule: dn_pixel with the colour stop sigma_color / 2^i, records (r, g, b, 0); VrRule: vr_pixel, whose colour
//           stop follows the variance in the records' fourth float (the 3 x 3 variance taps lie inside every halo);
//   IN_RGB  iteration 0 of the plain denoise reads the RGB film (dword loads: 4-byte alignment) and normalises it by the
//           sample table per fetched pixel; everything else reads the records of the context's two ping-pong buffers;
//   OUT     records, or for the last iteration RGB, or RGB multiplied by the divisors of the pixel's own albedo record
//           where there is one (al_remodulate: one extra 16-byte load a pixel);
//   S == 0  every tap from global memory;
//   S == 1, 2  the block first stages the colours (normalised once per staged pixel) and guides of its tile plus a halo
//           of 2*S pixels in LDS, and the taps are ds_read_b128s — for the steps whose halo is small against the tile.
// "denoise_lds_max_step" picks S per step (the measurement that chose the default).  The 21 instantiations
// are the launches enqueue_atrous can make: 12 of the plain denoise, 3 last iterations with an albedo, 6 variance-guided.
// The demodulated and the variance-guided denoise begin with k_dn_prepare, which writes the normalised film — divided by
// the albedo, beside the sanitised variance — as records; the plain denoise does not: its first iteration reads the film
// itself.
// Everything the passes need on the device (ping-pong buffers, staged sample table) is grown in the context on first use;
// after that the stream-ordered entry points do not allocate.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "yk_albedo.h"
#include "yk_denoise.h"
#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_staging.h"
#include "yk_variance.h"

namespace {

struct AtIo {
    const float* film;        // the RGB film ...
    const uint32_t* samples;  // ... and its sample table (may be NULL): iteration 0 of the plain denoise, the preparing pass
    const float4* in;         // the previous iteration's colour records
    const float4* guides;     // two float4 a pixel: (ns, hit), (p, t)
    const float4* albedo;     // may be NULL
    float4* out;              // colour records, or ...
    float* out_rgb;           // ... the last iteration's RGB
};

enum : int { OUT_RECORDS, OUT_RGB, OUT_RGB_ALBEDO };

// The two pixel rules as the kernel, the driver and the host loop see them: the tap a rule reads, filled from a colour
// record (WIDTH floats of it on the host) and the two halves of a guide record; what it computes per iteration on the
// host and carries to the device; its pixel.
struct DnRule {
    using Tap = DnTap;
    static constexpr int WIDTH = 3;  // a colour record's fourth float is 0 and is not read
    DnParams a;
    float den_c;
    YK_HD const DnParams& grid() const { return a; }
    void begin_iteration(uint32_t i) { den_c = dn_color_denominator(a.sigma_color, i); }
    static YK_HD void set_tap(Tap& t, const float* c, const float* ga, const float* gb) {
        t.c[0] = c[0];
        t.c[1] = c[1];
        t.c[2] = c[2];
        dn_guide(ga, gb, t.ns, t.hit, t.p);
    }
    template <class Fetch, class FetchVar>
    YK_HD void pixel(int s, uint32_t x, uint32_t y, const Fetch& fetch, const FetchVar&, float* out) const {
        dn_pixel(a, den_c, s, x, y, fetch, out);
    }
};
struct VrRule {
    using Tap = VrFilterTap;
    static constexpr int WIDTH = 4;
    VrParams a;
    YK_HD const DnParams& grid() const { return a.dn; }
    void begin_iteration(uint32_t) {}
    static YK_HD void set_tap(Tap& t, const float* c, const float* ga, const float* gb) {
        DnRule::set_tap(t.t, c, ga, gb);
        t.var = c[3];
    }
    template <class Fetch, class FetchVar>
    YK_HD void pixel(int s, uint32_t x, uint32_t y, const Fetch& fetch, const FetchVar& fetch_var, float* out) const {
        vr_pixel(a, s, x, y, fetch, fetch_var, out);
    }
};

// The colour record of pixel i = (x, y): the film normalised, or the previous iteration's — of which a rule of WIDTH 3
// reads 12 bytes.
template <class Rule, bool IN_RGB>
__device__ __forceinline__ float4 at_color(const DnParams& a, const AtIo& io, size_t i, uint32_t x, uint32_t y) {
    if (!IN_RGB && Rule::WIDTH == 4) return io.in[i];
    if (!IN_RGB) return make_float4(io.in[i].x, io.in[i].y, io.in[i].z, 0.0f);
    float c[3] = {io.film[3 * i], io.film[3 * i + 1], io.film[3 * i + 2]};
    dn_normalise(dn_count(a, io.samples, x, y), c);
    return make_float4(c[0], c[1], c[2], 0.0f);
}

// The film, the records and the output of one launch never overlap (enqueue_atrous sees to it); the guides and the albedo
// are only read.
template <class Rule, bool IN_RGB, int OUT, int S>
__global__ __launch_bounds__(FT_TX* FT_TY) void k_atrous(AtIo io, Rule r, int step) {
    using Tap = typename Rule::Tap;
    const DnParams& a = r.grid();
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    const bool inside = x < a.res_x && y < a.res_y;
    float rec[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (S == 0) {
        if (!inside) return;
        r.pixel(
            step, x, y,
            [&](uint32_t qx, uint32_t qy, Tap& t) {
                const size_t q = (size_t)qy * a.res_x + qx;
                const float4 c = at_color<Rule, IN_RGB>(a, io, q, qx, qy);
                const float4 ga = io.guides[2 * q], gb = io.guides[2 * q + 1];
                Rule::set_tap(t, &c.x, &ga.x, &gb.x);
            },
            [&](uint32_t qx, uint32_t qy) { return reinterpret_cast<const float*>(io.in)[4 * ((size_t)qy * a.res_x + qx) + 3]; }, rec);
    } else {
        using Tile = FilmTile<2 * S>;
        __shared__ float4 lds_c[Tile::N], lds_a[Tile::N], lds_b[Tile::N];
        const Tile tile;
        tile.stage(a.res_x, a.res_y, [&](int k, uint32_t gx, uint32_t gy) {
            const size_t q = (size_t)gy * a.res_x + gx;
            lds_c[k] = at_color<Rule, IN_RGB>(a, io, q, gx, gy);
            lds_a[k] = io.guides[2 * q];
            lds_b[k] = io.guides[2 * q + 1];
        });
        if (!inside) return;
        r.pixel(
            S, x, y,
            [&](uint32_t qx, uint32_t qy, Tap& t) {
                const int k = tile.index(qx, qy);
                const float4 c = lds_c[k], ga = lds_a[k], gb = lds_b[k];
                Rule::set_tap(t, &c.x, &ga.x, &gb.x);
            },
            [&](uint32_t qx, uint32_t qy) { return lds_c[tile.index(qx, qy)].w; }, rec);
    }
    const size_t i = (size_t)y * a.res_x + x;
    if (OUT == OUT_RECORDS) {
        io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
        return;
    }
    if (OUT == OUT_RGB_ALBEDO && io.albedo) {  // a uniform branch on a kernel argument
        const float4 al = io.albedo[i];
        const float alb[3] = {al.x, al.y, al.z};
        al_remodulate(alb, rec);
    }
    io.out_rgb[3 * i] = rec[0];
    io.out_rgb[3 * i + 1] = rec[1];
    io.out_rgb[3 * i + 2] = rec[2];
}

// The preparing pass of the demodulated and the variance-guided denoise: the normalised film, divided by the divisor of
// every pixel's albedo where there is an albedo (al_demodulate), with the sanitised variance where there is a variance,
// as colour records.  Every iteration then reads records.
__global__ __launch_bounds__(256) void k_dn_prepare(AtIo io, DnParams a, const float* __restrict__ variance) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.res_x * a.res_y) return;
    const uint32_t y = i / a.res_x, x = i - y * a.res_x;
    float4 al = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float var = 0.0f;
    if (io.albedo) al = io.albedo[i];  // loaded before the film is waited for: the three loads are in flight together
    if (variance) var = variance[i];
    float4 c = at_color<DnRule, true>(a, io, i, x, y);
    if (io.albedo) {
        const float alb[3] = {al.x, al.y, al.z};
        al_demodulate(alb, &c.x);
    }
    c.w = vr_sanitise(var);
    io.out[i] = c;
}

// The normalised film as colour records (a one-iteration denoise in place) or as RGB (iterations == 0; out_rgb may be the
// film: a lane reads its pixel before it writes it and touches no other).
__global__ __launch_bounds__(256) void k_dn_normalise(AtIo io, DnParams a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.res_x * a.res_y) return;
    const uint32_t y = i / a.res_x, x = i - y * a.res_x;
    const float4 c = at_color<DnRule, true>(a, io, i, x, y);
    if (io.out_rgb) {
        io.out_rgb[3 * (size_t)i] = c.x;
        io.out_rgb[3 * (size_t)i + 1] = c.y;
        io.out_rgb[3 * (size_t)i + 2] = c.z;
    } else {
        io.out[i] = c;
    }
}

template <class Rule, bool IN_RGB, int OUT>
void launch_atrous(hipStream_t st, int variant, const AtIo& io, const Rule& r, int step) {
    const dim3 grid = ft_grid(r.grid().res_x, r.grid().res_y), block = ft_block();
    if (variant == 1) hipLaunchKernelGGL((k_atrous<Rule, IN_RGB, OUT, 1>), grid, block, 0, st, io, r, step);
    else if (variant == 2) hipLaunchKernelGGL((k_atrous<Rule, IN_RGB, OUT, 2>), grid, block, 0, st, io, r, step);
    else hipLaunchKernelGGL((k_atrous<Rule, IN_RGB, OUT, 0>), grid, block, 0, st, io, r, step);
}

// One denoise on `st`: the sample table staged, then n_it iterations of rule r from `film` into `out` (which may be the
// film), through the context's ping-pong buffers.  PREPARED: k_dn_prepare fills ping[0] from the film, `variance` (may be
// NULL) and `albedo` (may be NULL) first, every iteration reads records and the last multiplies the albedo back; else the
// first iteration reads the film itself.  No iteration: the normalised film's bits — no division, no product.
template <class Rule, bool PREPARED>
yk_status enqueue_atrous(yk_context* ctx, hipStream_t st, Rule r, uint32_t n_it, const float* film, const void* guides, const float* variance, const void* albedo,
                         const uint32_t* samples, float* out) {
    const DnParams& a = r.grid();
    const uint32_t n_px = a.res_x * a.res_y;
    const dim3 px_grid((n_px - 1) / 256 + 1), px_block(256);
    auto& dn = ctx->denoise;
    AtIo io{};
    io.film = film;
    io.guides = reinterpret_cast<const float4*>(guides);
    if (yk_status ss = stage_samples(ctx, st, samples, (uint16_t)a.res_x, (uint16_t)a.res_y, (uint16_t)a.tile_dim, dn.samples, &io.samples)) return ss;
    if (n_it == 0) {
        if (samples) {
            io.out_rgb = out;
            hipLaunchKernelGGL(k_dn_normalise, px_grid, px_block, 0, st, io, a);
        } else if (film != out) {
            HIP_TRY(ctx, hipMemcpyAsync(out, film, (size_t)n_px * 12, hipMemcpyDeviceToDevice, st));
        }
        HIP_TRY(ctx, hipGetLastError());
        return YK_OK;
    }
    const bool in_place_single = !PREPARED && n_it == 1 && film == out;  // the one launch would read the film while it writes it
    const bool from_records = PREPARED || in_place_single;
    const uint32_t n_record_passes = n_it - 1 + (from_records ? 1 : 0);  // they alternate between ping[0] and ping[1]
    if (n_record_passes > 0) HIP_TRY(ctx, dn.ping[0].ensure((size_t)n_px * 16));
    if (n_record_passes > 1) HIP_TRY(ctx, dn.ping[1].ensure((size_t)n_px * 16));
    if (from_records) {
        io.out = dn.ping[0].as<float4>();
        if (PREPARED) {
            io.albedo = reinterpret_cast<const float4*>(albedo);
            hipLaunchKernelGGL(k_dn_prepare, px_grid, px_block, 0, st, io, a, variance);
        } else {
            hipLaunchKernelGGL(k_dn_normalise, px_grid, px_block, 0, st, io, a);
        }
    }
    int src = from_records ? 0 : -1;  // which ping-pong buffer holds the previous iteration's colours; -1: the film does
    for (uint32_t i = 0; i < n_it; ++i) {
        const int step = 1 << i;
        const int variant = step <= (int)dn.lds_max_step ? step : 0;
        const bool last = i + 1 == n_it;
        const int dst = src == 0 ? 1 : 0;
        r.begin_iteration(i);
        io.in = src >= 0 ? dn.ping[src].as<const float4>() : nullptr;
        io.out = last ? nullptr : dn.ping[dst].as<float4>();
        io.out_rgb = last ? out : nullptr;
        if (src >= 0) {
            if (last) launch_atrous<Rule, false, PREPARED ? OUT_RGB_ALBEDO : OUT_RGB>(st, variant, io, r, step);
            else launch_atrous<Rule, false, OUT_RECORDS>(st, variant, io, r, step);
        } else if constexpr (!PREPARED) {
            if (last) launch_atrous<Rule, true, OUT_RGB>(st, variant, io, r, step);
            else launch_atrous<Rule, true, OUT_RECORDS>(st, variant, io, r, step);
        }
        src = dst;
    }
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

// The host instance of the same: the film normalised (and demodulated, and beside its variance) as records of
// Rule::WIDTH floats, n_it iterations, the albedo multiplied back.  No iteration: neither division nor product.
template <class Rule>
void atrous_host(Rule r, uint32_t n_it, const float* film, const yk_guide* guides, const float* variance, const yk_albedo* albedo, const uint32_t* samples, float* out) {
    constexpr int W = Rule::WIDTH;
    const DnParams& a = r.grid();
    const size_t n_px = (size_t)a.res_x * a.res_y;
    if (n_it == 0) albedo = nullptr;
    std::vector<float> cur(W * n_px), nxt(n_it ? W * n_px : 0);
    for (uint32_t y = 0; y < a.res_y; ++y)
        for (uint32_t x = 0; x < a.res_x; ++x) {
            const size_t i = (size_t)y * a.res_x + x;
            std::memcpy(&cur[W * i], film + 3 * i, 12);
            dn_normalise(dn_count(a, samples, x, y), &cur[W * i]);
            if (albedo) al_demodulate(albedo[i].a, &cur[W * i]);
            if (W == 4) cur[W * i + 3] = vr_sanitise(variance[i]);
        }
    for (uint32_t it = 0; it < n_it; ++it) {
        r.begin_iteration(it);
        const auto fetch = [&](uint32_t qx, uint32_t qy, typename Rule::Tap& t) {
            const size_t q = (size_t)qy * a.res_x + qx;
            Rule::set_tap(t, &cur[W * q], guides[q].ns, guides[q].p);
        };
        const auto fetch_var = [&](uint32_t qx, uint32_t qy) { return cur[W * ((size_t)qy * a.res_x + qx) + 3]; };  // VrRule's alone
        for (uint32_t y = 0; y < a.res_y; ++y)
            for (uint32_t x = 0; x < a.res_x; ++x) r.pixel(1 << it, x, y, fetch, fetch_var, &nxt[W * ((size_t)y * a.res_x + x)]);
        cur.swap(nxt);
    }
    for (size_t i = 0; i < n_px; ++i) {
        if (albedo) al_remodulate(albedo[i].a, &cur[W * i]);
        std::memcpy(out + 3 * i, &cur[W * i], 12);
    }
}

// What the three denoisers refuse alike.  `variance` and `albedo` are NULL where the entry point does not take them; the
// albedo of yk_denoise_variance may be NULL as well.
yk_status check_call(bool desc_ok, const void* film, const void* guides, bool needs_variance, const void* variance, bool needs_albedo, const void* albedo, uint16_t res_x,
                     uint16_t res_y, uint16_t tile_dim, const void* out) {
    if (!desc_ok || !film || !guides || !out || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    if ((needs_variance && !variance) || (needs_albedo && !albedo)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(guides, n_px * sizeof(yk_guide), out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (variance && overlaps(variance, n_px * 4, out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (out != film && overlaps(film, n_px * 12, out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    if (albedo && overlaps(albedo, n_px * sizeof(yk_albedo), out, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}
bool desc_ok(const yk_denoise_desc* d) { return d && dn_desc_ok(d->iterations, d->sigma_color, d->sigma_normal, d->sigma_plane); }

DnRule make_rule(const yk_denoise_desc* d, uint16_t res_x, uint16_t res_y, uint16_t tile_dim) {
    DnRule r{};
    dn_set_grid(r.a, res_x, res_y, tile_dim);
    r.a.sigma_color = d->sigma_color;
    r.a.den_n = d->sigma_normal * d->sigma_normal;
    r.a.den_p = d->sigma_plane * d->sigma_plane;
    return r;
}

// albedo NULL: the plain denoise; else the demodulated one (yk_albedo.h), which divides before the first iteration and
// multiplies after the last — and does neither when there is no iteration.
yk_status enqueue(yk_context* ctx, hipStream_t st, const yk_denoise_desc* d, const float* film, const void* guides, const void* albedo, uint16_t res_x, uint16_t res_y,
                  uint16_t tile_dim, const uint32_t* samples, float* out) {
    const DnRule r = make_rule(d, res_x, res_y, tile_dim);
    if (albedo) return enqueue_atrous<DnRule, true>(ctx, st, r, d->iterations, film, guides, nullptr, albedo, samples, out);
    return enqueue_atrous<DnRule, false>(ctx, st, r, d->iterations, film, guides, nullptr, nullptr, samples, out);
}

yk_status enqueue_variance_guided(yk_context* ctx, hipStream_t st, const yk_variance_desc* d, const float* film, const void* guides, const float* variance, const void* albedo,
                                  uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out) {
    return enqueue_atrous<VrRule, true>(ctx, st, VrRule{vr_make_params(d, res_x, res_y, tile_dim)}, d->iterations, film, guides, variance, albedo, samples, out);
}

}  // namespace

// yk_denoise (albedo NULL) and yk_denoise_albedo behind one body each; `name` is the entry point's, for its messages.
static yk_status denoise_arrays(yk_context* ctx, const char* name, bool has_albedo, const yk_denoise_desc* desc, const float* film_rgb, const yk_guide* guides, const yk_albedo* albedo,
                                uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb) try {
    if (check_call(desc_ok(desc), film_rgb, guides, false, nullptr, has_albedo, albedo, res_x, res_y, tile_dim, out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (!ctx) {  // the host instance
        atrous_host(make_rule(desc, res_x, res_y, tile_dim), desc->iterations, film_rgb, guides, nullptr, albedo, samples, out_rgb);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const yk_albedo* d_albedo = albedo ? sg.upload(albedo, n_px) : nullptr;
    float* d_out = sg.output(out_rgb, n_px * 3);
    return sg.run([&] { return enqueue(ctx, sg.stream, desc, d_film, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out); });
} YK_CATCH(ctx)

static yk_status denoise_device(yk_context* ctx, const char* name, bool has_albedo, const yk_denoise_desc* desc, const void* d_film_rgb, const void* d_guides, const void* d_albedo,
                                uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(desc_ok(desc), d_film_rgb, d_guides, false, nullptr, has_albedo, d_albedo, res_x, res_y, tile_dim, d_out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    // dword loads and stores of the film and the output, 16-byte loads of the guides and the albedo
    if (misaligned(4, d_film_rgb, d_out_rgb) || misaligned(16, d_guides, d_albedo))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + (has_albedo ? ": film and output must be 4-byte aligned, guides and albedo 16-byte aligned"
                                                                                : ": film and output must be 4-byte aligned, guides 16-byte aligned"));
    return enqueue(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), d_guides, d_albedo, res_x, res_y, tile_dim, samples, reinterpret_cast<float*>(d_out_rgb));
}

extern "C" {

yk_status yk_denoise(yk_context* ctx, const yk_denoise_desc* desc, const float* film_rgb, const yk_guide* guides, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                     const uint32_t* samples, float* out_rgb) {
    return denoise_arrays(ctx, "yk_denoise", false, desc, film_rgb, guides, nullptr, res_x, res_y, tile_dim, samples, out_rgb);
}

yk_status yk_denoise_device(yk_context* ctx, const yk_denoise_desc* desc, const void* d_film_rgb, const void* d_guides, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                            const uint32_t* samples, void* d_out_rgb, void* stream) {
    return denoise_device(ctx, "yk_denoise_device", false, desc, d_film_rgb, d_guides, nullptr, res_x, res_y, tile_dim, samples, d_out_rgb, stream);
}

yk_status yk_denoise_albedo(yk_context* ctx, const yk_denoise_desc* desc, const float* film_rgb, const yk_guide* guides, const yk_albedo* albedo, uint16_t res_x, uint16_t res_y,
                            uint16_t tile_dim, const uint32_t* samples, float* out_rgb) {
    return denoise_arrays(ctx, "yk_denoise_albedo", true, desc, film_rgb, guides, albedo, res_x, res_y, tile_dim, samples, out_rgb);
}

yk_status yk_denoise_albedo_device(yk_context* ctx, const yk_denoise_desc* desc, const void* d_film_rgb, const void* d_guides, const void* d_albedo, uint16_t res_x, uint16_t res_y,
                                   uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream) {
    return denoise_device(ctx, "yk_denoise_albedo_device", true, desc, d_film_rgb, d_guides, d_albedo, res_x, res_y, tile_dim, samples, d_out_rgb, stream);
}

yk_status yk_denoise_variance(yk_context* ctx, const yk_variance_desc* desc, const float* film_rgb, const yk_guide* guides, const float* variance, const yk_albedo* albedo,
                              uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, float* out_rgb) try {
    if (check_call(vr_desc_ok(desc), film_rgb, guides, true, variance, false, albedo, res_x, res_y, tile_dim, out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance: bad argument");
    if (!ctx) {  // the host instance
        atrous_host(VrRule{vr_make_params(desc, res_x, res_y, tile_dim)}, desc->iterations, film_rgb, guides, variance, albedo, samples, out_rgb);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    const float* d_variance = sg.upload(variance, n_px);
    const yk_albedo* d_albedo = albedo ? sg.upload(albedo, n_px) : nullptr;
    float* d_out = sg.output(out_rgb, n_px * 3);
    return sg.run([&] { return enqueue_variance_guided(ctx, sg.stream, desc, d_film, d_guides, d_variance, d_albedo, res_x, res_y, tile_dim, samples, d_out); });
}
YK_CATCH(ctx)

yk_status yk_denoise_variance_device(yk_context* ctx, const yk_variance_desc* desc, const void* d_film_rgb, const void* d_guides, const void* d_variance, const void* d_albedo,
                                     uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_call(vr_desc_ok(desc), d_film_rgb, d_guides, true, d_variance, false, d_albedo, res_x, res_y, tile_dim, d_out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance_device: bad argument");
    // dword loads and stores of the film, the variance and the output, 16-byte loads of the guides and the albedo
    if (misaligned(4, d_film_rgb, d_variance, d_out_rgb) || misaligned(16, d_guides, d_albedo))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_denoise_variance_device: film, variance and output must be 4-byte aligned, guides and albedo 16-byte aligned");
    return enqueue_variance_guided(ctx, device_call_stream(ctx, stream), desc, reinterpret_cast<const float*>(d_film_rgb), d_guides, reinterpret_cast<const float*>(d_variance), d_albedo,
                                   res_x, res_y, tile_dim, samples, reinterpret_cast<float*>(d_out_rgb));
}

}  // extern "C"
