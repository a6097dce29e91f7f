// yk_temporal.hip — reproject and blend on gfx950, behind yk_history_reproject[_device] and yk_history_blend[_device]; the
// per-pixel arithmetic is yk_temporal.h's, whose host instance these entry points run without a context.
//
// k_reproject: one lane per pixel, a block is a 32 x 8 tile of the film (yk_film_tile.h: a wave covers two rows of 32
//   pixels, so under small motion neighbouring lanes project to neighbouring taps).  A lane reads its guide (two
//   16-byte loads), up to four taps of the previous view (two 16-byte guide loads and one 16-byte history load each, all
//   issued before the first is consumed; a tap outside the film is never read, its request goes to the nearest pixel inside) and writes one 16-byte record.  The previous
//   camera's two inverse matrices travel as kernel arguments: scalar registers.  No LDS: the footprint of a tile is not
//   known before the projection.
// k_record_blend: streaming, one lane per pixel: three dword loads of the film (4-byte alignment), one 16-byte load and one
//   16-byte store of the records, three dword stores of the RGB output.  The pixel rule is a template parameter:
//   tp_blend_pixel for yk_history_blend, vr_moments_pixel (yk_variance.h) for yk_moments_blend, whose entry points in
//   yk_variance.hip reach the kernel through record_blend_enqueue (yk_film_call.h).  "No table", "no records", "no record
//   output" and "no RGB output" are template variants: no lane tests a pointer.  Twelve instances of the history rule can be
//   launched (one output at least) and four of the moments rule (records out, never RGB).  A lane reads its own pixel only,
//   and before it writes it, so out_rec may be the records and out_rgb the film.
// k_reproject<true> (yk_history_reproject_moved): the same lane with the pixel's motion record (one 16-byte load, requested
//   with the guide loads) in the place of the guide's (p, t) half, which this instance does not read.  The motion pointer
//   is the kernel's last argument: k_reproject<false> is the kernel as it was.
// The sample table of either blend is staged into ctx->temporal.samples through the pinned copy the tone map and the
// denoiser share; the stream-ordered entry points allocate nothing once the context has seen a table of that size.
#include <hip/hip_runtime.h>

#include <cstring>

#include "yk_film_call.h"
#include "yk_film_tile.h"
#include "yk_staging.h"
#include "yk_variance.h"

namespace {

struct TpIo {
    const float4* prev_history;  // one float4 a pixel: (rgb, n)
    const float4* prev_guides;   // two float4 a pixel: (ns, hit), (p, t)
    const float4* guides;
    float4* out;
};

template <bool MOVED>
__global__ __launch_bounds__(FT_TX* FT_TY) void k_reproject(TpIo io, TpParams a, M44 c2w_inv, M44 r2c_inv, const float4* motion) {
    const uint32_t x = blockIdx.x * FT_TX + threadIdx.x, y = blockIdx.y * FT_TY + threadIdx.y;
    if (x >= a.dn.res_x || y >= a.dn.res_y) return;
    const size_t i = (size_t)y * a.dn.res_x + x;
    const float4 ga = io.guides[2 * i], gb = MOVED ? motion[i] : io.guides[2 * i + 1];  // MOVED: (p_prev, known) for (p, t)
    float rec[4];
    tp_reproject_pixel(a, c2w_inv.m, r2c_inv.m, V3{ga.x, ga.y, ga.z}, MOVED && gb.w == 0.0f ? 0.0f : ga.w, V3{gb.x, gb.y, gb.z},
                       [&](uint32_t qx, uint32_t qy, TpTap& t) {
                           const size_t q = (size_t)qy * a.dn.res_x + qx;
                           const float4 hv = io.prev_history[q], qa = io.prev_guides[2 * q], qb = io.prev_guides[2 * q + 1];
                           t.c[0] = hv.x;
                           t.c[1] = hv.y;
                           t.c[2] = hv.z;
                           t.n = hv.w;
                           t.ns[0] = qa.x;
                           t.ns[1] = qa.y;
                           t.ns[2] = qa.z;
                           t.hit = qa.w;
                           t.p[0] = qb.x;
                           t.p[1] = qb.y;
                           t.p[2] = qb.z;
                       },
                       rec);
    io.out[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
}

// The pixel rules of the record blend as stateless types: the kernel and the host loop are instantiated on one.
struct HistoryRule {  // yk_history_blend: (rgb, n) records, shown as RGB
    static constexpr bool RGB_OUTPUT = true;
    YK_HD void operator()(const TpParams& a, bool has_table, float m, const float* c, const float* h, float* out) const { tp_blend_pixel(a, has_table, m, c, h, out); }
};
struct MomentsRule {  // yk_moments_blend: (m1, m2, frames, n) records, never shown
    static constexpr bool RGB_OUTPUT = false;
    YK_HD void operator()(const TpParams& a, bool has_table, float m, const float* c, const float* h, float* out) const { vr_moments_pixel(a, has_table, m, c, h, out); }
};

struct BlendIo {
    const float* film;
    const uint32_t* samples;
    const float4* rec;
    float4* out_rec;
    float* out_rgb;
};

template <class Rule, bool TABLE, bool HIST, bool OUT_REC, bool OUT_RGB>
__global__ __launch_bounds__(256) void k_record_blend(BlendIo io, TpParams a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.dn.res_x * a.dn.res_y) return;
    const float c[3] = {io.film[3 * (size_t)i], io.film[3 * (size_t)i + 1], io.film[3 * (size_t)i + 2]};
    float m = 1.0f;
    if (TABLE) {
        const uint32_t y = i / a.dn.res_x, x = i - y * a.dn.res_x;
        m = dn_count(a.dn, io.samples, x, y);
    }
    float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HIST) {
        const float4 v = io.rec[i];
        h[0] = v.x;
        h[1] = v.y;
        h[2] = v.z;
        h[3] = v.w;
    }
    float rec[4];
    Rule()(a, TABLE, m, c, HIST ? h : nullptr, rec);
    if (OUT_REC) io.out_rec[i] = make_float4(rec[0], rec[1], rec[2], rec[3]);
    if (OUT_RGB) {
        io.out_rgb[3 * (size_t)i] = rec[0];
        io.out_rgb[3 * (size_t)i + 1] = rec[1];
        io.out_rgb[3 * (size_t)i + 2] = rec[2];
    }
}

// The outputs: one at least (record_blend_check).  A rule without an RGB output has the records-only instance alone.
template <class Rule, bool TABLE, bool HIST>
void launch_blend2(hipStream_t st, uint32_t n_px, const BlendIo& io, const TpParams& a) {
    const dim3 grid((n_px - 1) / 256 + 1), block(256);
    if constexpr (Rule::RGB_OUTPUT) {
        if (io.out_rgb) {
            if (io.out_rec) hipLaunchKernelGGL((k_record_blend<Rule, TABLE, HIST, true, true>), grid, block, 0, st, io, a);
            else hipLaunchKernelGGL((k_record_blend<Rule, TABLE, HIST, false, true>), grid, block, 0, st, io, a);
            return;
        }
    }
    hipLaunchKernelGGL((k_record_blend<Rule, TABLE, HIST, true, false>), grid, block, 0, st, io, a);
}
template <class Rule>
void launch_blend(hipStream_t st, uint32_t n_px, const BlendIo& io, const TpParams& a) {
    if (io.samples && io.rec) launch_blend2<Rule, true, true>(st, n_px, io, a);
    else if (io.samples) launch_blend2<Rule, true, false>(st, n_px, io, a);
    else if (io.rec) launch_blend2<Rule, false, true>(st, n_px, io, a);
    else launch_blend2<Rule, false, false>(st, n_px, io, a);
}

template <class Rule>
void blend_host(const TpParams& a, const float* film, const uint32_t* samples, const float* rec, float* out_rec, float* out_rgb) {
    for (uint32_t y = 0; y < a.dn.res_y; ++y)
        for (uint32_t x = 0; x < a.dn.res_x; ++x) {
            const size_t i = (size_t)y * a.dn.res_x + x;
            float c[3], h[4], r[4];
            std::memcpy(c, film + 3 * i, 12);
            if (rec) std::memcpy(h, rec + 4 * i, 16);
            Rule()(a, samples != nullptr, samples ? dn_count(a.dn, samples, x, y) : 1.0f, c, rec ? h : nullptr, r);
            if (out_rec) std::memcpy(out_rec + 4 * i, r, 16);
            if (out_rgb) std::memcpy(out_rgb + 3 * i, r, 12);
        }
}

// has_motion: the call is yk_history_reproject_moved's and `motion` is one more input
yk_status check_reproject(const yk_temporal_desc* d, const void* prev_history, const void* prev_guides, const yk_camera* prev_camera, const void* guides, uint16_t res_x, uint16_t res_y,
                          const void* out, bool has_motion = false, const void* motion = nullptr) {
    if (!tp_desc_ok(d) || !prev_history || !prev_guides || !prev_camera || !guides || !out || res_x == 0 || res_y == 0 || (has_motion && !motion)) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (overlaps(out, n_px * 16, prev_history, n_px * 16) || overlaps(out, n_px * 16, prev_guides, n_px * sizeof(yk_guide)) || overlaps(out, n_px * 16, guides, n_px * sizeof(yk_guide)))
        return YK_ERR_INVALID_ARGUMENT;
    if (has_motion && overlaps(out, n_px * 16, motion, n_px * sizeof(yk_motion))) return YK_ERR_INVALID_ARGUMENT;
    return YK_OK;
}

yk_status enqueue_reproject(yk_context* ctx, hipStream_t st, const yk_temporal_desc* d, const void* prev_history, const void* prev_guides, const yk_camera* cam, const void* guides,
                            uint16_t res_x, uint16_t res_y, void* out, const void* motion = nullptr) {
    const TpParams a = tp_make_params(d, res_x, res_y, 1);
    TpIo io{reinterpret_cast<const float4*>(prev_history), reinterpret_cast<const float4*>(prev_guides), reinterpret_cast<const float4*>(guides), reinterpret_cast<float4*>(out)};
    M44 c2w_inv, r2c_inv;
    std::memcpy(c2w_inv.m, cam->camera_to_world_inv, 64);
    std::memcpy(r2c_inv.m, cam->raster_to_camera_inv, 64);
    if (motion) hipLaunchKernelGGL(k_reproject<true>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, c2w_inv, r2c_inv, reinterpret_cast<const float4*>(motion));
    else hipLaunchKernelGGL(k_reproject<false>, ft_grid(res_x, res_y), ft_block(), 0, st, io, a, c2w_inv, r2c_inv, (const float4*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void fetch_host(const float* hist, const yk_guide* g, size_t q, TpTap& t) {
    std::memcpy(t.c, hist + 4 * q, 12);
    t.n = hist[4 * q + 3];
    std::memcpy(t.ns, g[q].ns, 12);
    t.hit = g[q].hit;
    std::memcpy(t.p, g[q].p, 12);
}

void reproject_host(const yk_temporal_desc* d, const yk_history* prev_history, const yk_guide* prev_guides, const yk_camera* cam, const yk_guide* guides, uint16_t res_x, uint16_t res_y,
                    yk_history* out, const yk_motion* motion = nullptr) {
    const TpParams a = tp_make_params(d, res_x, res_y, 1);
    const float* hist = reinterpret_cast<const float*>(prev_history);
    const auto fetch = [&](uint32_t qx, uint32_t qy, TpTap& t) { fetch_host(hist, prev_guides, (size_t)qy * res_x + qx, t); };
    for (uint32_t y = 0; y < res_y; ++y)
        for (uint32_t x = 0; x < res_x; ++x) {
            const size_t i = (size_t)y * res_x + x;
            const yk_guide& g = guides[i];
            float rec[4];
            if (motion) {
                const float mv[4] = {motion[i].p_prev[0], motion[i].p_prev[1], motion[i].p_prev[2], motion[i].known};
                tp_reproject_moved_pixel(a, cam->camera_to_world_inv, cam->raster_to_camera_inv, V3{g.ns[0], g.ns[1], g.ns[2]}, g.hit, mv, fetch, rec);
            } else
                tp_reproject_pixel(a, cam->camera_to_world_inv, cam->raster_to_camera_inv, V3{g.ns[0], g.ns[1], g.ns[2]}, g.hit, V3{g.p[0], g.p[1], g.p[2]}, fetch, rec);
            std::memcpy(&out[i], rec, 16);
        }
}

}  // namespace

// ------------------------------------------------------------------ the record blend (yk_film_call.h)
yk_status record_blend_check(const yk_temporal_desc* d, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* rec, const void* out_rec, const void* out_rgb) {
    if (!tp_desc_ok(d) || !film || res_x == 0 || res_y == 0 || tile_dim == 0) return YK_ERR_INVALID_ARGUMENT;
    if (!out_rec && !out_rgb) return YK_ERR_INVALID_ARGUMENT;
    const size_t n_px = (size_t)res_x * res_y;
    if (out_rec) {
        if (overlaps(out_rec, n_px * 16, film, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
        if (rec && out_rec != rec && overlaps(out_rec, n_px * 16, rec, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
        if (out_rgb && overlaps(out_rec, n_px * 16, out_rgb, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
    }
    if (out_rgb) {
        if (out_rgb != film && overlaps(out_rgb, n_px * 12, film, n_px * 12)) return YK_ERR_INVALID_ARGUMENT;
        if (rec && overlaps(out_rgb, n_px * 12, rec, n_px * 16)) return YK_ERR_INVALID_ARGUMENT;
    }
    return YK_OK;
}

yk_status record_blend_enqueue(yk_context* ctx, hipStream_t st, BlendRule rule, const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                               const uint32_t* samples, const void* rec, void* out_rec, float* out_rgb) {
    const TpParams a = tp_make_params(d, res_x, res_y, tile_dim);
    BlendIo io{film, nullptr, reinterpret_cast<const float4*>(rec), reinterpret_cast<float4*>(out_rec), out_rgb};
    if (yk_status ss = stage_samples(ctx, st, samples, res_x, res_y, tile_dim, ctx->temporal.samples, &io.samples)) return ss;
    if (rule == BlendRule::MOMENTS) launch_blend<MomentsRule>(st, (uint32_t)res_x * res_y, io, a);
    else launch_blend<HistoryRule>(st, (uint32_t)res_x * res_y, io, a);
    HIP_TRY(ctx, hipGetLastError());
    return YK_OK;
}

void record_blend_host(BlendRule rule, const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const void* rec, void* out_rec,
                       float* out_rgb) {
    const TpParams a = tp_make_params(d, res_x, res_y, tile_dim);
    if (rule == BlendRule::MOMENTS) blend_host<MomentsRule>(a, film, samples, static_cast<const float*>(rec), static_cast<float*>(out_rec), out_rgb);
    else blend_host<HistoryRule>(a, film, samples, static_cast<const float*>(rec), static_cast<float*>(out_rec), out_rgb);
}

// yk_history_reproject (has_motion false, motion NULL) and yk_history_reproject_moved behind one body each; `name` is the
// entry point's, for its messages.
static yk_status reproject_arrays(yk_context* ctx, const char* name, bool has_motion, const yk_temporal_desc* desc, const yk_history* prev_history, const yk_guide* prev_guides,
                                  const yk_camera* prev_camera, const yk_guide* guides, const yk_motion* motion, uint16_t res_x, uint16_t res_y, yk_history* out_history) {
    if (check_reproject(desc, prev_history, prev_guides, prev_camera, guides, res_x, res_y, out_history, has_motion, motion) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    if (!ctx) {  // the host instance
        reproject_host(desc, prev_history, prev_guides, prev_camera, guides, res_x, res_y, out_history, motion);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const yk_motion* d_motion = motion ? sg.upload(motion, n_px) : nullptr;
    const yk_history* d_prev_history = sg.upload(prev_history, n_px);
    const yk_guide* d_prev_guides = sg.upload(prev_guides, n_px);
    const yk_guide* d_guides = sg.upload(guides, n_px);
    yk_history* d_out = sg.output(out_history, n_px);
    return sg.run([&] { return enqueue_reproject(ctx, sg.stream, desc, d_prev_history, d_prev_guides, prev_camera, d_guides, res_x, res_y, d_out, d_motion); });
}

static yk_status reproject_device(yk_context* ctx, const char* name, bool has_motion, const yk_temporal_desc* desc, const void* d_prev_history, const void* d_prev_guides,
                                  const yk_camera* prev_camera, const void* d_guides, const void* d_motion, uint16_t res_x, uint16_t res_y, void* d_out_history, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (check_reproject(desc, d_prev_history, d_prev_guides, prev_camera, d_guides, res_x, res_y, d_out_history, has_motion, d_motion) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + ": bad argument");
    // 16-byte loads and stores of the records, the guides and the motion
    if (misaligned(16, d_prev_history, d_prev_guides, d_guides, d_motion, d_out_history))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + (has_motion ? ": histories, guides and motion must be 16-byte aligned" : ": histories and guides must be 16-byte aligned"));
    return enqueue_reproject(ctx, device_call_stream(ctx, stream), desc, d_prev_history, d_prev_guides, prev_camera, d_guides, res_x, res_y, d_out_history, d_motion);
}

extern "C" {

yk_status yk_history_reproject(yk_context* ctx, const yk_temporal_desc* desc, const yk_history* prev_history, const yk_guide* prev_guides, const yk_camera* prev_camera,
                               const yk_guide* guides, uint16_t res_x, uint16_t res_y, yk_history* out_history) {
    return reproject_arrays(ctx, "yk_history_reproject", false, desc, prev_history, prev_guides, prev_camera, guides, nullptr, res_x, res_y, out_history);
}

yk_status yk_history_reproject_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_prev_history, const void* d_prev_guides, const yk_camera* prev_camera,
                                      const void* d_guides, uint16_t res_x, uint16_t res_y, void* d_out_history, void* stream) {
    return reproject_device(ctx, "yk_history_reproject_device", false, desc, d_prev_history, d_prev_guides, prev_camera, d_guides, nullptr, res_x, res_y, d_out_history, stream);
}

yk_status yk_history_reproject_moved(yk_context* ctx, const yk_temporal_desc* desc, const yk_history* prev_history, const yk_guide* prev_guides, const yk_camera* prev_camera,
                                     const yk_guide* guides, const yk_motion* motion, uint16_t res_x, uint16_t res_y, yk_history* out_history) {
    return reproject_arrays(ctx, "yk_history_reproject_moved", true, desc, prev_history, prev_guides, prev_camera, guides, motion, res_x, res_y, out_history);
}

yk_status yk_history_reproject_moved_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_prev_history, const void* d_prev_guides, const yk_camera* prev_camera,
                                            const void* d_guides, const void* d_motion, uint16_t res_x, uint16_t res_y, void* d_out_history, void* stream) {
    return reproject_device(ctx, "yk_history_reproject_moved_device", true, desc, d_prev_history, d_prev_guides, prev_camera, d_guides, d_motion, res_x, res_y, d_out_history, stream);
}

yk_status yk_history_blend(yk_context* ctx, const yk_temporal_desc* desc, const float* film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                           const yk_history* history, yk_history* out_history, float* out_rgb) {
    if (record_blend_check(desc, film_rgb, res_x, res_y, tile_dim, history, out_history, out_rgb) != YK_OK) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_blend: bad argument");
    if (!ctx) {  // the host instance
        record_blend_host(BlendRule::HISTORY, desc, film_rgb, res_x, res_y, tile_dim, samples, history, out_history, out_rgb);
        return YK_OK;
    }
    YK_LOCK(ctx);
    Staging sg(ctx);
    const size_t n_px = (size_t)res_x * res_y;
    const float* d_film = sg.upload(film_rgb, n_px * 3);
    const yk_history* d_history = history ? sg.upload(history, n_px) : nullptr;
    yk_history* d_out_history = sg.output(out_history, n_px);  // an output the caller left out takes no slot and stays NULL
    float* d_out_rgb = sg.output(out_rgb, n_px * 3);
    return sg.run([&] { return record_blend_enqueue(ctx, sg.stream, BlendRule::HISTORY, desc, d_film, res_x, res_y, tile_dim, samples, d_history, d_out_history, d_out_rgb); });
}

yk_status yk_history_blend_device(yk_context* ctx, const yk_temporal_desc* desc, const void* d_film_rgb, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples,
                                  const void* d_history, void* d_out_history, void* d_out_rgb, void* stream) {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (record_blend_check(desc, d_film_rgb, res_x, res_y, tile_dim, d_history, d_out_history, d_out_rgb) != YK_OK)
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_blend_device: bad argument");
    // dword loads and stores of the film and the RGB output, 16-byte loads and stores of the records
    if (misaligned(4, d_film_rgb, d_out_rgb) || misaligned(16, d_history, d_out_history))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "yk_history_blend_device: film and RGB output must be 4-byte aligned, histories 16-byte aligned");
    return record_blend_enqueue(ctx, device_call_stream(ctx, stream), BlendRule::HISTORY, desc, reinterpret_cast<const float*>(d_film_rgb), res_x, res_y, tile_dim, samples, d_history, d_out_history,
                                reinterpret_cast<float*>(d_out_rgb));
}

}  // extern "C"
