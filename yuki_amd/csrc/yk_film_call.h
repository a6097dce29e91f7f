// yk_film_call.h — what the call paths of the film passes (tone map, present, overlay, denoise, temporal, motion, albedo,
// variance) share: the words of their argument checks, the scene-ownership refusal, and the two pieces of device work that
// serve more than one file (the record blend, the albedo mean).  Each pass keeps its own refusal rules — which pairs may
// alias, which may be equal, which are optional — and says them with these.  Library-private.
#pragma once
#include "yk_internal.h"

// [p, p + np) and [q, q + nq) share a byte
static inline bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p0 < q0 + nq && q0 < p0 + np;
}

// one of the pointers is not a multiple of `to` bytes (a power of two); NULL, an array the call leaves out, is aligned
template <class... P> static inline bool misaligned(uintptr_t to, const P*... p) { return (((uintptr_t)p | ...) & (to - 1)) != 0; }

// YK_OK when the scene lives on the context's device; else the refusal, recorded on the context.  `name`: the entry point's,
// the message's prefix — "" for the entry points that say it without one.
static inline yk_status scene_on_context(yk_context* ctx, const yk_scene* scene, const char* name) {
    if (scene->on_device && scene->device == ctx->device) return YK_OK;
    return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(name) + (*name ? ": " : "") + "scene was not created on this context's device");
}

// The streaming record blend (k_record_blend, yk_temporal.hip) behind yk_history_blend and yk_moments_blend, which differ in
// the pixel rule alone: tp_blend_pixel makes (rgb, n) records, vr_moments_pixel (m1, m2, frames, n).  `rec`, the carried
// records, may be NULL, and so may one of the outputs; the moments have no RGB output and pass NULL.
enum class BlendRule { HISTORY, MOMENTS };
// the refusals the two share: the descriptor, the sizes, an output at least, and which arrays may overlap (out_rec may BE
// rec and out_rgb the film: a pixel is read before it is written)
yk_status record_blend_check(const yk_temporal_desc* d, const void* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const void* rec, const void* out_rec, const void* out_rgb);
// one launch on `st`, the sample table (host memory, may be NULL) staged before it; nothing checked
yk_status record_blend_enqueue(yk_context* ctx, hipStream_t st, BlendRule rule, const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim,
                               const uint32_t* samples, const void* rec, void* out_rec, float* out_rgb);
// the host instance, on host arrays
void record_blend_host(BlendRule rule, const yk_temporal_desc* d, const float* film, uint16_t res_x, uint16_t res_y, uint16_t tile_dim, const uint32_t* samples, const void* rec, void* out_rec,
                       float* out_rgb);

// k_albedo_mean (yk_albedo.hip) over a res_x x rows film, or band of one, whose ids have s * res_x records to a row: one
// launch on `st`, nothing checked — its callers (yk_albedo_mean_device, the band driver in yk_render.cpp) did.
yk_status albedo_mean_enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* d_ids_ss, uint32_t res_x, uint32_t rows, uint32_t s, void* d_out);

// The stream of a `_device` entry point — the caller's, or the context's own — with the context's device made current.
static inline hipStream_t device_call_stream(yk_context* ctx, void* stream) {
    (void)hipSetDevice(ctx->device);
    return stream ? (hipStream_t)stream : ctx->stream;
}
