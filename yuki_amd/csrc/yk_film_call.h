// yk_film_call.h — what the argument checks of the film passes (tone map, present, overlay, denoise, temporal, motion, albedo)
// share.  Each pass keeps its own refusal rules — which pairs may alias, which may be equal, which are optional — and says
// them with these.  Library-private.
#pragma once
#include "yk_internal.h"

// [p, p + np) and [q, q + nq) share a byte
static inline bool overlaps(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    return p0 < q0 + nq && q0 < p0 + np;
}

// one of the pointers is not a multiple of `to` bytes (a power of two); NULL, an array the call leaves out, is aligned
template <class... P> static inline bool misaligned(uintptr_t to, const P*... p) { return (((uintptr_t)p | ...) & (to - 1)) != 0; }

// k_albedo_mean (yk_albedo.hip) over a res_x x rows film, or band of one, whose ids have s * res_x records to a row: one
// launch on `st`, nothing checked — its callers (yk_albedo_mean_device, the band driver in yk_render.cpp) did.
yk_status albedo_mean_enqueue(yk_context* ctx, hipStream_t st, const yk_scene* scene, const void* d_ids_ss, uint32_t res_x, uint32_t rows, uint32_t s, void* d_out);

// The stream of a `_device` entry point — the caller's, or the context's own — with the context's device made current.
static inline hipStream_t device_call_stream(yk_context* ctx, void* stream) {
    (void)hipSetDevice(ctx->device);
    return stream ? (hipStream_t)stream : ctx->stream;
}
