// yk_scene_route.h — what the host code of yk_scene_update.hip and yk_scene_edit.hip shares (their steps: yk_internal.h).
#pragma once
#include "yk_internal.h"

// a HIP call of a step that fails ends the step with its YK_LAYOUT_REASON_*, once stream `st` has run dry
#define ROUTE_TRY(st, expr)                 \
    do {                                    \
        const hipError_t e_ = (expr);       \
        if (e_ != hipSuccess) {             \
            (void)hipStreamSynchronize(st); \
            return layout_reason_of(e_);    \
        }                                   \
    } while (0)
static inline unsigned route_blocks(size_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }
