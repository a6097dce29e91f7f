// yk_scene_input.hip — the gfx950 kernels in front of the device builder when a scene's geometry is already in HBM
// (yk_scene_create_device, yk_scene.cpp): the per-triangle checks of check_description, the permutation test of
// shape_order and the shape bounds the builder starts from (yk_scene_input.h).  Streaming kernels, one element a lane,
// 256 lanes a block; consecutive lanes read consecutive 12-byte index triples.  Nothing here addresses memory through
// an index it has not compared with its count: the check kernels read the index arrays only, and the caller reads
// their words back before it launches k_shape_bounds or anything after it.
#include <hip/hip_runtime.h>

#include "yk_internal.h"
#include "yk_scene_input.h"

using namespace yk::inp;

namespace {

const int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_check_geometry(Geometry g, const uint8_t* __restrict__ light_kind, CheckWords* words) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= g.n_triangles) return;
    const uint32_t i = (uint32_t)t;
    const uint32_t failed = tri_check(g, i);
    if (failed != kCheckNone)
        atomicMin(&words->first, 4ull * i + failed);
    else if (!area_light_ok(g, light_kind, i))
        atomicMin(&words->light, 4ull * i);
}

// every entry below n_shapes, none seen twice: one bit a shape
__global__ void __launch_bounds__(kThreads) k_check_shape_order(const uint32_t* __restrict__ order, uint32_t n_shapes, uint32_t* seen, CheckWords* words) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_shapes) return;
    const uint32_t src = order[t];
    bool bad = src >= n_shapes;
    if (!bad) {
        const uint32_t bit = 1u << (src & 31u);
        bad = (atomicOr(&seen[src >> 5], bit) & bit) != 0u;
    }
    if (bad) atomicOr(&words->order_bad, 1u);
}

// one lane per position of the shape order: six floats into the builder's input
__global__ void __launch_bounds__(kThreads) k_shape_bounds(const float* __restrict__ points, const uint32_t* __restrict__ indices, const uint32_t* __restrict__ order, const float* __restrict__ sphere_bounds,
                                                           uint32_t n_triangles, uint32_t n_shapes, float* __restrict__ sb, CheckWords* words) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n_shapes) return;
    const uint32_t src = order ? order[t] : (uint32_t)t;
    if (src >= n_shapes) return;  // cannot happen (the order was checked); guards the gathers
    float b[6];
    if (src < n_triangles) {
        if (!tri_bound(points, indices, src, b)) atomicOr(&words->non_finite, 1u);
    } else {
        const float* s = sphere_bounds + 6 * (size_t)(src - n_triangles);
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = s[k];
    }
    float2* o = reinterpret_cast<float2*>(sb + 6 * t);  // 24 bytes a shape: 8-byte aligned
    o[0] = make_float2(b[0], b[1]);
    o[1] = make_float2(b[2], b[3]);
    o[2] = make_float2(b[4], b[5]);
}

unsigned blocks(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

hipError_t enqueue_geometry_checks(hipStream_t st, const Geometry& g, const uint8_t* d_light_kind, const uint32_t* d_order, uint32_t n_shapes, uint32_t* d_seen, CheckWords* d_words) {
    hipError_t e = hipMemsetAsync(d_words, 0xff, 2 * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(&d_words->order_bad, 0, 4 * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if (g.n_triangles) k_check_geometry<<<blocks(g.n_triangles), kThreads, 0, st>>>(g, d_light_kind, d_words);
    if (d_order) {
        if ((e = hipMemsetAsync(d_seen, 0, ((size_t)n_shapes + 31) / 32 * sizeof(uint32_t), st)) != hipSuccess) return e;
        k_check_shape_order<<<blocks(n_shapes), kThreads, 0, st>>>(d_order, n_shapes, d_seen, d_words);
    }
    return hipGetLastError();
}

hipError_t enqueue_shape_bounds(hipStream_t st, const float* d_points, const uint32_t* d_indices, const uint32_t* d_order, const float* d_sphere_bounds, uint32_t n_triangles, uint32_t n_shapes, float* d_sb, CheckWords* d_words) {
    k_shape_bounds<<<blocks(n_shapes), kThreads, 0, st>>>(d_points, d_indices, d_order, d_sphere_bounds, n_triangles, n_shapes, d_sb, d_words);
    return hipGetLastError();
}
