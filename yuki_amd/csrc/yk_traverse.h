// yk_traverse.h — the rules every BVH traversal kernel shares (yk_trace.hip, yk_packet.hip): the binary node's layout,
// the ray record and the root test, the primitive test, the occlusion rule and the leaf walks.
#pragma once
#include "yk_device.h"
#include "yk_geom.h"
#include "yk_wave.h"

namespace yk {

// ---- binary node (DevNode, yk_device.h): both children's boxes, their refs and the split axis
struct NodeBoxes {
    V3 lo0, hi0, lo1, hi1;
    unsigned ref0, ref1, axis;
};
// from the node's words q0, q1, q2 and the first half of q3: only 56 of its 64 bytes are fetched
__device__ __forceinline__ NodeBoxes decode_node(float4 a, float4 b, float4 c, uint2 d) {
    NodeBoxes n;
    n.lo0 = V3{a.x, a.y, a.z};
    n.hi0 = V3{a.w, b.x, b.y};
    n.lo1 = V3{b.z, b.w, c.x};
    n.hi1 = V3{c.y, c.z, c.w};
    n.ref0 = d.x;
    n.ref1 = d.y & ~YK_AXIS_MASK;
    n.axis = (d.y >> YK_AXIS_SHIFT) & 3u;
    return n;
}
// Three fetch paths, each through a pointer of its own address space so that the compiler keeps them apart (a generic
// pointer would become flat loads, which also tie the access to vmcnt):
//   global memory: per-lane vector loads
__device__ __forceinline__ NodeBoxes load_node(const DevNode* nodes, unsigned idx) {
    const float4* q = reinterpret_cast<const float4*>(nodes + idx);
    return decode_node(q[0], q[1], q[2], reinterpret_cast<const uint2*>(q)[6]);
}
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 f4(f4v v) { return make_float4(v.x, v.y, v.z, v.w); }
//   a block's LDS copy of the first tree levels (YK_TOP_BIT refs, index `idx` into the copy): ds_read
typedef const __attribute__((address_space(3))) f4v lf4;
typedef const __attribute__((address_space(3))) u2v lu2;
__device__ __forceinline__ NodeBoxes load_node_lds(lf4* top, unsigned idx) {
    lf4* q = top + 4 * idx;
    return decode_node(__builtin_bit_cast(float4, q[0]), __builtin_bit_cast(float4, q[1]), __builtin_bit_cast(float4, q[2]), __builtin_bit_cast(uint2, ((lu2*)q)[6]));
}
//   the constant address space, for a wave-uniform `idx` (wave packets): scene data never changes during a launch, and
//   reading it this way tells the compiler so; a wave-uniform address then becomes a scalar load (s_load_*, served by
//   the scalar cache) instead of 64 identical vector requests.  The packets read their primitives this way too.
typedef const __attribute__((address_space(4))) f4v cf4;
typedef const __attribute__((address_space(4))) u2v cu2;
__device__ __forceinline__ cf4* as_const(const float4* p) { return (cf4*)(unsigned long long)p; }
__device__ __forceinline__ float4 ldc(cf4* p, int i) { return f4(p[i]); }
__device__ __forceinline__ NodeBoxes load_node_uniform(const DevNode* nodes, unsigned idx) {
    cf4* q = as_const(reinterpret_cast<const float4*>(nodes + idx));
    const u2v d = ((cu2*)q)[6];
    return decode_node(ldc(q, 0), ldc(q, 1), ldc(q, 2), make_uint2(d.x, d.y));
}

// ---- the ray as every traversal kernel holds it
struct TraceRay {
    V3 o, inv, d;
    RayTri rt;
    float t_max;
    unsigned negmask;  // bit k: the direction is negative along axis k
};
__device__ __forceinline__ TraceRay ray_setup(V3 o, V3 d, float t_max) {
    TraceRay r;
    r.o = o;
    r.d = d;
    r.inv = V3{1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    r.negmask = (r.inv.x < 0.0f ? 1u : 0u) | (r.inv.y < 0.0f ? 2u : 0u) | (r.inv.z < 0.0f ? 4u : 0u);
    r.rt = ray_tri_setup(d);
    r.t_max = t_max;
    return r;
}
// what a lane of a persistent kernel holds before its first ray
__device__ __forceinline__ TraceRay idle_ray() {
    TraceRay r;
    r.o = r.inv = r.d = V3{0, 0, 0};
    r.rt = RayTri{0, 1, 2, 0, 0, 0};
    r.t_max = 0.0f;
    r.negmask = 0;
    return r;
}
// the root box's test, before the tree is entered
__device__ __forceinline__ bool root_hit(const DevScene& sc, const TraceRay& r) {
    float tmin;
    return slab(V3{sc.root_bmin[0], sc.root_bmin[1], sc.root_bmin[2]}, V3{sc.root_bmax[0], sc.root_bmax[1], sc.root_bmax[2]}, r.o, r.inv, r.t_max, tmin);
}

// ---- primitives: tris[3p .. 3p+2] = (p0, bits(area_light)) (p1, bits(source shape)) (p2, bits(YK_PRIM_*))
// One primitive record against the ray; spheres are looked for only when the scene has some (SPHERES).
template <bool SPHERES>
__device__ __forceinline__ bool prim_hit(const DevScene& sc, const TraceRay& r, float4 v0, float4 v1, float4 v2, TriHit& h) {
    h = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
    if (SPHERES && (__float_as_uint(v2.w) & YK_PRIM_SPHERE)) {
        V3 ro, rd;
        return sphere_hit_t(sc.spheres[__float_as_uint(v1.w) - sc.n_triangles], r.o, r.d, r.t_max, h.t, ro, rd);
    }
    return tri_intersect(r.o, r.rt, r.t_max, f4_xyz(v0), f4_xyz(v1), f4_xyz(v2), h);
}
// bvh.rs:269-280: a hit on the sampled area light's own surface does not occlude (spheres carry no area light: v0.w = -1)
__device__ __forceinline__ bool occludes(float4 v0, int area_light) {
    const int prim_light = (int)__float_as_uint(v0.w);
    return !(area_light >= 0 && prim_light >= 0 && prim_light == area_light);
}

// The closest-hit walk of the leaf that starts at primitive `prim`: primitives in leaf order, a later hit with t == t_max
// replaces the earlier one (triangle.rs:126-127).  Lanes whose `mine` is false only walk along.  UNIFORM: `prim` is
// wave-uniform and the records arrive through scalar loads (wave packets).  on_hit(prim, v1, pflags, hit) records a hit;
// STATS: *tests counts the primitives tested.
template <bool SPHERES, bool UNIFORM, bool STATS, class OnHit>
__device__ __forceinline__ void leaf_closest(const DevScene& sc, unsigned prim, bool mine, TraceRay& r, unsigned* tests, OnHit on_hit) {
    for (;;) {
        float4 v0, v1, v2;
        if (UNIFORM) {
            cf4* tq = as_const(sc.tris + 3 * prim);
            v0 = ldc(tq, 0), v1 = ldc(tq, 1), v2 = ldc(tq, 2);
        } else {
            v0 = sc.tris[3 * prim], v1 = sc.tris[3 * prim + 1], v2 = sc.tris[3 * prim + 2];
        }
        const unsigned pflags = __float_as_uint(v2.w);
        if (mine) {
            TriHit h;
            if (STATS) *tests += 1;
            if (prim_hit<SPHERES>(sc, r, v0, v1, v2, h)) {
                on_hit(prim, v1, pflags, h);
                r.t_max = h.t;
            }
        }
        if (pflags & YK_PRIM_LAST) break;
        ++prim;
    }
}
// The any-hit walk of one lane's leaf: true at the first primitive that occludes.
template <bool SPHERES>
__device__ __forceinline__ bool leaf_any(const DevScene& sc, unsigned prim, const TraceRay& r, int area_light) {
    for (;;) {
        const float4 v0 = sc.tris[3 * prim], v1 = sc.tris[3 * prim + 1], v2 = sc.tris[3 * prim + 2];
        TriHit h;
        if (prim_hit<SPHERES>(sc, r, v0, v1, v2, h) && occludes(v0, area_light)) return true;
        if (__float_as_uint(v2.w) & YK_PRIM_LAST) return false;
        ++prim;
    }
}

// The length of a launch's queue, 0 when the launch was interrupted before it started (CancelRef); block 0 adds it to `counter`.
__device__ __forceinline__ unsigned queue_length(const unsigned* count_ptr, const CancelRef& cancel, unsigned long long* counter) {
    const unsigned n = cancel_raised(cancel) ? 0u : *count_ptr;
    if (counter && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(counter, (unsigned long long)n);
    return n;
}

}  // namespace yk
