// yk_trace.hip — BVH traversal kernels for gfx950.
//
//   k_trace_closest_pt / k_trace_any_pt   production kernels: persistent waves,
//       per-lane ray replacement with software prefetch, wave-uniform choice
//       between an interior-node step and a leaf step (LDS-staged stacks)
//   k_trace_closest<STATS>  plain one-ray-per-lane loop; the STATS flavour reproduces
//       IntersectionResult's counters (bvh.rs:167-179) for the BVHIntersections
//       integrator and the parity tests
//   k_whitted / k_path_debug  one lane per sample: Whitted's recursion, Path::li_debug
//
// All of them implement BoundingVolumeHierarchy::intersect (bvh.rs:160-232) and
// ::any_intersect (bvh.rs:235-302) with the reference's visiting order, through the
// node steps below and the rules of yk_traverse.h.
#include <hip/hip_runtime.h>

#include "yk_device.h"
#include "yk_geom.h"
#include "yk_kernels.h"
#include "yk_shade.h"
#include "yk_traverse.h"
#include "yk_wave.h"

// build-time tuning knobs of the persistent traversal kernels
#ifndef TRACE_BLOCK
#define TRACE_BLOCK 256
#endif
#ifndef TRACE_LDS
#define TRACE_LDS 8  // stack entries per lane kept in LDS
#endif
#ifndef TRACE_TOP
#define TRACE_TOP 95  // interior nodes of the first tree levels kept in LDS (<= YK_TOP_MAX)
#endif
#ifndef TRACE_ANY_TOP
#define TRACE_ANY_TOP 224  // any-hit kernel: its stack entries are 4 bytes (a ref, no entry distance), which leaves LDS for this many top nodes
#endif
#ifndef TRACE_ANY_LDS
#define TRACE_ANY_LDS TRACE_LDS  // any-hit kernel: stack entries per lane kept in LDS (>= TRACE_LDS: both kernels share the spill buffer's depth)
#endif
#ifndef TRACE_MIN_WAVES
#define TRACE_MIN_WAVES 7  // waves per SIMD the register allocator must leave room for
#endif

namespace yk {

// Sensitivity experiments are compiled in only by tools/build_variant.sh (-DYK_TRACE_EXPERIMENTS pulls in
// tools/micro/trace_experiments.h); the product build sees an empty hook.
#ifdef YK_TRACE_EXPERIMENTS
#include "../../tools/micro/trace_experiments.h"
#else
#define YK_EXPERIMENT_NODE(p, nb)
#endif

// ------------------------------------------------------------------ traversal
// Traversal stack: entries [0, LDS_DEPTH) live in LDS laid out [depth][thread]
// (conflict-free: the bank depends on the lane only), deeper entries overflow to
// a per-thread slice of HBM scratch.  Capacity 64 like the reference (bvh.rs:172).
#define YK_REF_STACK_CAP 64  // the reference's to_visit_stack (bvh.rs:172-174): binary traversal
#define YK_STACK_CAP 96      // storage: 64 binary entries can become 96 in the 4-wide traversal

// Entry E: unsigned long long = ref | entry distance bits << 32 (closest hit); unsigned = the bare ref (any hit,
// which never re-tests a deferred box: half the LDS).  The spill buffer is sized for 8-byte entries; 4-byte ones use
// it as words with the same stride.  LDS words are addressed through an address_space(3) pointer so the compiler
// emits ds_read / ds_write (a generic pointer in a struct degrades to flat_load/flat_store, which also ties the
// access to vmcnt).
template <int BLOCK, int LDS_DEPTH, class E> struct TravStack {
    typedef __attribute__((address_space(3))) E lds_e;
    typedef __attribute__((address_space(1))) E glb_e;
    lds_e* lds;    // [LDS_DEPTH][BLOCK]
    glb_e* spill;  // [YK_STACK_CAP - LDS_DEPTH][spill_stride]
    unsigned spill_stride, gtid;
    __device__ __forceinline__ void push(int sp, unsigned ref, float tmin) {
        const E e = sizeof(E) == 8 ? (E)((unsigned long long)ref | ((unsigned long long)__float_as_uint(tmin) << 32)) : (E)ref;
        if (sp < LDS_DEPTH)
            lds[sp * BLOCK + threadIdx.x] = e;
        else
            spill[(size_t)(sp - LDS_DEPTH) * spill_stride + gtid] = e;
    }
    __device__ __forceinline__ E at(int sp) const {
        return sp < LDS_DEPTH ? lds[sp * BLOCK + threadIdx.x] : spill[(size_t)(sp - LDS_DEPTH) * spill_stride + gtid];
    }
};
// `lds`: the kernel's __shared__ E[LDS_DEPTH * BLOCK]
template <int BLOCK, int LDS_DEPTH, class E>
__device__ __forceinline__ TravStack<BLOCK, LDS_DEPTH, E> make_stack(E* lds, uint2* spill, unsigned spill_stride) {
    typedef TravStack<BLOCK, LDS_DEPTH, E> S;
    S s;
    s.lds = (typename S::lds_e*)lds;
    s.spill = (typename S::glb_e*)spill;
    s.spill_stride = spill_stride;
    s.gtid = blockIdx.x * BLOCK + threadIdx.x;
    return s;
}
// A push onto a full stack flags the overflow (the host reports YK_ERR_STACK_OVERFLOW), empties the stack and returns false.
template <int CAP, class Stack>
__device__ __forceinline__ bool push_capped(Stack& stk, int& sp, unsigned ref, float tmin, unsigned* err) {
    if (sp >= CAP) {
        atomicOr(err, 1u);
        sp = 0;
        return false;
    }
    stk.push(sp, ref, tmin);
    ++sp;
    return true;
}
// IntersectionResult's counters (bvh.rs:167-179); the traversal functions take a null pointer when nothing is counted
struct TraceStats {
    unsigned node_tests, node_hits, shape_tests;
};
// Closest hit: pops until an entry whose entry distance still satisfies tmin <= t_max (the reference's test at pop time).
template <bool STATS, class Stack>
__device__ __forceinline__ bool pop_closest(Stack& stk, int& sp, float t_max, unsigned& cur, TraceStats* stats) {
    while (sp > 0) {
        --sp;
        const unsigned long long e = stk.at(sp);
        if (STATS) stats->node_tests += 1;
        if (__uint_as_float((unsigned)(e >> 32)) <= t_max) {
            if (STATS) stats->node_hits += 1;
            cur = (unsigned)e;
            return true;
        }
    }
    return false;
}
template <class Stack> __device__ __forceinline__ bool pop_any(Stack& stk, int& sp, unsigned& cur) {
    if (sp == 0) return false;
    --sp;
    cur = (unsigned)stk.at(sp);
    return true;
}

// the first tree levels live in LDS (YK_TOP_BIT refs): a block copies them once
template <int BLOCK> __device__ __forceinline__ void fill_top(float4* lds_top, const DevNode* top_nodes, unsigned n_top) {
    const float4* src = reinterpret_cast<const float4*>(top_nodes);
    for (unsigned i = threadIdx.x; i < n_top * 4u; i += BLOCK) lds_top[i] = src[i];
    __syncthreads();
}
__device__ __forceinline__ NodeBoxes load_node(const float4* lds_top, const DevNode* nodes, unsigned ref) {
    return (ref & YK_TOP_BIT) ? load_node_lds((lf4*)lds_top, ref & ~YK_TOP_BIT) : load_node(nodes, ref);
}

// ---- 2-wide node steps
// What a step leaves: STEP_ENTER, `cur` is the child entered now; STEP_POP, the ray goes on with a pop; STEP_OVERFLOW,
// a push overflowed (flagged, the stack emptied; `cur` is the near child when it was entered).  The persistent kernels
// go on with the near child, the one-lane loops end the ray.
enum StepEnd { STEP_POP, STEP_ENTER, STEP_OVERFLOW };
// Closest hit with the reference's visiting order (near child first by the sign of the direction along the split
// axis, far child deferred).  The box of a deferred child is evaluated when its parent is visited — against a
// slightly relaxed bound, because a tie hit can raise t_max by a few ulps (deferred_t_max, yk_geom.h) — and completed
// at pop time by the exact `tmin <= t_max`, which is the reference's test at pop time (DESIGN.md §traversal
// equivalence).  A child entered right away gets the exact bound.  STATS counts the near child's test and pushes the
// far child even when its box is missed, so that its test is counted when it is popped, as the reference does.
template <bool STATS, class Stack>
__device__ __forceinline__ StepEnd node2_closest(const NodeBoxes& nb, const TraceRay& r, Stack& stk, int& sp, unsigned& cur, unsigned* err, TraceStats* stats) {
    float t0, t1;
    const float t_def = deferred_t_max(r.t_max);
    const bool h0 = slab(nb.lo0, nb.hi0, r.o, r.inv, t_def, t0);
    const bool h1 = slab(nb.lo1, nb.hi1, r.o, r.inv, t_def, t1);
    const bool swap = (r.negmask >> nb.axis) & 1u;
    const unsigned near_ref = swap ? nb.ref1 : nb.ref0, far_ref = swap ? nb.ref0 : nb.ref1;
    const bool near_hit = (swap ? h1 : h0) && (swap ? t1 : t0) <= r.t_max, far_hit = swap ? h0 : h1;
    const float far_t = swap ? t0 : t1;
    bool pushed = true;
    if (STATS) {
        stats->node_tests += 1;
        if (near_hit) stats->node_hits += 1;
        pushed = push_capped<YK_REF_STACK_CAP>(stk, sp, far_ref, far_hit ? far_t : __builtin_nanf(""), err);
    }
    if (near_hit) {
        if (!STATS && far_hit) pushed = push_capped<YK_REF_STACK_CAP>(stk, sp, far_ref, far_t, err);
        cur = near_ref;
        return pushed ? STEP_ENTER : STEP_OVERFLOW;
    }
    if (!pushed) return STEP_OVERFLOW;
    if (!STATS && far_hit && far_t <= r.t_max) {
        cur = far_ref;
        return STEP_ENTER;
    }
    return STEP_POP;
}
// Any hit: the verdict does not depend on the visiting order; near-first finds occluders sooner.
template <class Stack>
__device__ __forceinline__ StepEnd node2_any(const NodeBoxes& nb, const TraceRay& r, Stack& stk, int& sp, unsigned& cur, unsigned* err) {
    float t0, t1;
    const bool h0 = slab(nb.lo0, nb.hi0, r.o, r.inv, r.t_max, t0);
    const bool h1 = slab(nb.lo1, nb.hi1, r.o, r.inv, r.t_max, t1);
    const bool swap = (r.negmask >> nb.axis) & 1u;
    const unsigned near_ref = swap ? nb.ref1 : nb.ref0, far_ref = swap ? nb.ref0 : nb.ref1;
    const bool near_hit = swap ? h1 : h0, far_hit = swap ? h0 : h1;
    if (near_hit) {
        const bool pushed = !far_hit || push_capped<YK_REF_STACK_CAP>(stk, sp, far_ref, 0.0f, err);
        cur = near_ref;
        return pushed ? STEP_ENTER : STEP_OVERFLOW;
    }
    if (far_hit) {
        cur = far_ref;
        return STEP_ENTER;
    }
    return STEP_POP;
}

// ---- 4-wide node step ------------------------------------------------------------
// Tests the four grandchild boxes of a collapsed node and returns them in the reference's
// visiting order for this ray (slot k of the result is visited before slot k+1); a missed
// or absent slot has ref == YK_REF_NONE.
//
// Equivalence with the binary traversal (traversal equivalence): the reference
// would first test the intermediate child box A (or B) and only then its children.  For
// the slab test of bounds.rs:176-193 a box that contains another yields, axis by axis, an
// interval that contains the other's ((p - o) * inv is monotone in p, min/max keep order and
// drop the same NaNs), so hit(grandchild) implies hit(child) with any t_max: skipping the
// intermediate test visits exactly the same leaves.  Deferred slots keep their entry
// distance and are re-checked against the current t_max when popped, as in the 2-wide step.
struct Step4 {
    unsigned ref[4];
    float t[4];
};
__device__ __forceinline__ Step4 node4_boxes(const DevNode4* nodes, unsigned idx, const V3& o, const V3& inv, float t_max, unsigned negmask) {
    const float4* q = reinterpret_cast<const float4*>(nodes + idx);
    const float4 a0 = q[0], a1 = q[1], a2 = q[2], b0 = q[3], b1 = q[4], b2 = q[5];
    const uint4 refs = reinterpret_cast<const uint4*>(q)[6];
    const unsigned axes = reinterpret_cast<const uint4*>(q)[7].x;
    Step4 s;
    bool h0 = slab(V3{a0.x, a0.y, a0.z}, V3{a0.w, a1.x, a1.y}, o, inv, t_max, s.t[0]);
    bool h1 = slab(V3{a1.z, a1.w, a2.x}, V3{a2.y, a2.z, a2.w}, o, inv, t_max, s.t[1]);
    bool h2 = slab(V3{b0.x, b0.y, b0.z}, V3{b0.w, b1.x, b1.y}, o, inv, t_max, s.t[2]);
    bool h3 = slab(V3{b1.z, b1.w, b2.x}, V3{b2.y, b2.z, b2.w}, o, inv, t_max, s.t[3]);
    s.ref[0] = h0 ? refs.x : YK_REF_NONE;  // an absent slot already holds YK_REF_NONE
    s.ref[1] = h1 ? refs.y : YK_REF_NONE;
    s.ref[2] = h2 ? refs.z : YK_REF_NONE;
    s.ref[3] = h3 ? refs.w : YK_REF_NONE;
    const bool sp = (negmask >> (axes & 3u)) & 1u, sa = (negmask >> ((axes >> 2) & 3u)) & 1u, sb = (negmask >> ((axes >> 4) & 3u)) & 1u;
#define YK_CSWAP(c, i, j)                         \
    {                                             \
        const unsigned ri = s.ref[i], rj = s.ref[j]; \
        const float ti = s.t[i], tj = s.t[j];     \
        s.ref[i] = (c) ? rj : ri;                 \
        s.ref[j] = (c) ? ri : rj;                 \
        s.t[i] = (c) ? tj : ti;                   \
        s.t[j] = (c) ? ti : tj;                   \
    }
    YK_CSWAP(sa, 0, 1)
    YK_CSWAP(sb, 2, 3)
    YK_CSWAP(sp, 0, 2)
    YK_CSWAP(sp, 1, 3)
#undef YK_CSWAP
    return s;
}
// The first hit slot is entered now and the later ones are pushed, last first.  Closest hit: boxes are screened with the
// relaxed bound, and the first slot (in visiting order) that passes the exact bound is the one entered; slots before it
// fail now as they would in the reference (t_max cannot change before they are tested), the later ones are deferred:
// exact when popped (yk_geom.h).
template <bool CLOSEST, class Stack>
__device__ __forceinline__ bool node4_step(const DevNode4* nodes, const TraceRay& r, Stack& stk, int& sp, unsigned& cur, unsigned* err) {
    Step4 st = node4_boxes(nodes, cur, r.o, r.inv, CLOSEST ? deferred_t_max(r.t_max) : r.t_max, r.negmask);
    if (CLOSEST) {
        bool entered = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool exact = st.ref[k] != YK_REF_NONE && st.t[k] <= r.t_max;
            if (!entered && !exact) st.ref[k] = YK_REF_NONE;
            entered = entered || exact;
        }
    }
    unsigned next = YK_REF_NONE;
    float next_t = 0.0f;
#pragma unroll
    for (int k = 3; k >= 0; --k) {
        if (st.ref[k] != YK_REF_NONE) {
            if (next != YK_REF_NONE) push_capped<YK_STACK_CAP>(stk, sp, next, next_t, err);
            next = st.ref[k];
            next_t = st.t[k];
        }
    }
    if (next == YK_REF_NONE) return false;
    cur = next;  // no leaf was visited since the test: its result is final
    return true;
}

// ---- one-lane loops (k_trace_closest<STATS>, k_whitted, k_path_debug): out_tri = the source shape hit, or -1
template <bool STATS, class Stack>
__device__ __forceinline__ void traverse_closest(const DevScene& sc, TraceRay r, Stack& stk, int& out_tri, TriHit& out_hit, TraceStats* stats, unsigned* err) {
    out_tri = -1;
    if (STATS) stats->node_tests += 1;
    if (!root_hit(sc, r)) return;
    if (STATS) stats->node_hits += 1;
    unsigned cur = sc.root_ref;
    int sp = 0;
    for (;;) {
        if (!(cur & YK_LEAF_BIT)) {
            const StepEnd e = node2_closest<STATS>(load_node(sc.nodes, cur), r, stk, sp, cur, err, stats);
            if (e == STEP_ENTER) continue;
            if (e == STEP_OVERFLOW) return;
        } else {
            leaf_closest<true, false, STATS>(sc, cur & ~YK_LEAF_BIT, true, r, STATS ? &stats->shape_tests : nullptr, [&](unsigned, float4 v1, unsigned, const TriHit& h) {
                out_hit = h;
                out_tri = (int)__float_as_uint(v1.w);
            });
        }
        if (!pop_closest<STATS>(stk, sp, r.t_max, cur, stats)) return;
    }
}
// true = occluded
template <class Stack>
__device__ __forceinline__ bool traverse_any(const DevScene& sc, const TraceRay& r, int area_light, Stack& stk, unsigned* err) {
    if (!root_hit(sc, r)) return false;
    unsigned cur = sc.root_ref;
    int sp = 0;
    for (;;) {
        if (!(cur & YK_LEAF_BIT)) {
            const StepEnd e = node2_any(load_node(sc.nodes, cur), r, stk, sp, cur, err);
            if (e == STEP_ENTER) continue;
            if (e == STEP_OVERFLOW) return false;
        } else if (leaf_any<true>(sc, cur & ~YK_LEAF_BIT, r, area_light)) {
            return true;
        }
        if (!pop_any(stk, sp, cur)) return false;
    }
}

// ------------------------------------------------------------------ persistent-thread traversal
// A wave owns 64 ray slots.  Work arrives in CHUNK-sized index ranges claimed with
// one atomic on the queue head; inside a chunk indices are handed to lanes by a
// wave-local cursor.  Every lane keeps the NEXT ray it will trace already loaded
// in registers (issued as soon as PF_MIN lanes lack one, consumed iterations
// later), so replacing a finished ray costs no memory round trip: with plain
// "fetch when idle" the wave stalled 2-4 us per refill and lost more than the
// idle lanes had cost (profiles/r01_b_sweep.txt).  Each iteration the wave then
// runs ONE of two bodies — an interior-node step for all lanes on interior nodes,
// or, once LEAF_MIN lanes are parked on leaves (or none is on a node), the leaf
// intersection for the parked lanes — so neither body executes at a handful of
// lanes (lane utilisation of the plain loop: 26 %, profiles/r01_a_pmc_summary.json).
// Per-ray arithmetic and visiting order are exactly those of traverse_closest /
// traverse_any above.

// Wave-local work distribution: claims CHUNK indices at a time from *head.
struct ChunkCursor {
    unsigned cur, end;  // wave-uniform
    bool exhausted, took_share;
    __device__ __forceinline__ void init() {
        cur = end = 0;
        exhausted = took_share = false;
    }
    // hands `want` lanes consecutive indices; returns the index of this lane or
    // 0xffffffff.  All lanes of the wave call it (converged).
    // Long queues: CHUNK indices per claim, one atomic on *head each.  A queue that one chunk
    // per wave covers (n <= waves * CHUNK: late bounces, small per-GPU shares, interactive
    // passes) is cut into equal shares instead, wave w takes share w and nothing else: the
    // two atomics per wave of the dynamic scheme (a claim and a failed claim, ~14 K per launch on
    // one address at ~100 M/s) were most of what such a launch cost beyond its longest ray.
    // `cancel`: the launch's relay wave (first wave of block 0) also looks at the host's interruption word when it claims
    // (yk_device.h); finding it set it poisons the head, and every wave's next claim comes back beyond the queue's end.
    template <int CHUNK> __device__ __forceinline__ unsigned take(bool want, unsigned n, unsigned* head, const CancelRef& cancel) {
        unsigned long long mask = __ballot(want);
        if (mask == 0ull || exhausted) return 0xffffffffu;
        if (cur >= end) {
            const unsigned waves = gridDim.x * (blockDim.x / YK_WAVE);
            unsigned base;
            unsigned chunk;
            if (n <= waves * (unsigned)CHUNK) {
                if (took_share) {
                    exhausted = true;
                    return 0xffffffffu;
                }
                took_share = true;
                chunk = (n + waves - 1u) / waves;
                chunk = chunk < 8u ? 8u : chunk;  // fewer, fuller waves for very short queues
                base = (blockIdx.x * (blockDim.x / YK_WAVE) + threadIdx.x / YK_WAVE) * chunk;
            } else {
                chunk = (unsigned)CHUNK;
                base = 0;
                if (lane_id() == 0) {
                    base = atomicAdd(head, chunk);
                    if (blockIdx.x == 0 && threadIdx.x == 0 && cancel_relay(cancel, head)) base = 0xffffffffu;
                }
                base = __shfl(base, 0);
            }
            if (base >= n) {
                exhausted = true;
                return 0xffffffffu;
            }
            cur = base;
            end = base + chunk < n ? base + chunk : n;
        }
        unsigned rank = (unsigned)__popcll(mask & ((1ull << lane_id()) - 1ull));
        unsigned idx = cur + rank;
        unsigned total = (unsigned)__popcll(mask);
        cur = cur + total < end ? cur + total : end;
        return (want && idx < end) ? idx : 0xffffffffu;
    }
};

// The loop both persistent kernels run; they supply the per-ray parts: prefetch(idx) loads queue entry idx into the
// lane's prefetch registers, start() begins the prefetched ray (false: it missed the root box and is done), and
// node_step() / leaf_step() advance a ray standing on an interior node / a leaf (false: the ray is done).  `cur` is the
// lane's current ref.
template <int PF_MIN, int START_MIN, int LEAF_MIN, int CHUNK, class Prefetch, class Start, class NodeStep, class LeafStep>
__device__ __forceinline__ void persistent_rays(unsigned n, unsigned* head, const CancelRef& cancel, const unsigned& cur, Prefetch prefetch, Start start,
                                                NodeStep node_step, LeafStep leaf_step) {
    ChunkCursor work;
    work.init();
    bool active = false, pf_valid = false;
    for (;;) {
        // ---- start prefetched rays once START_MIN lanes are idle (the setup code —
        // six IEEE divisions and the root test — runs divergently, so it is batched)
        const bool startable = !active && pf_valid;
        const bool go = (unsigned)__popcll(__ballot(startable)) >= (unsigned)START_MIN || !__any(active);
        if (go && startable) {
            pf_valid = false;
            active = start();
        }
        // ---- top up the prefetch registers (loads are consumed in a later iteration)
        const unsigned n_need = (unsigned)__popcll(__ballot(!pf_valid));
        if (!work.exhausted && (n_need >= (unsigned)PF_MIN || !__any(active))) {
            const unsigned idx = work.take<CHUNK>(!pf_valid, n, head, cancel);
            if (idx != 0xffffffffu) {
                prefetch(idx);
                pf_valid = true;
            }
        }
        if (!__any(active)) {
            if (work.exhausted && !__any(pf_valid)) break;
            continue;
        }
        // ---- one step, chosen for the whole wave
        const bool on_leaf = active && (cur & YK_LEAF_BIT);
        const bool on_node = active && !(cur & YK_LEAF_BIT);
        const unsigned n_leaf = (unsigned)__popcll(__ballot(on_leaf));
        if (__any(on_node) && n_leaf < (unsigned)LEAF_MIN) {
            if (on_node) active = node_step();
        } else if (on_leaf) {
            active = leaf_step();
        }
    }
}

template <int BLOCK, int LDS_DEPTH, int PF_MIN, int START_MIN, int LEAF_MIN, int CHUNK, bool SPHERES, bool API, bool WIDE>
__global__ __launch_bounds__(BLOCK, TRACE_MIN_WAVES) void k_trace_closest_pt(DevScene sc, const float4* __restrict__ rayO, const float4* __restrict__ rayD,
                                                            const float* __restrict__ t_max_opt, const unsigned* count_ptr, unsigned* head,
                                                            int* __restrict__ hit_tri, float4* __restrict__ hit_out, uint2* spill,
                                                            unsigned spill_stride, unsigned* ctrl, unsigned long long* ray_counter, const unsigned* cancel_host) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH * BLOCK];
    __shared__ float4 lds_top[WIDE ? 1 : TRACE_TOP * 4];
    if (!WIDE) fill_top<BLOCK>(lds_top, sc.top_nodes, sc.n_top);
    auto stk = make_stack<BLOCK, LDS_DEPTH>(lds_stack, spill, spill_stride);
    const CancelRef cancel = CancelRef{cancel_host, cancel_host ? ctrl + YK_CTRL_CANCELLED : nullptr};  // render loop: ctrl is the context's error block
    const unsigned n = queue_length(count_ptr, cancel, ray_counter);
    const unsigned root = WIDE ? 0u : (sc.n_top ? YK_TOP_BIT : sc.root_ref);
    unsigned* err = ctrl + YK_CTRL_ERR;

    float4 pf_o = make_float4(0, 0, 0, 0), pf_d = make_float4(0, 0, 1, 0);
    float pf_t = 0.0f;
    unsigned pf_idx = 0, ray_i = 0, cur = 0;
    TraceRay r = idle_ray();
    int sp = 0, best = -1;
    TriHit best_hit = TriHit{0, 0, 0, 0};
    const auto retire = [&]() {
        hit_tri[ray_i] = best;
        if (API && hit_out) hit_out[ray_i] = make_float4(best_hit.t, best_hit.b0, best_hit.b1, best_hit.b2);
        return false;
    };
    persistent_rays<PF_MIN, START_MIN, LEAF_MIN, CHUNK>(
        n, head, cancel, cur,
        [&](unsigned idx) {
            pf_o = rayO[idx];
            pf_d = rayD[idx];
            pf_t = (API && t_max_opt) ? t_max_opt[idx] : __builtin_inff();
            pf_idx = idx;
        },
        [&]() {
            r = ray_setup(f4_xyz(pf_o), f4_xyz(pf_d), API ? pf_t : __builtin_inff());
            ray_i = pf_idx;
            if (!root_hit(sc, r)) {
                hit_tri[ray_i] = -1;
                return false;
            }
            cur = root;
            sp = 0;
            best = -1;
            return true;
        },
        [&]() {
            if (WIDE) {
                if (node4_step<true>(sc.nodes4, r, stk, sp, cur, err)) return true;
            } else {
                const NodeBoxes nb = load_node(lds_top, sc.nodes, cur);
                YK_EXPERIMENT_NODE(sc.nodes + cur, nb);
                if (node2_closest<false>(nb, r, stk, sp, cur, err, nullptr) != STEP_POP) return true;  // after an overflow: the near child, an empty stack
            }
            return pop_closest<false>(stk, sp, r.t_max, cur, nullptr) || retire();
        },
        [&]() {
            leaf_closest<SPHERES, false, false>(sc, cur & ~YK_LEAF_BIT, true, r, nullptr, [&](unsigned prim, float4 v1, unsigned pflags, const TriHit& h) {
                if (API) best_hit = h;
                // API callers get the source shape; the render loop gets the leaf-order slot, from which k_shade reaches
                // everything it needs in one hop (hit_surface_prim)
                best = API ? (int)__float_as_uint(v1.w) : YK_HIT_WORD(prim, pflags);
            });
            return pop_closest<false>(stk, sp, r.t_max, cur, nullptr) || retire();
        });
}

// Shadow rays: shO/shD are dense (compacted by `shade`); slot_of[k] is where the
// verdict goes (vis[slot] = 2 when occluded); slot_of == NULL (API mode): vis[k] = 0/1.
template <int BLOCK, int LDS_DEPTH, int PF_MIN, int START_MIN, int LEAF_MIN, int CHUNK, bool SPHERES, bool WIDE>
__global__ __launch_bounds__(BLOCK, TRACE_MIN_WAVES) void k_trace_any_pt(DevScene sc, const float4* __restrict__ shO, const float4* __restrict__ shD,
                                                        const unsigned* __restrict__ slot_of, const unsigned* count_ptr, unsigned* head,
                                                        unsigned char* __restrict__ vis, uint2* spill, unsigned spill_stride, unsigned* ctrl,
                                                        unsigned long long* shadow_counter, const unsigned* cancel_host) {
    __shared__ unsigned lds_stack[LDS_DEPTH * BLOCK];
    __shared__ float4 lds_top[WIDE ? 1 : TRACE_ANY_TOP * 4];
    if (!WIDE) fill_top<BLOCK>(lds_top, sc.top_nodes_any, sc.n_top_any);
    auto stk = make_stack<BLOCK, LDS_DEPTH>(lds_stack, spill, spill_stride);
    const CancelRef cancel = CancelRef{cancel_host, cancel_host ? ctrl + YK_CTRL_CANCELLED : nullptr};
    const unsigned n = queue_length(count_ptr, cancel, shadow_counter);
    const unsigned root = WIDE ? 0u : (sc.n_top_any ? YK_TOP_BIT : sc.root_ref);
    unsigned* err = ctrl + YK_CTRL_ERR;

    float4 pf_o = make_float4(0, 0, 0, 0), pf_d = make_float4(0, 0, 1, 0);
    unsigned pf_slot = 0, slot = 0, cur = 0;
    TraceRay r = idle_ray();
    int sp = 0, area_light = -1;
    const auto unoccluded = [&]() {
        if (!slot_of) vis[slot] = 0;
        return false;
    };
    persistent_rays<PF_MIN, START_MIN, LEAF_MIN, CHUNK>(
        n, head, cancel, cur,
        [&](unsigned k) {
            pf_o = shO[k];
            pf_d = shD[k];
            pf_slot = slot_of ? slot_of[k] : k;
        },
        [&]() {
            r = ray_setup(f4_xyz(pf_o), f4_xyz(pf_d), pf_o.w);
            area_light = (int)__float_as_uint(pf_d.w);
            slot = pf_slot;
            if (!root_hit(sc, r)) return unoccluded();
            cur = root;
            sp = 0;
            return true;
        },
        [&]() {
            const bool entered = WIDE ? node4_step<false>(sc.nodes4, r, stk, sp, cur, err)
                                      : node2_any(load_node(lds_top, sc.nodes, cur), r, stk, sp, cur, err) != STEP_POP;  // after an overflow: the near child, an empty stack
            if (entered) return true;
            return pop_any(stk, sp, cur) || unoccluded();
        },
        [&]() {
            if (leaf_any<SPHERES>(sc, cur & ~YK_LEAF_BIT, r, area_light)) {
                vis[slot] = slot_of ? 2 : 1;
                return false;
            }
            return pop_any(stk, sp, cur) || unoccluded();
        });
}

// Persistent waves: each wave pulls 64 consecutive rays from a global head until
// the queue (whose length only the device knows) is drained.
template <int BLOCK, int LDS_DEPTH, bool STATS>
__global__ __launch_bounds__(BLOCK) void k_trace_closest(DevScene sc, const float4* rayO, const float4* rayD, const float* t_max_opt,
                                                         const unsigned* count_ptr, unsigned* head, int* hit_tri, float4* hit_out,
                                                         uint4* stats_out, uint2* spill, unsigned spill_stride, unsigned* ctrl,
                                                         unsigned long long* ray_counter) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH * BLOCK];
    auto stk = make_stack<BLOCK, LDS_DEPTH>(lds_stack, spill, spill_stride);
    const unsigned n = queue_length(count_ptr, CancelRef{nullptr, nullptr}, ray_counter);
    for (;;) {
        unsigned base = 0;
        if (lane_id() == 0) base = atomicAdd(head, YK_WAVE);
        base = __shfl(base, 0);
        if (base >= n) break;
        unsigned i = base + lane_id();
        if (i < n) {
            float4 ro = rayO[i], rd = rayD[i];
            float tm = t_max_opt ? t_max_opt[i] : __builtin_inff();
            int tri;
            TriHit h = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
            TraceStats s = TraceStats{0, 0, 0};
            traverse_closest<STATS>(sc, ray_setup(f4_xyz(ro), f4_xyz(rd), tm), stk, tri, h, &s, ctrl + YK_CTRL_ERR);
            hit_tri[i] = tri;
            if (hit_out) hit_out[i] = make_float4(h.t, h.b0, h.b1, h.b2);
            if (STATS) stats_out[i] = make_uint4(s.node_tests, s.node_hits, s.shape_tests, 0u);
        }
    }
}


// ------------------------------------------------------------------ Whitted
// Whitted::li_internal (whitted.rs:74-181), one lane per camera sample.  The recursion —
// direct lighting, then the specular reflection subtree, then the specular transmission
// subtree, each child weighted as (f * li) * |wi . ns| with no pdf (whitted.rs:66) — is run
// depth first with an explicit frame stack, because the ONE sampler of the pixel sample is
// drawn from in exactly that order (2 dimensions per light at every hit).  Child rays come from
// sample_f with u = (0, 0) (whitted.rs:49-51): the tree itself does not depend on the sampler,
// and only glass has specular lobes, so only glass hits push a frame.
#define YK_WHITTED_MAX_DEPTH 16
struct WhittedFrame {
    RGB sum;          // sum_li of the suspended call
    RGB pend_f;       // weight of the child being evaluated
    float pend_cos;
    bool t_valid;     // the transmission child, evaluated after the reflection subtree
    V3 t_o, t_d;
    RGB t_f;
    float t_cos;
};

template <int BLOCK, int LDS_DEPTH>
__global__ __launch_bounds__(BLOCK) void k_whitted(DevScene sc, RenderParams prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab, PathBuffers cur,
                                                   uint32_t n, float4* sample_buf, uint2* spill, unsigned spill_stride, unsigned* ctrl,
                                                   unsigned long long* counters) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH * BLOCK];
    auto stk = make_stack<BLOCK, LDS_DEPTH>(lds_stack, spill, spill_stride);
    unsigned* err = ctrl + YK_CTRL_ERR;
    unsigned long long n_rays = 0, n_shadow = 0;
    if (cancel_raised(prm.cancel)) n = 0;  // interrupted before this launch started (yk_device.h, CancelRef)
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const PathState ps = path_load(cur, i);
        V3 o = ps.o, d = ps.d;
        const unsigned sid = ps.sid;
        SamplerState st = path_sampler(prm, pixel_xy, sample_index_tab, ps);
        WhittedFrame frames[YK_WHITTED_MAX_DEPTH];
        int sp = 0;  // frames on the stack = depth of the call being evaluated
        bool is_specular = false;
        RGB ret = RGB{0.0f, 0.0f, 0.0f};
        unsigned sample_rays = 0;  // RadianceResult::ray_scene_intersections of this sample (whitted.rs:174-178)
        for (;;) {
            // ---- call: li_internal(ray (o, d), depth = sp, is_specular)
            n_rays += 1;
            sample_rays += 1;
            int shape;
            TriHit th = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
            traverse_closest<false>(sc, ray_setup(o, d, __builtin_inff()), stk, shape, th, nullptr, err);
            bool called = false;
            if (shape < 0) {
                ret = RGB{sc.background[0], sc.background[1], sc.background[2]};  // whitted.rs:171
            } else {
                Surface sf = hit_surface(sc, (uint32_t)shape, o, d);
                Material mat = sc.materials[sf.material];
                if (mat.tex) {  // matte.rs:29-30
                    RGB kd = texture_eval(sc, mat.tex - 1u, sf.u, sf.v);
                    mat.a[0] = kd.r;
                    mat.a[1] = kd.g;
                    mat.a[2] = kd.b;
                    if (is_black(kd)) mat.kind = MK_BLACK;
                }
                const Frame fr = make_frame(sf.n, sf.ns, sf.dpdus);
                RGB sum = RGB{0.0f, 0.0f, 0.0f};
                for (unsigned l = 0; l < sc.n_lights; ++l) {  // whitted.rs:113-133, the fold of path.rs:102-119
                    float ux, uy;
                    light_draw_2d(prm.sampler, st, sc.lights[l], ux, uy);
                    LightSample ls = sample_light(sc.lights[l], (int)l, sf.p, ux, uy);
                    if (is_black(ls.li)) continue;
                    RGB f = bsdf_f(mat, fr, sf.wo, ls.l);
                    if (!ls.has_vis || is_black(f)) continue;
                    V3 offset = sf.n * 0.001f;  // VisibilityTester::ray = p0.spawn_ray_to(p1), interaction.rs:44-59
                    V3 so = dot(ls.p1 - sf.p, sf.n) > 0.0f ? sf.p + offset : sf.p - offset;
                    n_shadow += 1;
                    const RGB contrib = f * ls.li * rclamp(dot_nv(sf.ns, ls.l), 0.0f, 1.0f) / ls.pdf;
                    if ((prm.nee_skip & YK_NEE_SKIP_ZERO) && is_black(contrib)) continue;  // vertex_light's rule (yk_shade.h): sum + (+-0) is sum, the ray is counted and not walked
                    if (!traverse_any(sc, ray_setup(so, ls.p1 - so, 0.9999f), ls.area_light, stk, err)) sum = sum + contrib;
                }
                if (sp == 0 || is_specular) {  // whitted.rs:135-137, rectangular_light.rs:75-81
                    if (sf.area_light >= 0) {
                        const DevLight& L = sc.lights[sf.area_light];
                        sum = sum + (dot_nv(sf.n, -d) > 0.0f ? RGB{L.i[0], L.i[1], L.i[2]} : RGB{0.0f, 0.0f, 0.0f});
                    } else {
                        sum = sum + RGB{0.0f, 0.0f, 0.0f};
                    }
                }
                ret = sum;
                if ((unsigned)sp + 1u < prm.max_depth && mat.kind == MK_GLASS) {  // whitted.rs:139-167
                    BsdfSample rs = bsdf_sample_specular(mat, fr, sf.wo, BX_REFLECTION);
                    BsdfSample ts = bsdf_sample_specular(mat, fr, sf.wo, BX_TRANSMISSION);
                    if (rs.type != BX_NONE || ts.type != BX_NONE) {
                        WhittedFrame& fm = frames[sp];
                        fm.sum = sum;
                        fm.t_valid = false;
                        const BsdfSample& first = rs.type != BX_NONE ? rs : ts;
                        if (rs.type != BX_NONE && ts.type != BX_NONE) {
                            fm.t_valid = true;
                            fm.t_o = spawn_origin(sf.p, sf.n, ts.wi);
                            fm.t_d = ts.wi;
                            fm.t_f = ts.f;
                            fm.t_cos = fabsf(dot_nv(ts.wi, sf.ns));
                        }
                        fm.pend_f = first.f;
                        fm.pend_cos = fabsf(dot_nv(first.wi, sf.ns));
                        o = spawn_origin(sf.p, sf.n, first.wi);
                        d = first.wi;
                        is_specular = true;  // sample_type.contains(SPECULAR), whitted.rs:64
                        ++sp;
                        called = true;
                    }
                }
            }
            if (called) continue;
            // ---- return: fold `ret` into the suspended callers
            bool again = false;
            while (sp > 0) {
                WhittedFrame& fm = frames[sp - 1];
                fm.sum = fm.sum + fm.pend_f * ret * fm.pend_cos;  // ret.li = f * ret.li * |wi . ns| ; sum_li += li
                if (fm.t_valid) {
                    fm.t_valid = false;
                    fm.pend_f = fm.t_f;
                    fm.pend_cos = fm.t_cos;
                    o = fm.t_o;
                    d = fm.t_d;
                    is_specular = true;
                    again = true;
                    break;
                }
                ret = fm.sum;
                --sp;
            }
            if (!again) break;
        }
        sample_buf[sid] = make_float4(ret.r, ret.g, ret.b, __uint_as_float(sample_rays));  // .w: read by yk_li alone, as bits
    }
    // ray counts: one atomic per wave
    for (int off = 32; off > 0; off >>= 1) {
        n_rays += __shfl_down(n_rays, off);
        n_shadow += __shfl_down(n_shadow, off);
    }
    if (lane_id() == 0 && counters) {
        if (n_rays) atomicAdd(counters, n_rays);
        if (n_shadow) atomicAdd(counters + 1, n_shadow);
    }
}

// ------------------------------------------------------------------ Path::li_debug
// Path::li_internal with ray collection (path.rs:48-204) for yk_li_debug, one lane per sample: the bounce loop of the
// wavefront — traverse_closest, the shading steps of yk_shade.h, traverse_any for each shadow ray, vertex_accumulate —
// run to the end of the path in one lane, so the radiance is the wavefront's bit for bit.  Each sample writes its
// yk_integrator_ray records (two float4: o.xyz d.x | d.yz t_max type) in the reference's push order, the first
// `ray_cap` of them at out_rays[i * ray_cap ...], and in out_n_rays the number it produced.
__device__ __forceinline__ void debug_ray_store(float4* out, uint32_t i, unsigned ray_cap, unsigned k, V3 o, V3 d, float t_max, unsigned type) {
    if (k >= ray_cap) return;
    float4* r = out + 2 * ((size_t)i * ray_cap + k);
    r[0] = make_float4(o.x, o.y, o.z, d.x);
    r[1] = make_float4(d.y, d.z, t_max, __uint_as_float(type));
}
// Bounds3::intersections (bounds.rs:176-206) of the root box for a ray with t_max = inf: the exit distance, or
// `miss_len` when the box is missed.  Operation by operation with Rust's f32::min / max (rmin / rmax).
__device__ __forceinline__ float root_exit(const DevScene& sc, V3 o, V3 d, float miss_len) {
    const float ix = 1.0f / d.x, iy = 1.0f / d.y, iz = 1.0f / d.z;
    const float t0x = (sc.root_bmin[0] - o.x) * ix, t0y = (sc.root_bmin[1] - o.y) * iy, t0z = (sc.root_bmin[2] - o.z) * iz;
    const float t1x = (sc.root_bmax[0] - o.x) * ix, t1y = (sc.root_bmax[1] - o.y) * iy, t1z = (sc.root_bmax[2] - o.z) * iz;
    const float tmin = rmax(rmax(rmin(t0x, t1x), rmax(rmin(t0y, t1y), rmin(t0z, t1z))), 0.0f);
    const float tmax = rmin(rmin(rmax(t0x, t1x), rmin(rmax(t0y, t1y), rmax(t0z, t1z))), __builtin_inff());
    return tmin <= tmax ? tmax : miss_len;
}

template <int BLOCK, int LDS_DEPTH>
__global__ __launch_bounds__(BLOCK) void k_path_debug(DevScene sc, RenderParams prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab, PathBuffers cur,
                                                      uint32_t n, float4* sample_buf, uint32_t* out_counts, float4* out_rays, unsigned ray_cap,
                                                      uint32_t* out_n_rays, float min_len, uint2* spill, unsigned spill_stride, unsigned* ctrl) {
    __shared__ unsigned long long lds_stack[LDS_DEPTH * BLOCK];
    auto stk = make_stack<BLOCK, LDS_DEPTH>(lds_stack, spill, spill_stride);
    unsigned* err = ctrl + YK_CTRL_ERR;
    if (cancel_raised(prm.cancel)) n = 0;  // interrupted before this launch started (yk_device.h, CancelRef)
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const PathState ps = path_load(cur, i);
        V3 o = ps.o, d = ps.d;
        const unsigned sid = ps.sid;
        SamplerState st = path_sampler(prm, pixel_xy, sample_index_tab, ps);
        RGB L = RGB{0.0f, 0.0f, 0.0f}, beta = ps.beta;
        unsigned bounces = 0, n_closest = 0, k = 0, type = YK_RAY_DIRECT;
        bool specular_bounce = false, alive = prm.max_depth > 0;
        while (alive) {
            // the segment: Direct keeps the camera ray's t_max, later ones the root box's exit; a hit replaces it with t
            n_closest += 1;
            int shape;
            TriHit th = TriHit{0.0f, 0.0f, 0.0f, 0.0f};
            traverse_closest<false>(sc, ray_setup(o, d, __builtin_inff()), stk, shape, th, nullptr, err);
            if (shape < 0) {
                debug_ray_store(out_rays, i, ray_cap, k++, o, d, type == YK_RAY_DIRECT ? __builtin_inff() : root_exit(sc, o, d, min_len), type);
                L = vertex_accumulate(prm, L, RGB{1.0f, 1.0f, 1.0f}, RGB{0.0f, 0.0f, 0.0f}, vertex_miss_term(sc, beta), YK_PEND_MISS);
                break;
            }
            debug_ray_store(out_rays, i, ray_cap, k++, o, d, th.t, type);
            PathVertex v;
            v.sf = hit_surface(sc, (uint32_t)shape, o, d);  // the source shape, as k_whitted (vertex_setup takes a leaf-order slot)
            vertex_setup_material(sc, d, v);
            debug_ray_store(out_rays, i, ray_cap, k++, v.sf.p, v.sf.n, min_len, YK_RAY_NORMAL);
            RGB radiance = RGB{0.0f, 0.0f, 0.0f};
            for (unsigned l = 0; l < sc.n_lights; ++l) {
                const NeeSample ne = vertex_light<true>(sc, prm, st, l, v);
                if (ne.want || ne.has_ray) debug_ray_store(out_rays, i, ray_cap, k++, ne.so, ne.sd, YK_SHADOW_T_MAX, YK_RAY_SHADOW);
                if (ne.want && !traverse_any(sc, ray_setup(ne.so, ne.sd, YK_SHADOW_T_MAX), ne.al, stk, err)) radiance = radiance + ne.contrib;
            }
            const RGB beta_in = beta;  // vertex_accumulate takes the throughput the vertex was entered with
            const VertexEnd e = vertex_finish(sc, prm, st, v, beta, bounces, specular_bounce);
            L = vertex_accumulate(prm, L, beta_in, radiance, e.term, e.kind);
            alive = e.alive;
            o = e.no;
            d = e.wi;
            type = (e.lobe & BX_REFLECTION) ? YK_RAY_REFLECTION : YK_RAY_REFRACTION;
        }
        sample_buf[sid] = make_float4(L.r, L.g, L.b, 0.0f);
        out_counts[i] = n_closest;
        out_n_rays[i] = k;
    }
}

// ------------------------------------------------------------------ launchers
#ifndef TRACE_PF_MIN
#define TRACE_PF_MIN 16
#endif
#ifndef TRACE_START_MIN
#define TRACE_START_MIN 8
#endif
#ifndef TRACE_LEAF_MIN
#define TRACE_LEAF_MIN 16
#endif
#ifndef TRACE_CHUNK
#define TRACE_CHUNK 128
#endif

unsigned trace_block_size() { return TRACE_BLOCK; }
unsigned trace_spill_depth() { return YK_STACK_CAP - TRACE_LDS; }
unsigned trace_top_nodes() { return TRACE_TOP; }
unsigned trace_top_nodes_any() { return TRACE_ANY_TOP; }
static_assert(TRACE_ANY_LDS * TRACE_BLOCK * 4 + TRACE_ANY_TOP * 64 <= TRACE_LDS * TRACE_BLOCK * 8 + TRACE_TOP * 64 + 1024, "the any-hit kernel must fit the block count of the closest-hit kernel");
static_assert(TRACE_ANY_LDS >= TRACE_LDS, "the spill buffer is sized for TRACE_LDS entries in LDS");
unsigned trace_blocks_per_cu() {
    unsigned by_lds = (160u * 1024u) / (TRACE_LDS * TRACE_BLOCK * 8u + TRACE_TOP * 64u);
    unsigned by_waves = (unsigned)TRACE_MIN_WAVES * 256u / TRACE_BLOCK;
    return by_lds < by_waves ? by_lds : by_waves;
}

void launch_trace_closest(hipStream_t s, unsigned grid, const DevScene& sc, const float4* rayO, const float4* rayD, const float* t_max_opt,
                          const unsigned* count_ptr, unsigned* head, int* hit_tri, float4* hit_out, uint4* stats_out, uint2* spill,
                          unsigned spill_stride, unsigned* ctrl, unsigned long long* ray_counter, const unsigned* cancel_host) {
    if (stats_out)
        hipLaunchKernelGGL((k_trace_closest<TRACE_BLOCK, TRACE_LDS, true>), dim3(grid), dim3(TRACE_BLOCK), 0, s, sc, rayO, rayD, t_max_opt, count_ptr,
                           head, hit_tri, hit_out, stats_out, spill, spill_stride, ctrl, ray_counter);
    else {
        const bool api = t_max_opt != nullptr || hit_out != nullptr;
#define YK_LAUNCH_CLOSEST(SPH, API, WIDE)                                                                                                              \
    hipLaunchKernelGGL((k_trace_closest_pt<TRACE_BLOCK, TRACE_LDS, TRACE_PF_MIN, TRACE_START_MIN, TRACE_LEAF_MIN, TRACE_CHUNK, SPH, API, WIDE>), dim3(grid), \
                       dim3(TRACE_BLOCK), 0, s, sc, rayO, rayD, t_max_opt, count_ptr, head, hit_tri, hit_out, spill, spill_stride, ctrl, ray_counter, cancel_host)
#define YK_LAUNCH_CLOSEST_W(SPH, API) \
    if (sc.nodes4) YK_LAUNCH_CLOSEST(SPH, API, true); else YK_LAUNCH_CLOSEST(SPH, API, false)
        if (sc.spheres) {
            if (api) { YK_LAUNCH_CLOSEST_W(true, true); } else { YK_LAUNCH_CLOSEST_W(true, false); }
        } else {
            if (api) { YK_LAUNCH_CLOSEST_W(false, true); } else { YK_LAUNCH_CLOSEST_W(false, false); }
        }
#undef YK_LAUNCH_CLOSEST_W
#undef YK_LAUNCH_CLOSEST
    }
}
void launch_whitted(hipStream_t s, unsigned grid, const DevScene& sc, const RenderParams& prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab,
                    PathBuffers cur, uint32_t n, float4* sample_buf, uint2* spill, unsigned spill_stride, unsigned* ctrl, unsigned long long* counters) {
    hipLaunchKernelGGL((k_whitted<TRACE_BLOCK, TRACE_LDS>), dim3(grid), dim3(TRACE_BLOCK), 0, s, sc, prm, pixel_xy, sample_index_tab, cur, n, sample_buf, spill,
                       spill_stride, ctrl, counters);
}
unsigned whitted_max_depth() { return YK_WHITTED_MAX_DEPTH; }
void launch_path_debug(hipStream_t s, unsigned grid, const DevScene& sc, const RenderParams& prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab,
                       PathBuffers cur, uint32_t n, float4* sample_buf, uint32_t* out_counts, float4* out_rays, unsigned ray_cap, uint32_t* out_n_rays,
                       float min_len, uint2* spill, unsigned spill_stride, unsigned* ctrl) {
    hipLaunchKernelGGL((k_path_debug<TRACE_BLOCK, TRACE_LDS>), dim3(grid), dim3(TRACE_BLOCK), 0, s, sc, prm, pixel_xy, sample_index_tab, cur, n, sample_buf,
                       out_counts, out_rays, ray_cap, out_n_rays, min_len, spill, spill_stride, ctrl);
}
void launch_trace_any(hipStream_t s, unsigned grid, const DevScene& sc, const ShadowQueue& q, unsigned char* vis, uint2* spill, unsigned spill_stride,
                      unsigned* ctrl, unsigned long long* shadow_counter, const unsigned* cancel_host) {
#define YK_LAUNCH_ANY(SPH, WIDE)                                                                                                                       \
    hipLaunchKernelGGL((k_trace_any_pt<TRACE_BLOCK, TRACE_ANY_LDS, TRACE_PF_MIN, TRACE_START_MIN, TRACE_LEAF_MIN, TRACE_CHUNK, SPH, WIDE>), dim3(grid),     \
                       dim3(TRACE_BLOCK), 0, s, sc, (const float4*)q.O, (const float4*)q.D, (const unsigned*)q.slot, (const unsigned*)q.count, q.head, vis, spill, spill_stride, ctrl, shadow_counter, cancel_host)
    if (sc.spheres) {
        if (sc.nodes4) YK_LAUNCH_ANY(true, true); else YK_LAUNCH_ANY(true, false);
    } else {
        if (sc.nodes4) YK_LAUNCH_ANY(false, true); else YK_LAUNCH_ANY(false, false);
    }
#undef YK_LAUNCH_ANY
}

}  // namespace yk
