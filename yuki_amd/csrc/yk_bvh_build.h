// yk_bvh_build.h — the level-synchronous BVH builder's steps, written once for the gfx950 kernels
// (yk_bvh_build.hip) and for the host instance of the same algorithm (ibid.).  The tree it builds is
// the host recursion's (yk_host.cpp, Builder::build), bit for bit; the expressions below restate that
// file's, they do not replace them — the recursion stays the yardstick.
//
// Shape of the build
//   * The primitive array is SoA (Prims).  Open ranges [start, end) of it are worked level by level
//     (level_range): bounds, centroid bounds, split decision, partition — on the device by one block
//     of 8 waves per range.  A range of at most
//     `small_range` shapes is finished by ONE lane running the recursion's logic with its pending
//     right children chained through the node slots themselves (build_serial): no local stack.
//   * Node slots: the node of range [s, e) at slot p owns slots [p, p + 2(e-s) - 1); its first child
//     sits at p + 1, its second at p + 2(mid - s).  Slots are disjoint by construction and their
//     order IS the depth-first order, so the final numbering is a compaction of the used slots.
//   * Interior bounds are not the range reduction: they are rmin / rmax of the two children's boxes
//     in child order, filled in bottom-up after the compaction (yk_host.cpp:508-511).
//
// Which reductions must keep the fold's order.  rmin / rmax keep the LEFT operand on a tie, and the
// only tie between different bit patterns is +0 / -0 (non-finite input never reaches this builder).
// The sign of a zero can reach the result only through a LEAF's stored box: centroid bounds, SAH
// bucket boxes and the range bounds of a split node feed differences, areas and comparisons, where
// +0 and -0 act alike (the cost is `1 + x`, the bucket index `(int)max(12 o, 0)`, the middle
// `(lo + hi) / 2` is compared only).  So the parallel reductions are free in their order, and every
// leaf box is folded by one lane from left to right, exactly as emit_leaf's caller does.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/yuki_hip.h"
#include "yk_math.h"

namespace yk {
namespace lv {

struct Prims {  // SoA primitive array: bounds, "centroid" (p_min + diagonal / 0.5, yk_host.cpp:544), shape id
    float* bmin[3];
    float* bmax[3];
    float* c[3];
    uint32_t* shape;
};
struct Params {
    uint32_t max_shapes, method, small_range;
};
struct Range {
    uint32_t start, end, slot, depth;
};
struct Counters {  // one block of words the kernels update with integer atomics
    uint32_t n_next, n_small, max_depth, max_leaf, split_failed, reason, pad0, pad1;
};
struct Box {
    float lo[3], hi[3];
};
const int kBuckets = 12;
const uint32_t kNone = 0xffffffffu;

YK_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
YK_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

YK_HD Box box_empty() {
    const float big = 3.40282347e+38f;
    return Box{{big, big, big}, {-big, -big, -big}};
}
YK_HD void box_add(Box& b, const float* lo, const float* hi) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = rmin(b.lo[k], lo[k]);
        b.hi[k] = rmax(b.hi[k], hi[k]);
    }
}
// v[axis] by selects: a variable index into a local array would put the array into scratch on the device
template <class T> YK_HD T pick3(const T* v, int axis) { return axis == 0 ? v[0] : (axis == 1 ? v[1] : v[2]); }
YK_HD float box_area(const Box& b) {  // bounds.rs:134-138
    float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return 2.0f * (dx * dy + dz * dy + dx * dz);
}
YK_HD int box_max_extent(const Box& b) {  // bounds.rs:147-156
    float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    if (dx > dy && dx > dz) return 0;
    if (dy > dz) return 1;
    return 2;
}
// impl_bounds.rs offset() then `(12*o).max(0) as usize` (yk_host.cpp sah_bucket)
YK_HD int sah_bucket(float cb_lo, float cb_hi, float c) {
    float o = c - cb_lo;
    if (cb_hi != cb_lo) o /= cb_hi - cb_lo;
    float bf = (float)kBuckets * o;
    float m = rmax(bf, 0.0f);
    if (m != m) return 0;
    if (m >= (float)kBuckets) return kBuckets - 1;
    int b = (int)m;
    return b < kBuckets - 1 ? b : kBuckets - 1;
}
// The cost loop of split_sah: the bucket to split after, or -1 when a leaf is cheaper (kNoSplit).
YK_HD int sah_choose(const uint32_t* counts, const Box* boxes, const Box& bounds, uint32_t n) {
    float best_cost = 0.0f;
    int best = 0;
    const float denom = rmax(box_area(bounds), 1e-10f);
    for (int i = 0; i < kBuckets - 1; ++i) {
        Box b0 = box_empty(), b1 = box_empty();
        uint32_t c0 = 0, c1 = 0;
        for (int j = 0; j <= i; ++j) {
            box_add(b0, boxes[j].lo, boxes[j].hi);
            c0 += counts[j];
        }
        for (int j = i + 1; j < kBuckets; ++j) {
            box_add(b1, boxes[j].lo, boxes[j].hi);
            c1 += counts[j];
        }
        float cost = 1.0f + ((float)c0 * box_area(b0) + (float)c1 * box_area(b1)) / denom;
        if (i == 0 || cost < best_cost) {  // min_by keeps the first minimum
            best_cost = cost;
            best = i;
        }
    }
    return best_cost < (float)n ? best : -1;
}

YK_HD void prim_swap(const Prims& p, uint32_t i, uint32_t j) {
    for (int k = 0; k < 3; ++k) {
        float t = p.bmin[k][i];
        p.bmin[k][i] = p.bmin[k][j];
        p.bmin[k][j] = t;
        t = p.bmax[k][i];
        p.bmax[k][i] = p.bmax[k][j];
        p.bmax[k][j] = t;
        t = p.c[k][i];
        p.c[k][i] = p.c[k][j];
        p.c[k][j] = t;
    }
    uint32_t s = p.shape[i];
    p.shape[i] = p.shape[j];
    p.shape[j] = s;
}

// "select_nth spec" (DESIGN.md): 3-way quickselect, middle pivot, on c[axis]
YK_HD void select_nth(const Prims& p, uint32_t lo, uint32_t hi, uint32_t k, int axis) {
    const float* c = pick3(p.c, axis);
    while (hi - lo > 1) {
        const float pivot = c[lo + (hi - lo) / 2];
        uint32_t i = lo, lt = lo, gt = hi;
        while (i < gt) {
            const float v = c[i];
            if (v < pivot) {
                if (lt != i) prim_swap(p, lt, i);
                ++lt;
                ++i;
            } else if (v > pivot) {
                --gt;
                if (i != gt) prim_swap(p, i, gt);
            } else {
                ++i;
            }
        }
        if (k < lt)
            hi = lt;
        else if (k >= gt)
            lo = gt;
        else
            return;
    }
}

// ---- the two-ended swap partition in closed form -------------------------------------------------
// swap_partition (yk_host.cpp, the algorithm of itertools::partition) leaves this arrangement: with
// F[k] the k-th position from the left whose element FAILS the predicate and T[k] the k-th position
// from the right whose element PASSES it, F[k] and T[k] are exchanged for every k while F[k] < T[k];
// nothing else moves; the result is the number of passing elements.  Both lists live in one array of
// positions over the range: F[k] at start + k, the j-th passing position FROM THE LEFT at end - 1 - j,
// which puts T[k] at start + n_fail + k.
YK_HD uint32_t part_list_slot(uint32_t start, uint32_t end, uint32_t i, bool pass, uint32_t pass_before) {
    return pass ? end - 1u - pass_before : start + ((i - start) - pass_before);
}
YK_HD bool part_swap_pair(const uint32_t* list, uint32_t start, uint32_t end, uint32_t n_pass, uint32_t k, uint32_t& f, uint32_t& t) {
    const uint32_t n_fail = (end - start) - n_pass;
    if (k >= n_fail || k >= n_pass) return false;
    f = list[start + k];
    t = list[start + n_fail + k];
    return f < t;
}

// ---- node slots ------------------------------------------------------------------------------------
// A slot is the 8 words of a yk_bvh_node; an interior node's `a` holds the SLOT of its second child
// until the compaction renumbers it.  slot_depth[s] is the node's depth, 0 while the slot is unused.
YK_HD void write_leaf(uint32_t* slots, uint32_t* slot_depth, const Prims& p, const Range& r) {
    Box b = box_empty();  // the exact fold, left to right: a leaf's box is stored
    for (uint32_t i = r.start; i < r.end; ++i) {
        const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
        box_add(b, lo, hi);
    }
    uint32_t* w = slots + 8 * (size_t)r.slot;
    for (int k = 0; k < 3; ++k) {
        w[k] = f2u(b.lo[k]);
        w[3 + k] = f2u(b.hi[k]);
    }
    w[6] = r.start;                                         // first_shape_index: leaves come in range order
    w[7] = ((r.end - r.start) & 0xffffu) | (1u << 24);      // count (u16), axis 0, is_leaf 1
    slot_depth[r.slot] = r.depth;
}
YK_HD uint32_t write_interior(uint32_t* slots, uint32_t* slot_depth, const Range& r, uint32_t mid, int axis) {
    const uint32_t second = r.slot + 2u * (mid - r.start);
    uint32_t* w = slots + 8 * (size_t)r.slot;
    for (int k = 0; k < 6; ++k) w[k] = 0u;  // filled bottom-up from the children
    w[6] = second;
    w[7] = (uint32_t)axis << 16;
    slot_depth[r.slot] = r.depth;
    return second;
}

struct SerialStats {
    uint32_t max_depth, max_leaf, split_failed;
};

// One lane finishes a range: Builder::build with an explicit stack.  A pending second child is
// parked in its own (still unused) slot — {start, end, depth, previous pending slot} — so the stack
// needs no storage of its own and no bound on its depth.
YK_HD void build_serial(const Prims& p, const Params& prm, Range cur, uint32_t* slots, uint32_t* slot_depth, SerialStats& st) {
    uint32_t top = kNone;
    for (;;) {
        if (cur.depth > st.max_depth) st.max_depth = cur.depth;
        const uint32_t start = cur.start, end = cur.end, n = end - start;
        bool leaf = n <= prm.max_shapes;
        uint32_t mid = start;
        int axis = 0;
        if (!leaf) {
            Box bounds = box_empty(), cb = box_empty();
            for (uint32_t i = start; i < end; ++i) {
                const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
                const float c[3] = {p.c[0][i], p.c[1][i], p.c[2][i]};
                box_add(bounds, lo, hi);
                box_add(cb, c, c);
            }
            axis = box_max_extent(cb);
            const float cl = pick3(cb.lo, axis), ch = pick3(cb.hi, axis);
            const float* ca = pick3(p.c, axis);
            if (ch == cl) {
                leaf = true;
            } else {
                bool fallback = prm.method == YK_SPLIT_EQUAL_COUNTS;
                int best = 0;
                if (prm.method == YK_SPLIT_SAH) {
                    if (n <= 2) {
                        fallback = true;
                    } else {
                        uint32_t counts[kBuckets];
                        Box boxes[kBuckets];
                        for (int b = 0; b < kBuckets; ++b) {
                            counts[b] = 0;
                            boxes[b] = box_empty();
                        }
                        for (uint32_t i = start; i < end; ++i) {
                            const int b = sah_bucket(cl, ch, ca[i]);
                            const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
                            counts[b] += 1;
                            box_add(boxes[b], lo, hi);
                        }
                        best = sah_choose(counts, boxes, bounds, n);
                        if (best < 0) leaf = true;
                    }
                }
                if (!leaf && !fallback) {  // swap_partition as it stands
                    const float mid_value = (cl + ch) / 2.0f;
                    const bool sah = prm.method == YK_SPLIT_SAH;
                    uint32_t count = 0, front = start, back = end;
                    while (front < back) {
                        const uint32_t f = front++;
                        if (!(sah ? sah_bucket(cl, ch, ca[f]) <= best : ca[f] < mid_value)) {
                            bool swapped = false;
                            while (front < back) {
                                const uint32_t b = --back;
                                if (sah ? sah_bucket(cl, ch, ca[b]) <= best : ca[b] < mid_value) {
                                    prim_swap(p, f, b);
                                    swapped = true;
                                    break;
                                }
                            }
                            if (!swapped) break;
                        }
                        ++count;
                    }
                    mid = start + count;
                    if (mid == start || mid == end) fallback = true;
                }
                if (!leaf && fallback) {  // split_equal_counts
                    mid = (start + end) / 2;
                    select_nth(p, start, end, mid, axis);
                    if (mid == start) {
                        st.split_failed = 1;
                        leaf = true;
                    }
                }
            }
        }
        if (leaf) {
            write_leaf(slots, slot_depth, p, cur);
            if (n > st.max_leaf) st.max_leaf = n;
            if (top == kNone) return;
            const uint32_t* w = slots + 8 * (size_t)top;
            cur = Range{w[0], w[1], top, w[2]};
            top = w[3];
        } else {
            const uint32_t second = write_interior(slots, slot_depth, cur, mid, axis);
            uint32_t* w = slots + 8 * (size_t)second;
            w[0] = mid;
            w[1] = end;
            w[2] = cur.depth + 1;
            w[3] = top;
            top = second;
            cur = Range{start, mid, cur.slot + 1, cur.depth + 1};
        }
    }
}

// ---- one range of a level ----------------------------------------------------------------------------
// Run by a whole block on the device and by the calling thread in the host instance; `Exec` is what
// differs between the two (yk_bvh_build.hip): its lane id and count, a barrier, an all-reduce of
// boxes and counts, an exclusive scan of a flag over the lanes, and a counter increment.
struct Shared {  // block-shared scratch the Exec reduces into
    Box box[kBuckets];
    uint32_t cnt[kBuckets];
    int best;
    uint32_t wave_total[16];
    float part[16][kBuckets * 7];
};
struct Queues {
    Range* next;   // ranges of the next level
    Range* small;  // ranges the small-range phase finishes
    Counters* ctr;
};

template <class Exec> YK_HD void push_child(Exec& ex, const Params& prm, const Queues& q, const Range& c) {
    if (c.end - c.start <= prm.small_range)
        q.small[ex.count_up(&q.ctr->n_small)] = c;
    else
        q.next[ex.count_up(&q.ctr->n_next)] = c;
}

template <class Exec> YK_HD void level_range(Exec& ex, const Prims& p, const Params& prm, const Range r, uint32_t* list, uint32_t* slots, uint32_t* slot_depth, const Queues& q) {
    const uint32_t start = r.start, end = r.end, n = end - start;
    Shared& sh = *ex.sh;
    {  // range bounds and centroid bounds
        Box b[2] = {box_empty(), box_empty()};
        uint32_t none[2] = {0u, 0u};
        for (uint32_t i = start + ex.tid; i < end; i += ex.nt) {
            const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
            const float c[3] = {p.c[0][i], p.c[1][i], p.c[2][i]};
            box_add(b[0], lo, hi);
            box_add(b[1], c, c);
        }
        ex.template all_reduce<2>(b, none);
    }
    const Box bounds = sh.box[0], cb = sh.box[1];
    ex.sync();  // sh.box is reused below
    bool leaf = n <= prm.max_shapes;
    const int axis = box_max_extent(cb);
    const float cl = pick3(cb.lo, axis), ch = pick3(cb.hi, axis);
    const float* ca = pick3(p.c, axis);
    if (!leaf && ch == cl) leaf = true;
    bool fallback = false;
    int best = 0;
    uint32_t mid = start;
    if (!leaf && prm.method == YK_SPLIT_SAH) {
        if (n <= 2) {
            fallback = true;
        } else {
            Box bx[kBuckets];
            uint32_t cnt[kBuckets];
#pragma unroll
            for (int k = 0; k < kBuckets; ++k) {
                bx[k] = box_empty();
                cnt[k] = 0u;
            }
            for (uint32_t i = start + ex.tid; i < end; i += ex.nt) {
                const int bk = sah_bucket(cl, ch, ca[i]);
                const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
#pragma unroll
                for (int k = 0; k < kBuckets; ++k)  // constant indices: the accumulators stay in registers
                    if (bk == k) {
                        cnt[k] += 1u;
                        box_add(bx[k], lo, hi);
                    }
            }
            ex.template all_reduce<kBuckets>(bx, cnt);
            if (ex.tid == 0) sh.best = sah_choose(sh.cnt, sh.box, bounds, n);
            ex.sync();
            best = sh.best;
            ex.sync();
            if (best < 0) leaf = true;
        }
    }
    if (!leaf && !fallback) {  // the partition, in closed form
        const float mid_value = (cl + ch) / 2.0f;
        const bool sah = prm.method == YK_SPLIT_SAH;
        uint32_t n_pass = 0;
        for (uint32_t base = start; base < end; base += ex.nt) {
            const uint32_t i = base + ex.tid;
            const bool in = i < end;
            bool pass = false;
            if (in) pass = sah ? sah_bucket(cl, ch, ca[i]) <= best : ca[i] < mid_value;
            uint32_t total;
            const uint32_t before = n_pass + ex.scan(pass, total);
            if (in) list[part_list_slot(start, end, i, pass, before)] = i;
            n_pass += total;
        }
        mid = start + n_pass;
        if (mid == start || mid == end) {
            fallback = true;  // one side empty: nothing would move
        } else {
            ex.sync_memory();
            const uint32_t pairs = n_pass < n - n_pass ? n_pass : n - n_pass;
            for (uint32_t k = ex.tid; k < pairs; k += ex.nt) {
                uint32_t f, t;
                if (part_swap_pair(list, start, end, n_pass, k, f, t)) prim_swap(p, f, t);
            }
            ex.sync_memory();
        }
    }
    if (!leaf && fallback) {  // split_equal_counts: one lane, short ranges only
        const uint32_t limit = prm.small_range > 2u ? prm.small_range : 2u;
        if (n > limit) {
            if (ex.tid == 0) q.ctr->reason = YK_BVH_REASON_SELECT_NTH;  // the caller abandons this build
            return;
        }
        mid = (start + end) / 2;
        if (ex.tid == 0) select_nth(p, start, end, mid, axis);
        ex.sync_memory();
        if (mid == start) {
            if (ex.tid == 0) q.ctr->split_failed = 1u;
            leaf = true;
        }
    }
    if (ex.tid != 0) return;
    ex.max_up(&q.ctr->max_depth, r.depth);
    if (leaf) {
        write_leaf(slots, slot_depth, p, r);
        ex.max_up(&q.ctr->max_leaf, n);
        return;
    }
    const uint32_t second = write_interior(slots, slot_depth, r, mid, axis);
    push_child(ex, prm, q, Range{start, mid, r.slot + 1u, r.depth + 1u});
    push_child(ex, prm, q, Range{mid, end, second, r.depth + 1u});
}

// Bottom-up step of the layout: an interior node's box from its two children, in child order.
YK_HD void interior_bounds(uint32_t* nodes, uint32_t i) {
    uint32_t* w = nodes + 8 * (size_t)i;
    const uint32_t* a = nodes + 8 * (size_t)(i + 1u);
    const uint32_t* b = nodes + 8 * (size_t)w[6];
    for (int k = 0; k < 3; ++k) {  // BVHBuildNode::interior: child0.bounds.union_b(child1.bounds)
        w[k] = f2u(rmin(u2f(a[k]), u2f(b[k])));
        w[3 + k] = f2u(rmax(u2f(a[k + 3]), u2f(b[k + 3])));
    }
}

}  // namespace lv
}  // namespace yk
