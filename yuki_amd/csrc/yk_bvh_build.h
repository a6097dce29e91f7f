// yk_bvh_build.h — how a BVH is built, written once for every builder: the host recursion (yk_host.cpp,
// Builder::build), the single-lane finisher (build_serial) and the block-per-range step (level_range) of the
// level-synchronous builder (yk_bvh_build.hip: its gfx950 kernels and their host instance).  One function,
// split_range, decides how a range splits; the builders differ only in the steps they hand it.  The yardstick
// is none of them: it is the oracle's sequential builder (oracle/obvh.h), to which tests/test_host_parity.py,
// tests/test_bvh_levels.py and tests/test_gpu_bvh_build.py pin every builder byte for byte.
//
// Shape of the level-synchronous build
//   * The primitive array is SoA (Prims).  Open ranges [start, end) of it are worked level by level
//     (level_range): bounds, centroid bounds, split decision, partition — on the device by one block
//     of 8 waves per range.  A range of at most
//     `small_range` shapes is finished by ONE lane running the recursion with its pending
//     right children chained through the node slots themselves (build_serial): no local stack.
//   * Node slots: the node of range [s, e) at slot p owns slots [p, p + 2(e-s) - 1); its first child
//     sits at p + 1, its second at p + 2(mid - s).  Slots are disjoint by construction and their
//     order IS the depth-first order, so the final numbering is a compaction of the used slots.
//   * Interior bounds are not the range reduction: they are child_union of the two children's boxes
//     in child order, filled in bottom-up after the compaction.
//
// Which reductions must keep the fold's order.  rmin / rmax keep the LEFT operand on a tie, and the
// only tie between different bit patterns is +0 / -0 (non-finite input never reaches the level builder).
// The sign of a zero can reach the result only through a LEAF's stored box: centroid bounds, SAH
// bucket boxes and the range bounds of a split node feed differences, areas and comparisons, where
// +0 and -0 act alike (the cost is `1 + x`, the bucket index `(int)max(12 o, 0)`, the middle
// `(lo + hi) / 2` is compared only).  So the parallel reductions are free in their order, and every
// leaf box of the level builder is folded by one lane from left to right.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/yuki_hip.h"
#include "yk_math.h"

namespace yk {
namespace lv {

struct Prims {  // SoA primitive array: bounds, "centroid" (prim_from_bound), shape id
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

// A primitive from a shape bound: its "centroid" p_min + diagonal / 0.5 (sic, bvh.rs:56), and whether
// bound and centroid are all finite.
YK_HD bool prim_from_bound(const float* lo, const float* hi, float* c) {
    bool finite = true;
    for (int k = 0; k < 3; ++k) {
        c[k] = lo[k] + ((hi[k] - lo[k]) / 0.5f);
        finite = finite && fabsf(lo[k]) <= 3.40282347e+38f && fabsf(hi[k]) <= 3.40282347e+38f && fabsf(c[k]) <= 3.40282347e+38f;
    }
    return finite;
}

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
// An interior node's box, BVHBuildNode::interior: child0.bounds.union_b(child1.bounds)
YK_HD Box child_union(const float* lo0, const float* hi0, const float* lo1, const float* hi1) {
    Box b = {{lo0[0], lo0[1], lo0[2]}, {hi0[0], hi0[1], hi0[2]}};
    box_add(b, lo1, hi1);
    return b;
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
// SAH bucket of a centroid coordinate: impl_bounds.rs offset() then `(12*o).max(0) as usize`
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
// The cost loop of split_sah: the bucket to split after, or -1 when a leaf is cheaper.
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
// Which side of a split a primitive goes to, by its centroid coordinate on the split axis: true = first child.
struct Pass {
    bool sah;  // SAH: buckets up to `best`; Middle: below the middle of the centroid bounds
    float cl, ch, mid_value;
    int best;
    YK_HD bool operator()(float c) const { return sah ? sah_bucket(cl, ch, c) <= best : c < mid_value; }
};

// ---- a primitive array with a key and a swap -------------------------------------------------------
// select_nth and the partitions see an array `a` through a.key(i) and a.swap(i, j): SoaKeys here, the host
// recursion's array of structs in yk_host.cpp.
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
struct SoaKeys {
    const Prims& p;
    const float* c;  // p.c[axis]
    YK_HD SoaKeys(const Prims& prims, int axis) : p(prims), c(pick3(prims.c, axis)) {}
    YK_HD float key(uint32_t i) const { return c[i]; }
    YK_HD void swap(uint32_t i, uint32_t j) const { prim_swap(p, i, j); }
};

// "select_nth spec" (DESIGN.md): 3-way quickselect, middle pivot, on the key
template <class A, class I> YK_HD void select_nth(const A& a, I lo, I hi, I k) {
    while (hi - lo > 1) {
        const float pivot = a.key(lo + (hi - lo) / 2);
        I i = lo, lt = lo, gt = hi;
        while (i < gt) {
            const float v = a.key(i);
            if (v < pivot) {
                if (lt != i) a.swap(lt, i);
                ++lt;
                ++i;
            } else if (v > pivot) {
                --gt;
                if (i != gt) a.swap(i, gt);
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

// The two-ended swap partition (the algorithm of itertools::partition): elements whose key passes come
// first; returns the position of the first one that fails.
template <class A, class I, class Pred> YK_HD I swap_partition(const A& a, I lo, I hi, const Pred& pass) {
    I count = 0, front = lo, back = hi;
    while (front < back) {
        const I f = front++;
        if (!pass(a.key(f))) {
            bool swapped = false;
            while (front < back) {
                const I b = --back;
                if (pass(a.key(b))) {
                    a.swap(f, b);
                    swapped = true;
                    break;
                }
            }
            if (!swapped) break;
        }
        ++count;
    }
    return lo + count;
}

// ---- the two-ended swap partition in closed form, run by a block ----------------------------------
// swap_partition leaves this arrangement: with
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
// `Exec` is what differs between the device block and the calling thread of the host instance
// (yk_bvh_build.hip): see level_range.  `list` holds one word per element of the array.
template <class Exec, class A, class Pred> YK_HD uint32_t block_partition(Exec& ex, const A& a, uint32_t* list, uint32_t start, uint32_t end, const Pred& pass) {
    const uint32_t n = end - start;
    uint32_t n_pass = 0;
    for (uint32_t base = start; base < end; base += ex.nt) {
        const uint32_t i = base + ex.tid;
        const bool in = i < end;
        bool flag = false;
        if (in) flag = pass(a.key(i));
        uint32_t total;
        const uint32_t before = n_pass + ex.scan(flag, total);
        if (in) list[part_list_slot(start, end, i, flag, before)] = i;
        n_pass += total;
    }
    const uint32_t mid = start + n_pass;
    if (mid != start && mid != end) {  // one side empty: nothing would move
        ex.sync_memory();
        const uint32_t pairs = n_pass < n - n_pass ? n_pass : n - n_pass;
        for (uint32_t k = ex.tid; k < pairs; k += ex.nt) {
            uint32_t f, t;
            if (part_swap_pair(list, start, end, n_pass, k, f, t)) a.swap(f, t);
        }
        ex.sync_memory();
    }
    return mid;
}

// ---- the split rule ----------------------------------------------------------------------------------
// How the range [start, end) splits (bvh.rs:305-420), for every builder.  `Steps` is what differs between them:
//   reduce(start, end, bounds, cb)                 the range's bounds and centroid bounds
//   sah_best(start, end, axis, cl, ch, bounds)     fills the twelve buckets and returns sah_choose of them
//   partition(start, end, axis, pass)              primitives whose centroid passes first; returns the middle
//   select_nth(start, end, mid, axis)              false: refused, the build is abandoned
// A block runs this in lockstep on every lane: all its inputs are block-uniform.
template <class I> struct Split {
    bool leaf, split_failed, refused;
    I mid;
    int axis;
    Box bounds;  // of the range, where it holds more than max_shapes shapes
};
template <class I, class Steps> YK_HD Split<I> split_range(Steps& s, uint32_t max_shapes, uint32_t method, I start, I end) {
    Split<I> r = {true, false, false, start, 0, box_empty()};
    const I n = end - start;
    if (n <= max_shapes) return r;
    Box cb;
    s.reduce(start, end, r.bounds, cb);
    const int axis = r.axis = box_max_extent(cb);
    const float cl = pick3(cb.lo, axis), ch = pick3(cb.hi, axis);
    if (ch == cl) return r;  // a degenerate centroid box
    bool equal_counts = method != YK_SPLIT_SAH && method != YK_SPLIT_MIDDLE;
    if (!equal_counts) {
        Pass pass = {method == YK_SPLIT_SAH, cl, ch, (cl + ch) / 2.0f, 0};
        if (pass.sah && n <= 2) {
            equal_counts = true;
        } else {
            if (pass.sah) {
                pass.best = s.sah_best(start, end, axis, cl, ch, r.bounds);
                if (pass.best < 0) return r;  // a leaf is cheaper
            }
            r.mid = s.partition(start, end, axis, pass);
            equal_counts = r.mid == start || r.mid == end;  // an empty side
        }
    }
    if (equal_counts) {  // split_equal_counts
        r.mid = (start + end) / 2;
        if (!s.select_nth(start, end, r.mid, axis)) {
            r.refused = true;
            return r;
        }
        if (r.mid == start) {
            r.split_failed = true;
            return r;
        }
    }
    r.leaf = false;
    return r;
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

// ---- one lane finishes a range -----------------------------------------------------------------------
struct SerialSteps {
    const Prims& p;
    YK_HD void reduce(uint32_t start, uint32_t end, Box& bounds, Box& cb) const {
        bounds = box_empty();
        cb = box_empty();
        for (uint32_t i = start; i < end; ++i) {
            const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
            const float c[3] = {p.c[0][i], p.c[1][i], p.c[2][i]};
            box_add(bounds, lo, hi);
            box_add(cb, c, c);
        }
    }
    YK_HD int sah_best(uint32_t start, uint32_t end, int axis, float cl, float ch, const Box& bounds) const {
        const float* ca = pick3(p.c, axis);
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
        return sah_choose(counts, boxes, bounds, end - start);
    }
    YK_HD uint32_t partition(uint32_t start, uint32_t end, int axis, const Pass& pass) const { return swap_partition(SoaKeys(p, axis), start, end, pass); }
    YK_HD bool select_nth(uint32_t start, uint32_t end, uint32_t mid, int axis) const {
        lv::select_nth(SoaKeys(p, axis), start, end, mid);
        return true;
    }
};
struct SerialStats {
    uint32_t max_depth, max_leaf, split_failed;
};

// The recursion with an explicit stack.  A pending second child is
// parked in its own (still unused) slot — {start, end, depth, previous pending slot} — so the stack
// needs no storage of its own and no bound on its depth.
YK_HD void build_serial(const Prims& p, const Params& prm, Range cur, uint32_t* slots, uint32_t* slot_depth, SerialStats& st) {
    SerialSteps steps = {p};
    uint32_t top = kNone;
    for (;;) {
        if (cur.depth > st.max_depth) st.max_depth = cur.depth;
        const Split<uint32_t> s = split_range(steps, prm.max_shapes, prm.method, cur.start, cur.end);
        if (s.split_failed) st.split_failed = 1;
        if (s.leaf) {
            write_leaf(slots, slot_depth, p, cur);
            if (cur.end - cur.start > st.max_leaf) st.max_leaf = cur.end - cur.start;
            if (top == kNone) return;
            const uint32_t* w = slots + 8 * (size_t)top;
            cur = Range{w[0], w[1], top, w[2]};
            top = w[3];
        } else {
            const uint32_t second = write_interior(slots, slot_depth, cur, s.mid, s.axis);
            uint32_t* w = slots + 8 * (size_t)second;
            w[0] = s.mid;
            w[1] = cur.end;
            w[2] = cur.depth + 1;
            w[3] = top;
            top = second;
            cur = Range{cur.start, s.mid, cur.slot + 1, cur.depth + 1};
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

template <class Exec> struct BlockSteps {
    Exec& ex;
    const Prims& p;
    uint32_t* list;
    uint32_t select_limit;  // select_nth runs on one lane: short ranges only
    YK_HD void reduce(uint32_t start, uint32_t end, Box& bounds, Box& cb) const {
        Box b[2] = {box_empty(), box_empty()};
        uint32_t none[2] = {0u, 0u};
        for (uint32_t i = start + ex.tid; i < end; i += ex.nt) {
            const float lo[3] = {p.bmin[0][i], p.bmin[1][i], p.bmin[2][i]}, hi[3] = {p.bmax[0][i], p.bmax[1][i], p.bmax[2][i]};
            const float c[3] = {p.c[0][i], p.c[1][i], p.c[2][i]};
            box_add(b[0], lo, hi);
            box_add(b[1], c, c);
        }
        ex.template all_reduce<2>(b, none);
        bounds = ex.sh->box[0];
        cb = ex.sh->box[1];
        ex.sync();  // sh->box is reused by sah_best
    }
    YK_HD int sah_best(uint32_t start, uint32_t end, int axis, float cl, float ch, const Box& bounds) const {
        const float* ca = pick3(p.c, axis);
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
        if (ex.tid == 0) ex.sh->best = sah_choose(ex.sh->cnt, ex.sh->box, bounds, end - start);
        ex.sync();
        const int best = ex.sh->best;
        ex.sync();
        return best;
    }
    YK_HD uint32_t partition(uint32_t start, uint32_t end, int axis, const Pass& pass) const { return block_partition(ex, SoaKeys(p, axis), list, start, end, pass); }
    YK_HD bool select_nth(uint32_t start, uint32_t end, uint32_t mid, int axis) const {
        if (end - start > select_limit) return false;
        if (ex.tid == 0) lv::select_nth(SoaKeys(p, axis), start, end, mid);
        ex.sync_memory();
        return true;
    }
};

template <class Exec> YK_HD void push_child(Exec& ex, const Params& prm, const Queues& q, const Range& c) {
    if (c.end - c.start <= prm.small_range)
        q.small[ex.count_up(&q.ctr->n_small)] = c;
    else
        q.next[ex.count_up(&q.ctr->n_next)] = c;
}

template <class Exec> YK_HD void level_range(Exec& ex, const Prims& p, const Params& prm, const Range r, uint32_t* list, uint32_t* slots, uint32_t* slot_depth, const Queues& q) {
    BlockSteps<Exec> steps = {ex, p, list, prm.small_range > 2u ? prm.small_range : 2u};
    const Split<uint32_t> s = split_range(steps, prm.max_shapes, prm.method, r.start, r.end);
    if (ex.tid != 0) return;
    if (s.refused) {
        q.ctr->reason = YK_BVH_REASON_SELECT_NTH;  // the caller abandons this build
        return;
    }
    if (s.split_failed) q.ctr->split_failed = 1u;
    ex.max_up(&q.ctr->max_depth, r.depth);
    if (s.leaf) {
        write_leaf(slots, slot_depth, p, r);
        ex.max_up(&q.ctr->max_leaf, r.end - r.start);
        return;
    }
    const uint32_t second = write_interior(slots, slot_depth, r, s.mid, s.axis);
    push_child(ex, prm, q, Range{r.start, s.mid, r.slot + 1u, r.depth + 1u});
    push_child(ex, prm, q, Range{s.mid, r.end, second, r.depth + 1u});
}

// Bottom-up step of the layout: an interior node's box from its two children, in child order.
YK_HD void interior_bounds(uint32_t* nodes, uint32_t i) {
    uint32_t* w = nodes + 8 * (size_t)i;
    const uint32_t* a = nodes + 8 * (size_t)(i + 1u);
    const uint32_t* b = nodes + 8 * (size_t)w[6];
    float fa[6], fb[6];
    for (int k = 0; k < 6; ++k) {
        fa[k] = u2f(a[k]);
        fb[k] = u2f(b[k]);
    }
    const Box u = child_union(fa, fa + 3, fb, fb + 3);
    for (int k = 0; k < 3; ++k) {
        w[k] = f2u(u.lo[k]);
        w[3 + k] = f2u(u.hi[k]);
    }
}

}  // namespace lv
}  // namespace yk
