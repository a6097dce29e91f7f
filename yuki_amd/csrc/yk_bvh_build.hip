// yk_bvh_build.hip — the level-synchronous BVH builder (yk_bvh_build.h): its gfx950 kernels and driver
// (build_bvh_device) and the host instance of the same algorithm (build_bvh_levels).  Both return the
// one tree that every builder builds (yk_bvh_build.h) or refuse with a reason; neither changes `out` when it refuses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "yk_bvh_build.h"
#include "yk_internal.h"
#include "yk_scan.h"

using namespace yk::lv;
using namespace yk::scan;

namespace {

const int kLevelThreads = 512;  // one block per open range

// ------------------------------------------------------------------ the two executors of level_range
struct HostExec {
    uint32_t tid = 0, nt = 1;
    Shared* sh = nullptr;
    void sync() {}
    void sync_memory() {}
    template <int NB> void all_reduce(Box (&b)[NB], uint32_t (&cnt)[NB]) {
        for (int k = 0; k < NB; ++k) {
            sh->box[k] = b[k];
            sh->cnt[k] = cnt[k];
        }
    }
    uint32_t scan(bool flag, uint32_t& total) {
        total = flag ? 1u : 0u;
        return 0u;
    }
    uint32_t count_up(uint32_t* p) { return (*p)++; }
    void max_up(uint32_t* p, uint32_t v) {
        if (v > *p) *p = v;
    }
};

struct DevExec {
    uint32_t tid, nt;
    Shared* sh;
    __device__ void sync() { __syncthreads(); }
    __device__ void sync_memory() {
        __threadfence_block();
        __syncthreads();
    }
    // min / max / sum over the block; the results land in sh->box / sh->cnt.  Free in its order (yk_bvh_build.h).
    template <int NB> __device__ void all_reduce(Box (&b)[NB], uint32_t (&cnt)[NB]) {
        const uint32_t lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float lo = b[k].lo[j], hi = b[k].hi[j];
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    lo = fminf(lo, __shfl_xor(lo, off));
                    hi = fmaxf(hi, __shfl_xor(hi, off));
                }
                if (lane == 0) {
                    sh->part[wave][k * 7 + j] = lo;
                    sh->part[wave][k * 7 + 3 + j] = hi;
                }
            }
            uint32_t c = cnt[k];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0) sh->part[wave][k * 7 + 6] = u2f(c);
        }
        __syncthreads();
        for (uint32_t v = tid; v < (uint32_t)(NB * 7); v += nt) {  // one value each: box k, word j of {lo[3], hi[3], count}
            const uint32_t k = v / 7u, j = v % 7u;
            if (j == 6u) {
                uint32_t c = 0u;
                for (uint32_t w = 0; w < nw; ++w) c += f2u(sh->part[w][v]);
                sh->cnt[k] = c;
            } else if (j < 3u) {
                float x = sh->part[0][v];
                for (uint32_t w = 1; w < nw; ++w) x = fminf(x, sh->part[w][v]);
                sh->box[k].lo[j] = x;
            } else {
                float x = sh->part[0][v];
                for (uint32_t w = 1; w < nw; ++w) x = fmaxf(x, sh->part[w][v]);
                sh->box[k].hi[j - 3u] = x;
            }
        }
        __syncthreads();
    }
    __device__ uint32_t scan(bool flag, uint32_t& total) {
        const uint32_t lane = tid & 63u, wave = tid >> 6, nw = nt >> 6;
        const unsigned long long m = __ballot(flag);
        if (lane == 0) sh->wave_total[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), all = 0u;
        for (uint32_t w = 0; w < nw; ++w) {
            const uint32_t t = sh->wave_total[w];
            if (w < wave) before += t;
            all += t;
        }
        __syncthreads();
        total = all;
        return before;
    }
    __device__ uint32_t count_up(uint32_t* p) { return atomicAdd(p, 1u); }
    __device__ void max_up(uint32_t* p, uint32_t v) { atomicMax(p, v); }
};

// ------------------------------------------------------------------ kernels
// shape bounds (6 floats each) -> the SoA primitive array; flags a non-finite bound or centroid
__global__ void k_prepare(const float* __restrict__ sb, uint32_t n, Prims p, uint32_t* bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* b = sb + 6 * (size_t)i;
    const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
    float c[3];
    const bool ok = prim_from_bound(lo, hi, c);
    for (int k = 0; k < 3; ++k) {
        p.bmin[k][i] = lo[k];
        p.bmax[k][i] = hi[k];
        p.c[k][i] = c[k];
    }
    p.shape[i] = i;
    if (!ok) *bad = 1u;
}

__global__ void __launch_bounds__(kLevelThreads) k_level(Prims p, Params prm, const Range* __restrict__ cur, uint32_t* list, uint32_t* slots, uint32_t* slot_depth, Queues q) {
    __shared__ Shared sh;
    DevExec ex{threadIdx.x, blockDim.x, &sh};
    level_range(ex, p, prm, cur[blockIdx.x], list, slots, slot_depth, q);
}

// one lane per small range
__global__ void __launch_bounds__(64) k_small(Prims p, Params prm, const Range* __restrict__ jobs, uint32_t n_jobs, uint32_t* slots, uint32_t* slot_depth, Counters* ctr) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    SerialStats st = {0u, 0u, 0u};
    build_serial(p, prm, jobs[j], slots, slot_depth, st);
    atomicMax(&ctr->max_depth, st.max_depth);
    atomicMax(&ctr->max_leaf, st.max_leaf);
    if (st.split_failed) ctr->split_failed = 1u;
}

// the compaction's scan (yk_scan.h) counts the used slots
struct SlotUsed {
    const uint32_t* __restrict__ slot_depth;
    __device__ uint32_t operator()(uint32_t s) const { return slot_depth[s] != 0u ? 1u : 0u; }
};
// slots -> the depth-first node array: second-child slots become node indices
__global__ void k_compact(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_depth, uint32_t n_slots, const uint32_t* __restrict__ index, const uint32_t* __restrict__ bsum, uint32_t* nodes,
                          uint32_t* depth) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots || slot_depth[s] == 0u) return;
    const uint32_t i = scan_rank(index, bsum, s);
    const uint4* src = reinterpret_cast<const uint4*>(slots + 8 * (size_t)s);
    uint4 a = src[0], b = src[1];
    if ((b.w >> 24) == 0u) b.z = scan_rank(index, bsum, b.z);
    uint4* dst = reinterpret_cast<uint4*>(nodes + 8 * (size_t)i);
    dst[0] = a;
    dst[1] = b;
    depth[i] = slot_depth[s];
}
__global__ void k_interior_bounds(uint32_t* nodes, const uint32_t* __restrict__ depth, uint32_t n_nodes, uint32_t d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes || depth[i] != d || (nodes[8 * (size_t)i + 7] >> 24) != 0u) return;
    interior_bounds(nodes, i);
}

bool refuse(yk_bvh_build_info& bi, uint32_t reason) {
    bi.reason = reason;
    return false;
}

void words_to_nodes(const uint32_t* w, size_t n, std::vector<yk_bvh_node>& out) {
    out.resize(n);
    static_assert(sizeof(yk_bvh_node) == 32, "a node slot is 8 words");
    if (n) std::memcpy(out.data(), w, n * 32);
}

}  // namespace

// ------------------------------------------------------------------ the device builder
bool build_bvh_device(yk_context* ctx, const std::vector<ShapeBounds>& sb, uint32_t max_shapes, uint32_t method, uint32_t small_range, HostBvh& out, yk_bvh_build_info& bi, DeviceTree* keep) {
    return build_bvh_device(ctx, sb.data(), nullptr, sb.size(), max_shapes, method, small_range, out, bi, keep);
}

// The builder proper.  The bounds (six floats a shape) come from the host (h_sb) or are in HBM already (d_bounds, written
// on the context's stream or ordered before it): then nothing is uploaded.
bool build_bvh_device(yk_context* ctx, const ShapeBounds* h_sb, const float* d_bounds, size_t n_bounds, uint32_t max_shapes, uint32_t method, uint32_t small_range, HostBvh& out, yk_bvh_build_info& bi,
                      DeviceTree* keep) {
    bi.small_range = small_range;
    if (method != YK_SPLIT_SAH && method != YK_SPLIT_MIDDLE) return refuse(bi, YK_BVH_REASON_SPLIT_METHOD);
    if (n_bounds == 0 || n_bounds > ((size_t)1 << 28)) return refuse(bi, YK_BVH_REASON_TOO_MANY_NODES);
    const uint32_t N = (uint32_t)n_bounds, n_slots = 2u * N;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    DevScratch mem;
    float *d_sb = nullptr, *d_soa = nullptr;
    uint32_t *d_shape = nullptr, *d_list = nullptr, *d_slots = nullptr, *d_slot_depth = nullptr, *d_index = nullptr, *d_bsum = nullptr, *d_nodes = nullptr, *d_depth = nullptr, *d_words = nullptr;
    Range *d_q[2] = {nullptr, nullptr}, *d_small = nullptr;
    if ((!d_bounds && !mem.get(d_sb, 6 * (size_t)N)) || !mem.get(d_soa, 9 * (size_t)N) || !mem.get(d_shape, N) || !mem.get(d_list, N) || !mem.get(d_slots, 8 * (size_t)n_slots) || !mem.get(d_slot_depth, n_slots) ||
        !mem.get(d_index, n_slots) || !mem.get(d_bsum, scan_blocks(n_slots)) || !mem.get(d_nodes, 8 * (size_t)n_slots) || !mem.get(d_depth, n_slots) || !mem.get(d_words, 16) || !mem.get(d_q[0], N) || !mem.get(d_q[1], N) ||
        !mem.get(d_small, N))
        return refuse(bi, YK_BVH_REASON_OUT_OF_MEMORY);
    Counters* d_ctr = reinterpret_cast<Counters*>(d_words);  // 8 words; word 8: non-finite flag; word 9: node count
    Prims p;
    for (int k = 0; k < 3; ++k) {
        p.bmin[k] = d_soa + (size_t)k * N;
        p.bmax[k] = d_soa + (size_t)(3 + k) * N;
        p.c[k] = d_soa + (size_t)(6 + k) * N;
    }
    p.shape = d_shape;
    const Params prm = {max_shapes, method, small_range};
#define DEV_TRY(expr)                                        \
    if ((expr) != hipSuccess) {                              \
        (void)hipGetLastError();                             \
        (void)hipStreamSynchronize(st);                      \
        return refuse(bi, YK_BVH_REASON_DEVICE_ERROR);       \
    }
    double t0 = now_seconds();
    uint32_t words[16];
    if (!d_bounds) {
        DEV_TRY(hipMemcpyAsync(d_sb, h_sb, 6 * (size_t)N * sizeof(float), hipMemcpyHostToDevice, st));
    }
    DEV_TRY(hipMemsetAsync(d_words, 0, 16 * sizeof(uint32_t), st));
    DEV_TRY(hipMemsetAsync(d_slot_depth, 0, (size_t)n_slots * sizeof(uint32_t), st));
    k_prepare<<<(N + 255) / 256, 256, 0, st>>>(d_bounds ? d_bounds : d_sb, N, p, d_words + 8);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    bi.seconds_upload = now_seconds() - t0;
    if (words[8]) return refuse(bi, YK_BVH_REASON_NON_FINITE);

    // ---- level phase
    t0 = now_seconds();
    const Range root = {0u, N, 0u, 1u};
    uint32_t n_cur = 0, n_small = 0, levels = 0;
    int cur = 0;
    if (N <= small_range) {
        DEV_TRY(hipMemcpyAsync(d_small, &root, sizeof(root), hipMemcpyHostToDevice, st));
        n_small = 1;
        words[1] = 1u;
        DEV_TRY(hipMemcpyAsync(&d_ctr->n_small, &words[1], 4, hipMemcpyHostToDevice, st));
    } else {
        DEV_TRY(hipMemcpyAsync(d_q[0], &root, sizeof(root), hipMemcpyHostToDevice, st));
        n_cur = 1;
    }
    Counters ctr;
    std::memset(&ctr, 0, sizeof(ctr));
    while (n_cur) {
        const Queues q = {d_q[cur ^ 1], d_small, d_ctr};
        DEV_TRY(hipMemsetAsync(&d_ctr->n_next, 0, 4, st));
        k_level<<<n_cur, kLevelThreads, 0, st>>>(p, prm, d_q[cur], d_list, d_slots, d_slot_depth, q);
        DEV_TRY(hipGetLastError());
        DEV_TRY(hipMemcpyAsync(&ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
        DEV_TRY(hipStreamSynchronize(st));
        ++levels;
        if (ctr.reason) return refuse(bi, ctr.reason);
        n_cur = ctr.n_next;
        n_small = ctr.n_small;
        cur ^= 1;
    }
    bi.levels = levels;
    bi.seconds_levels = now_seconds() - t0;

    // ---- small-range phase
    t0 = now_seconds();
    if (n_small) {
        k_small<<<(n_small + 63) / 64, 64, 0, st>>>(p, prm, d_small, n_small, d_slots, d_slot_depth, d_ctr);
        DEV_TRY(hipGetLastError());
    }
    DEV_TRY(hipMemcpyAsync(&ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    bi.small_ranges = n_small;
    bi.seconds_small = now_seconds() - t0;

    // ---- depth-first layout: compaction of the used slots, then the interior boxes bottom-up
    t0 = now_seconds();
    enqueue_scan(st, SlotUsed{d_slot_depth}, n_slots, d_index, d_bsum, d_words + 9, false);  // k_compact folds the block sums in itself
    k_compact<<<(n_slots + 255) / 256, 256, 0, st>>>(d_slots, d_slot_depth, n_slots, d_index, d_bsum, d_nodes, d_depth);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    const uint32_t n_nodes = words[9];
    if (n_nodes == 0 || n_nodes > YK_REF_INDEX_MAX) return refuse(bi, YK_BVH_REASON_TOO_MANY_NODES);
    for (uint32_t d = ctr.max_depth; d-- > 1u;) k_interior_bounds<<<(n_nodes + 255) / 256, 256, 0, st>>>(d_nodes, d_depth, n_nodes, d);
    DEV_TRY(hipGetLastError());
    DEV_TRY(hipStreamSynchronize(st));
    bi.seconds_layout = now_seconds() - t0;

    // ---- copy back: the arrays, or node 0 alone when the tree stays in HBM for the device layout
    t0 = now_seconds();
    std::vector<yk_bvh_node> nodes(keep ? 0 : n_nodes);
    std::vector<uint32_t> order(keep ? 0 : N);
    if (keep) {
        DEV_TRY(hipMemcpyAsync(keep->root_words, d_nodes, 32, hipMemcpyDeviceToHost, st));
    } else {
        DEV_TRY(hipMemcpyAsync(nodes.data(), d_nodes, (size_t)n_nodes * 32, hipMemcpyDeviceToHost, st));
        DEV_TRY(hipMemcpyAsync(order.data(), d_shape, (size_t)N * 4, hipMemcpyDeviceToHost, st));
    }
    DEV_TRY(hipStreamSynchronize(st));
#undef DEV_TRY
    if (keep) {
        mem.give(d_nodes, 8 * (size_t)n_slots, keep->nodes);
        mem.give(d_depth, n_slots, keep->depth);
        mem.give(d_shape, N, keep->order);
        keep->n_nodes = n_nodes;
        keep->n_shapes = N;
    }
    out.nodes.swap(nodes);
    out.shape_order.swap(order);
    out.max_leaf_shapes = ctr.max_leaf;
    out.depth = ctr.max_depth;
    out.split_failed = ctr.split_failed != 0;
    bi.seconds_copy_back = now_seconds() - t0;
    bi.builder = YK_BVH_BUILDER_DEVICE;
    bi.reason = 0;
    return true;
}

// ------------------------------------------------------------------ the host instance of the level algorithm
bool build_bvh_levels(const std::vector<ShapeBounds>& sb, uint32_t max_shapes, uint32_t method, uint32_t small_range, HostBvh& out, yk_bvh_build_info& bi) {
    bi.small_range = small_range;
    if (method != YK_SPLIT_SAH && method != YK_SPLIT_MIDDLE) return refuse(bi, YK_BVH_REASON_SPLIT_METHOD);
    if (sb.empty() || sb.size() > ((size_t)1 << 28)) return refuse(bi, YK_BVH_REASON_TOO_MANY_NODES);
    const uint32_t N = (uint32_t)sb.size(), n_slots = 2u * N;
    std::vector<float> soa(9 * (size_t)N);
    std::vector<uint32_t> shape(N), list(N), slots(8 * (size_t)n_slots), slot_depth(n_slots, 0u);
    Prims p;
    for (int k = 0; k < 3; ++k) {
        p.bmin[k] = soa.data() + (size_t)k * N;
        p.bmax[k] = soa.data() + (size_t)(3 + k) * N;
        p.c[k] = soa.data() + (size_t)(6 + k) * N;
    }
    p.shape = shape.data();
    for (uint32_t i = 0; i < N; ++i) {
        float c[3];
        if (!prim_from_bound(sb[i].bmin, sb[i].bmax, c)) return refuse(bi, YK_BVH_REASON_NON_FINITE);
        for (int k = 0; k < 3; ++k) {
            p.bmin[k][i] = sb[i].bmin[k];
            p.bmax[k][i] = sb[i].bmax[k];
            p.c[k][i] = c[k];
        }
        shape[i] = i;
    }
    const Params prm = {max_shapes, method, small_range};
    std::vector<Range> qa(N), qb(N), small(N);
    Counters ctr;
    std::memset(&ctr, 0, sizeof(ctr));
    Shared sh;
    HostExec ex;
    ex.sh = &sh;
    uint32_t n_cur = 0, levels = 0;
    Range *cur = qa.data(), *next = qb.data();
    const Range root = {0u, N, 0u, 1u};
    if (N <= small_range)
        small[ctr.n_small++] = root;
    else
        cur[n_cur++] = root;
    while (n_cur) {
        const Queues q = {next, small.data(), &ctr};
        ctr.n_next = 0;
        for (uint32_t r = 0; r < n_cur; ++r) {
            level_range(ex, p, prm, cur[r], list.data(), slots.data(), slot_depth.data(), q);
            if (ctr.reason) return refuse(bi, ctr.reason);
        }
        ++levels;
        n_cur = ctr.n_next;
        std::swap(cur, next);
    }
    for (uint32_t j = 0; j < ctr.n_small; ++j) {
        SerialStats st = {0u, 0u, 0u};
        build_serial(p, prm, small[j], slots.data(), slot_depth.data(), st);
        ctr.max_depth = std::max(ctr.max_depth, st.max_depth);
        ctr.max_leaf = std::max(ctr.max_leaf, st.max_leaf);
        ctr.split_failed |= st.split_failed;
    }
    // layout
    std::vector<uint32_t> index(n_slots);
    uint32_t n_nodes = 0;
    for (uint32_t s = 0; s < n_slots; ++s) {
        index[s] = n_nodes;
        n_nodes += slot_depth[s] != 0u ? 1u : 0u;
    }
    if (n_nodes == 0 || n_nodes > YK_REF_INDEX_MAX) return refuse(bi, YK_BVH_REASON_TOO_MANY_NODES);
    std::vector<uint32_t> nodes(8 * (size_t)n_nodes), depth(n_nodes);
    for (uint32_t s = 0; s < n_slots; ++s) {
        if (!slot_depth[s]) continue;
        uint32_t* w = nodes.data() + 8 * (size_t)index[s];
        std::memcpy(w, slots.data() + 8 * (size_t)s, 32);
        if ((w[7] >> 24) == 0u) w[6] = index[w[6]];
        depth[index[s]] = slot_depth[s];
    }
    std::vector<std::vector<uint32_t>> by_depth(ctr.max_depth + 1);
    for (uint32_t i = 0; i < n_nodes; ++i)
        if ((nodes[8 * (size_t)i + 7] >> 24) == 0u) by_depth[depth[i]].push_back(i);
    for (uint32_t d = ctr.max_depth; d-- > 1u;)
        for (uint32_t i : by_depth[d]) interior_bounds(nodes.data(), i);
    words_to_nodes(nodes.data(), n_nodes, out.nodes);
    out.shape_order.swap(shape);
    out.max_leaf_shapes = ctr.max_leaf;
    out.depth = ctr.max_depth;
    out.split_failed = ctr.split_failed != 0;
    bi.levels = levels;
    bi.small_ranges = ctr.n_small;
    bi.builder = YK_BVH_BUILDER_HOST_LEVELS;
    bi.reason = 0;
    return true;
}

// The block partition on flags given one by one: `order` is the array, its key the flag of the position.
namespace {
struct PlanArray {
    const uint8_t* pass;
    uint32_t* order;
    bool key(uint32_t i) const { return pass[i] != 0; }
    void swap(uint32_t i, uint32_t j) const { std::swap(order[i], order[j]); }
};
}  // namespace
extern "C" size_t yk_bvh_partition_plan(const uint8_t* pass, size_t n, uint32_t* order) {
    if (!pass || !order || n == 0 || n > 0x7fffffffu) return 0;
    std::vector<uint32_t> list(n);
    HostExec ex;
    return block_partition(ex, PlanArray{pass, order}, list.data(), 0u, (uint32_t)n, [](bool passes) { return passes; });
}
