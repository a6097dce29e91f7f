// yk_shade_queue.h — the two parts of `k_shade` (yk_kernels.hip) that are not physics: the sort of a window of paths by
// material kind, and the LDS staging of shadow rays and surviving paths with its flush protocol.  The physics of a vertex
// is yk_shade.h; the kernel strings the three together.
//
// Stream compaction: survivors and shadow rays are first appended to LDS staging
// buffers (wave ballot + one LDS atomic per wave) and flushed to HBM in dense runs
// of >= BLOCK entries with ONE global atomic per flush.  A global atomic per wave
// per append saturated the counter word (~90 M atomics/s, MI355X_MICROARCH.md
// "dequeue") and made this kernel atomic-bound (profiles/r01_a_*: 0.178 s/frame,
// 79 % of wave cycles waiting).
//
// Everything here is called by every thread of the block, converged: the barriers need block-uniform control flow and
// the ballots whole waves.
#pragma once
#include "yk_device.h"
#include "yk_path_state.h"
#include "yk_shade.h"
#include "yk_wave.h"

#ifndef SHADE_CAP
#define SHADE_CAP 335  // staged continuation paths per block (64 B each).  With SHADE_CAPQ, the sort window's order table and the round-3
                       // interruption flag the block's LDS is 53248 B: three blocks per CU (LDS is handed out in 1280-byte granules on gfx950:
                       // 42 granules = 53760 B x 3 fit 160 KB, one granule more does not).  335, not 336: the flag word would have made it
                       // 53312 B — inside the same 42 granules on paper, but only 53248 and 53296 are measured sizes
#endif
#ifndef SHADE_CAPQ
#define SHADE_CAPQ 768  // staged shadow rays per block (36 B each): a whole iteration of 256 paths x 3 lights fits
#endif
#ifndef SHADE_WIN
#define SHADE_WIN 8  // at most this many iterations (of 256 paths) are sorted by material kind together (the launch passes the actual number)
#endif
#ifndef SHADE_MIN_WAVES
#define SHADE_MIN_WAVES 3  // waves per SIMD the register allocator must leave room for (blocks of 256 threads)
#endif

namespace yk {

template <int CAP, int CAPQ> struct ShadeStaging {
    float4 pO[CAP], pD[CAP], pT[CAP];
    uint4 pR[CAP];
    float4 qO[CAPQ], qD[CAPQ];
    unsigned qS[CAPQ];
    unsigned fill_p, fill_q, gbase;
    unsigned q_delta;  // class of the staged shadow rays: 1 = towards a point/spot/distant light
    unsigned cancel;   // the render was interrupted (yk_device.h, CancelRef): block-uniform copy of what thread 0 read
    unsigned untraced;  // shadow rays the block reported without staging them (NeeSample::zero); sits in what was padding: the struct keeps its 53248 bytes
    unsigned bucket[8];                 // material-kind histogram of the window's paths
    unsigned short order[SHADE_WIN * 256];  // sorted position -> offset of the path inside the window
};

// what the launch tells k_shade beside its queues
struct ShadeArgs {
    unsigned split_delta;  // shadow rays towards point / spot / distant lights go to the delta queue
    unsigned reorder;      // sort the windows by material kind
    unsigned win_max;      // iterations per window at most (<= SHADE_WIN)
    unsigned block_slots;  // resident blocks on the device
    unsigned sid_base;     // first sample slot of the batch
    unsigned long long* shadow_counter;  // the batch's count of reported shadow rays (the word queue_length adds the any-hit queues to)
};

// returns the staging position of the lanes that `want` one
__device__ __forceinline__ unsigned block_append(bool want, unsigned* lds_fill) {
    unsigned long long mask = __ballot(want);
    unsigned total = (unsigned)__popcll(mask);
    unsigned prefix = (unsigned)__popcll(mask & ((1ull << lane_id()) - 1ull));
    unsigned base = 0;
    if (total && lane_id() == 0) base = atomicAdd(lds_fill, total);
    base = __shfl(base, 0);
    return base + prefix;
}

// ------------------------------------------------------------------ the window sort
// After the first bounce the 64 paths of a wave hit surfaces of five material kinds and every wave runs every
// kind's BSDF code (PMC: 3750 VALU instructions per wave and vertex at 55 % lane utilisation against 2740 at
// 91 % for the camera rays' vertices).  The paths of a window — win_iters (<= SHADE_WIN) iterations of the block, starting
// at `wbase` of a queue of `n` — are therefore dealt to the lanes sorted by the material kind of what they hit (the
// traversal kernel left the kind in the hit word): with 4 x 256 paths and six keys most waves see ONE kind.  Which lane
// shades which path has no influence on any result.  Counting sort: per key one ballot per wave and one LDS atomic per
// wave and key.  Leaves the `order` table in `stg` and returns the number of iterations that hold a path.
template <int BLOCK, class Staging>
__device__ __forceinline__ unsigned sort_window(Staging& stg, const int* hit_tri, unsigned wbase, unsigned win_iters, unsigned n) {
    if (threadIdx.x < 8) stg.bucket[threadIdx.x] = 0;
    __syncthreads();
    unsigned key[SHADE_WIN], rank[SHADE_WIN];
#pragma unroll
    for (int k = 0; k < SHADE_WIN; ++k) {
        const unsigned i0 = wbase + k * BLOCK + threadIdx.x;
        const bool in = (unsigned)k < win_iters && i0 < n;
        const int t = in ? hit_tri[i0] : -1;
        key[k] = !in ? 7u : (t < 0 ? 6u : ((unsigned)t >> YK_HIT_KIND_SHIFT));
    }
#pragma unroll
    for (int k = 0; k < SHADE_WIN; ++k) {
        rank[k] = 0;
        if ((unsigned)k >= win_iters) continue;  // block-uniform
        for (unsigned q = 0; q < 8; ++q) {  // wave-uniform loop: every lane takes part in every ballot
            const unsigned long long m = __ballot(key[k] == q);
            if (m == 0ull) continue;
            unsigned b0 = 0;
            if (lane_id() == 0) b0 = atomicAdd(&stg.bucket[q], (unsigned)__popcll(m));
            b0 = __shfl(b0, 0);
            if (key[k] == q) rank[k] = b0 + (unsigned)__popcll(m & ((1ull << lane_id()) - 1ull));
        }
    }
    __syncthreads();
    unsigned first[8], n_sub;
    {
        unsigned acc = 0;
        for (unsigned q = 0; q < 8; ++q) {
            first[q] = acc;
            acc += stg.bucket[q];
        }
        n_sub = (acc - stg.bucket[7] + BLOCK - 1) / BLOCK;  // the invalid entries sort last: trailing iterations without any path are skipped
    }
#pragma unroll
    for (int k = 0; k < SHADE_WIN; ++k)
        if ((unsigned)k < win_iters) stg.order[first[key[k]] + rank[k]] = (unsigned short)(k * BLOCK + threadIdx.x);
    __syncthreads();
    return n_sub;
}
// an unsorted window's iterations (wbase < n: at least one path)
template <int BLOCK> __device__ __forceinline__ unsigned plain_window(unsigned wbase, unsigned win_iters, unsigned n) {
    const unsigned left = n - wbase;
    return left >= win_iters * BLOCK ? win_iters : (left + BLOCK - 1) / BLOCK;
}
// the path this thread shades in iteration `sub` of the window, as an offset from the window's base
template <int BLOCK, class Staging> __device__ __forceinline__ unsigned window_offset(const Staging& stg, unsigned reorder, unsigned sub) {
    return reorder ? (unsigned)stg.order[sub * BLOCK + threadIdx.x] : sub * BLOCK + threadIdx.x;
}

// ------------------------------------------------------------------ the staging protocol
// The staging buffer only ever holds shadow rays of ONE class — towards area lights, or (`split_delta`) towards point /
// spot / distant lights — and is flushed to that class's queue when the class of the light changes.
//
// Two modes.  `per_iter`: a whole iteration's shadow rays fit the staging buffer and they all go to one queue, so the
// flush decisions are taken once per iteration (room_for_iteration) and the appends need no barriers — the barriers of
// the per-light decisions cost more than the math between them.  Otherwise the decisions are taken light by light
// (room_for_light) and once more before the survivors (room_for_survivor).
template <int BLOCK, int CAP, int CAPQ> struct ShadeQueue {
    ShadeStaging<CAP, CAPQ>& stg;
    const BounceQueues& q;
    const PathBuffers& nxt;
    const DevScene& sc;
    const unsigned nl, split_delta;
    const bool per_iter;

    __device__ __forceinline__ ShadeQueue(ShadeStaging<CAP, CAPQ>& stg_, const BounceQueues& q_, const PathBuffers& nxt_, const DevScene& sc_, unsigned split_delta_)
        : stg(stg_), q(q_), nxt(nxt_), sc(sc_), nl(sc_.n_lights), split_delta(split_delta_), per_iter(!split_delta_ && BLOCK * sc_.n_lights <= (unsigned)CAPQ) {}

    // Empties the staging and returns the length of the bounce's path queue.  An interrupted render: the queue counts as
    // empty for the WHOLE block (the barriers need block-uniform control flow, so the word is read by one thread and shared
    // through LDS) and nothing is appended for the next bounce; a block lives for one or two windows of a long launch (the
    // grid has 256 blocks per CU), so this is also the launch's look "per window".
    // (readfirstlane: an LDS read is per-lane to the compiler, the queue length has to stay a scalar)
    __device__ __forceinline__ unsigned begin(const CancelRef& cancel) {
        if (threadIdx.x == 0) {
            stg.fill_p = 0;
            stg.fill_q = 0;
            stg.q_delta = 0;
            stg.untraced = 0;
            stg.cancel = cancel_raised(cancel) ? 1u : 0u;
        }
        __syncthreads();
        return __builtin_amdgcn_readfirstlane((int)stg.cancel) ? 0u : *q.count;
    }

    __device__ __forceinline__ void flush_q(unsigned fill, unsigned delta) {
        if (threadIdx.x == 0) stg.gbase = atomicAdd(delta ? q.delta.count : q.area.count, fill);
        __syncthreads();
        const unsigned gb = stg.gbase;
        float4* dO = delta ? q.delta.O : q.area.O;
        float4* dD = delta ? q.delta.D : q.area.D;
        unsigned* dS = delta ? q.delta.slot : q.area.slot;
        for (unsigned k = threadIdx.x; k < fill; k += BLOCK) {
            dO[gb + k] = stg.qO[k];
            dD[gb + k] = stg.qD[k];
            dS[gb + k] = stg.qS[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) stg.fill_q = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void flush_p(unsigned fill) {
        if (threadIdx.x == 0) stg.gbase = atomicAdd(q.next_count, fill);
        __syncthreads();
        const unsigned gb = stg.gbase;
        for (unsigned k = threadIdx.x; k < fill; k += BLOCK) {
            nxt.rayO[gb + k] = stg.pO[k];
            nxt.rayD[gb + k] = stg.pD[k];
            nxt.thru[gb + k] = stg.pT[k];
            nxt.rngs[gb + k] = stg.pR[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) stg.fill_p = 0;
        __syncthreads();
    }

    // per_iter: ONE block-wide decision per iteration — room for every shadow ray (BLOCK x nl) and every continuation
    // (BLOCK) this iteration can stage
    __device__ __forceinline__ void room_for_iteration() {
        if (!per_iter) return;
        __syncthreads();
        const unsigned fq = stg.fill_q, fp = stg.fill_p, staged = stg.q_delta;
        __syncthreads();
        if (fq && fq + BLOCK * nl > CAPQ) flush_q(fq, staged);
        if (fp + BLOCK > CAP) flush_p(fp);
    }
    // light by light: room for BLOCK shadow rays of light l's class
    __device__ __forceinline__ void room_for_light(unsigned l) {
        if (per_iter) return;
        __syncthreads();
        const unsigned f = stg.fill_q, staged = stg.q_delta;
        const unsigned delta = (split_delta && sc.lights[l].kind != YK_LIGHT_RECT) ? 1u : 0u;
        __syncthreads();  // every wave has read the same fill before any wave appends again
        if (f && (staged != delta || f + BLOCK > CAPQ)) flush_q(f, staged);
        if (threadIdx.x == 0) stg.q_delta = delta;
    }
    __device__ __forceinline__ void room_for_survivor() {
        if (per_iter) return;
        __syncthreads();
        const unsigned f = stg.fill_p;
        __syncthreads();
        if (f + BLOCK > CAP) flush_p(f);
    }

    // Light l's verdict byte and shadow ray of path i.  Verdict bytes: up to four lights share one word (`vword`, written
    // once after the loop by store_verdicts, read once by k_accumulate).  The shadow ray is appended densely (coalesced for
    // the any-hit kernel) with the verdict byte it belongs to; the contribution stays at its (path, light) slot for
    // `accumulate`.
    __device__ __forceinline__ void stage_shadow(const NeeSample& ne, bool valid, unsigned i, unsigned l, unsigned& vword) {
        const unsigned vs = YK_VIS_STRIDE(nl);
        const unsigned slot = i * nl + l, vslot = i * vs + l;
        const bool want = ne.want;
        if (vs == 4u)
            vword |= (want ? 1u : 0u) << (8u * l);
        else if (valid)
            q.vis[vslot] = want ? 1 : 0;
        const unsigned long long zm = __ballot(ne.zero);  // not wanted, but shadow rays of the render: finish() reports the block's
        if (zm != 0ull && lane_id() == 0) atomicAdd(&stg.untraced, (unsigned)__popcll(zm));
        room_for_light(l);
        const unsigned k = block_append(want, &stg.fill_q);
        if (want) {
            stg.qO[k] = make_float4(ne.so.x, ne.so.y, ne.so.z, YK_SHADOW_T_MAX);
            stg.qD[k] = make_float4(ne.sd.x, ne.sd.y, ne.sd.z, __uint_as_float((unsigned)ne.al));
            stg.qS[k] = vslot;
            q.shC[slot] = make_float4(ne.contrib.r, ne.contrib.g, ne.contrib.b, 0.0f);
        }
    }
    __device__ __forceinline__ void store_verdicts(bool valid, unsigned i, unsigned vword) {
        if (YK_VIS_STRIDE(nl) == 4u && valid) reinterpret_cast<unsigned*>(q.vis)[i] = vword;
    }

    // stream compaction of the survivors into the other path buffer
    __device__ __forceinline__ void stage_survivor(bool alive, const PathWords& w) {
        room_for_survivor();
        const unsigned j = block_append(alive, &stg.fill_p);
        if (alive) {
            stg.pO[j] = w.O;
            stg.pD[j] = w.D;
            stg.pT[j] = w.T;
            stg.pR[j] = w.R;
        }
    }

    // Flushes what is staged and reports the block's untraced shadow rays: one atomic per block that has any, the last thing
    // the block does (an agent-scope access at a block's start or in front of a barrier is waited for: yk_device.h, cancel_raised).
    // The waves count into LDS as they go (stage_shadow): a count carried in a register through the loops cost k_shade two
    // spilled VGPRs at its 168.
    __device__ __forceinline__ void finish(unsigned long long* shadow_counter) {
        __syncthreads();
        const unsigned fq = stg.fill_q, fp = stg.fill_p, nz = stg.untraced;
        if (fq) flush_q(fq, stg.q_delta);
        if (fp) flush_p(fp);
        if (threadIdx.x == 0 && nz && shadow_counter) atomicAdd(shadow_counter, (unsigned long long)nz);
    }
};

}  // namespace yk
