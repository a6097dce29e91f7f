// yk_guides_through.hip — guides through glass on gfx950 (the rule: yk_guides_through.h), behind yk_render_guides_through.
//
// k_guides_step: one lane per queued ray of pass k, 256 to a block.  A lane reads its ray (two 16-byte loads) and
//   hit word, rebuilds the surface (hit_surface_prim: the primitive's 48-byte record, its shading word and, where the scene
//   has them, 64 bytes of vertex attributes), reads the material record and either writes the pixel's final records (two
//   16-byte stores, one more for the id, four bytes for `through`) or appends the continuation ray to the other path buffer
//   (two 16-byte stores).  Compaction: one ballot per wave, the block's four wave totals through 20 bytes of LDS, and ONE
//   global atomic per block that continues at all.  One atomic per WAVE was measured first (profiles/guides_through_device.json,
//   "per_wave_atomic"): on cfg5 at 1080p, where a quarter of the camera rays continue, the 32 K returning atomics on one
//   word made pass 0 take 172.6 us against 76.7 us with one per block (cfg3: 71.3 against 52.4 us) — the counter word is
//   the cost, as yk_shade_queue.h found for k_shade.  Queue order depends on which block's atomic lands first; the outputs
//   are per pixel and do not.  All lanes of a block stay to the barriers together: the only early exit is block-uniform.
//   LAST (k == max_through): every hit is final — no material read, no lobe, no ballot; the instantiation of max_through = 0
//   is k_guides<true> plus the `through` store.
#include <hip/hip_runtime.h>

#include "yk_guides_through.h"
#include "yk_path_state.h"
#include "yk_wave.h"

namespace {

using namespace yk;

template <bool LAST>
__global__ __launch_bounds__(256) void k_guides_step(DevScene sc, PathBuffers cur, PathBuffers nxt, const int* __restrict__ hit_tri, const unsigned* __restrict__ count,
                                                     unsigned* next_count, uint32_t k, const uint32_t* __restrict__ pixel_xy, uint32_t res_x, float4* guides, uint4* ids,
                                                     uint32_t* through) {
    const unsigned n = *count;
    if (blockIdx.x * blockDim.x >= n) return;  // block-uniform: launched for the batch's worst case
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    bool cont = false;
    float4 nO = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nD = nO;
    if (valid) {
        const float4 rd = cur.rayD[i];
        const uint32_t xy = pixel_xy[path_sample_id(rd)];
        const size_t px = (size_t)(xy >> 16) * res_x + (xy & 0xffffu);
        const int tri = hit_tri[i];
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;  // step 2: a miss
        uint4 id = make_uint4(YK_SURFACE_NONE, 0u, 0u, 0u);
        if (tri >= 0) {
            const float4 ro = cur.rayO[i];
            float t = 0.0f;
            const Surface sf = hit_surface_prim(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, f4_xyz(ro), f4_xyz(rd), sc.texels != nullptr, &t, &id);  // step 3
            const float T = k == 0u ? t : ro.w + t;
            V3 no = V3{0.0f, 0.0f, 0.0f}, wi = no;
            if (!LAST) cont = gt_continue(sc, sf, f4_xyz(rd), no, wi);  // step 5
            nO = make_float4(no.x, no.y, no.z, T);
            nD = make_float4(wi.x, wi.y, wi.z, rd.w);
            a = make_float4(sf.ns.x, sf.ns.y, sf.ns.z, 1.0f);  // step 4
            b = make_float4(sf.p.x, sf.p.y, sf.p.z, T);
        }
        if (!cont) {
            if (guides) {
                guides[2 * px] = a;
                guides[2 * px + 1] = b;
            }
            if (ids) ids[px] = id;
            if (through) through[px] = k;
        }
    }
    if (LAST) return;
    // compaction: a ballot per wave, the four wave totals through LDS, one global atomic per block that continues at all
    __shared__ unsigned wave_total[4], block_base;
    const unsigned wv = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(cont);
    const unsigned prefix = (unsigned)__popcll(mask & ((1ull << lane_id()) - 1ull));
    if (lane_id() == 0) wave_total[wv] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        block_base = total ? atomicAdd(next_count, total) : 0u;
    }
    __syncthreads();
    if (cont) {  // j < *count <= the buffers' capacity: a pass appends at most one ray per ray it was given
        unsigned j = block_base + prefix;
        for (unsigned w = 0; w < wv; ++w) j += wave_total[w];
        nxt.rayO[j] = nO;
        nxt.rayD[j] = nD;
    }
}

}  // namespace

namespace yk {

void launch_guides_step(hipStream_t s, const DevScene& sc, PathBuffers cur, PathBuffers nxt, const int* hit_tri, const unsigned* count, unsigned* next_count,
                        uint32_t n_max, uint32_t k, bool last, const uint32_t* pixel_xy, uint32_t res_x, float4* guides, uint4* ids, uint32_t* through) {
    if (!n_max) return;
    const dim3 grid((n_max + 255u) / 256u), block(256);
    if (last)
        hipLaunchKernelGGL(k_guides_step<true>, grid, block, 0, s, sc, cur, nxt, hit_tri, count, next_count, k, pixel_xy, res_x, guides, ids, through);
    else
        hipLaunchKernelGGL(k_guides_step<false>, grid, block, 0, s, sc, cur, nxt, hit_tri, count, next_count, k, pixel_xy, res_x, guides, ids, through);
}

}  // namespace yk
