// yk_scan.h — the exclusive scan over a device array that the builder's compaction (yk_bvh_build.hip) and the scene
// layout (yk_scene_layout.hip) share: ranks inside blocks of kScanThreads (k_scan_block), one block scans the block
// sums (k_scan_sums), an optional third pass makes the ranks absolute (k_scan_add).  Device side: .hip files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yk {
namespace scan {

const int kScanThreads = 1024;  // elements per block of a scan

// inclusive scan of v over the 64 lanes of a wave; lane: the caller's lane id
__device__ inline uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off);
        if (lane >= (uint32_t)off) v += o;
    }
    return v;
}
// exclusive scan of v over the block; wt: 16 words of LDS
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t& total, uint32_t* wt) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63u) wt[wave] = inc;
    __syncthreads();
    uint32_t before = inc - v, all = 0u;
    for (uint32_t w = 0; w < nw; ++w) {
        const uint32_t t = wt[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    total = all;
    return before;
}
// value(i), i < n -> its rank inside the block (index) and the block's sum (bsum)
template <class Value> __global__ void __launch_bounds__(kScanThreads) k_scan_block(Value value, uint32_t n, uint32_t* index, uint32_t* bsum) {
    __shared__ uint32_t wt[16];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t total;
    const uint32_t r = block_excl_scan(i < n ? value(i) : 0u, total, wt);
    if (i < n) index[i] = r;
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// one block: bsum -> its exclusive scan; *total_out = the sum of everything
static __global__ void __launch_bounds__(kScanThreads) k_scan_sums(uint32_t* bsum, uint32_t nb, uint32_t* total_out) {
    __shared__ uint32_t wt[16];
    uint32_t run = 0u;
    for (uint32_t base = 0; base < nb; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        uint32_t total;
        const uint32_t r = block_excl_scan(i < nb ? bsum[i] : 0u, total, wt);
        if (i < nb) bsum[i] = run + r;
        run += total;
    }
    if (threadIdx.x == 0) *total_out = run;
}
static __global__ void k_scan_add(uint32_t* index, const uint32_t* __restrict__ bsum, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) index[i] += bsum[i / kScanThreads];
}
// the exclusive scan at i from the two arrays the first two passes leave
__device__ inline uint32_t scan_rank(const uint32_t* index, const uint32_t* bsum, uint32_t i) { return index[i] + bsum[i / kScanThreads]; }

inline uint32_t scan_blocks(uint32_t n) { return (n + kScanThreads - 1) / kScanThreads; }  // words of bsum
// Enqueues the scan of value(0 .. n-1): index and bsum as scan_rank reads them and *total; with `absolute` the third pass
// folds bsum into index, which is then the scan itself.  The caller checks hipGetLastError.
template <class Value> void enqueue_scan(hipStream_t st, Value value, uint32_t n, uint32_t* index, uint32_t* bsum, uint32_t* total, bool absolute) {
    k_scan_block<<<scan_blocks(n), kScanThreads, 0, st>>>(value, n, index, bsum);
    k_scan_sums<<<1, kScanThreads, 0, st>>>(bsum, scan_blocks(n), total);
    if (absolute) k_scan_add<<<(n + 255) / 256, 256, 0, st>>>(index, bsum, n);
}

}  // namespace scan
}  // namespace yk
