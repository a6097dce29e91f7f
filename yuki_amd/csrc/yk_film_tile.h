// yk_film_tile.h — the block shape of the film kernels that map a lane to a pixel of a 2-D tile, and the staging of a
// block's tile plus a halo in LDS.  The shape: the à-trous kernel (yk_denoise.hip), k_variance (yk_variance.hip), k_reproject
// (yk_temporal.hip), k_motion (yk_motion.hip), k_albedo and k_albedo_mean (yk_albedo.hip); the LDS tile: the first two.  Device
// code, library-private.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace yk {

constexpr unsigned FT_TX = 32, FT_TY = 8;  // a block is a 32 x 8 tile of the film, a lane a pixel: 256 lanes, 4 waves of 64

inline dim3 ft_grid(uint32_t res_x, uint32_t res_y) { return dim3((res_x + FT_TX - 1) / FT_TX, (res_y + FT_TY - 1) / FT_TY); }
inline dim3 ft_block() { return dim3(FT_TX, FT_TY); }

// This block's tile with a halo of H pixels on every side, as N entries of the caller's __shared__ arrays, row-major.
// Entries outside the film are neither written nor read: stage() skips them, and a tap outside the film is skipped by the
// per-pixel rules before it is fetched.
template <int H>
struct FilmTile {
    static constexpr int W = (int)FT_TX + 2 * H, ROWS = (int)FT_TY + 2 * H, N = W * ROWS;
    int bx, by;  // the film coordinate of entry 0
    __device__ FilmTile() : bx((int)(blockIdx.x * FT_TX) - H), by((int)(blockIdx.y * FT_TY) - H) {}
    // the entry of film pixel (qx, qy), which lies inside the tile plus halo
    __device__ int index(uint32_t qx, uint32_t qy) const { return ((int)qy - by) * W + ((int)qx - bx); }
    // load(k, gx, gy) fills entry k from film pixel (gx, gy), for every entry inside the film; then the block meets
    template <class Load>
    __device__ void stage(uint32_t res_x, uint32_t res_y, const Load& load) const {
        for (int k = (int)(threadIdx.y * FT_TX + threadIdx.x); k < N; k += (int)(FT_TX * FT_TY)) {
            const int gx = bx + k % W, gy = by + k / W;
            if (gx < 0 || gy < 0 || gx >= (int)res_x || gy >= (int)res_y) continue;
            load(k, (uint32_t)gx, (uint32_t)gy);
        }
        __syncthreads();
    }
};

}  // namespace yk
