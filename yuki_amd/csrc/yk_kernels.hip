// yk_kernels.hip — gfx950 kernels of the wavefront Path integrator.
//
// One bounce of every in-flight path = four launches over dense, compacted arrays:
//
//   trace_closest   BoundingVolumeHierarchy::intersect      bvh.rs:160-232
//   shade           Path::li_internal body                   path.rs:89-169
//                   (surface reconstruction, NEE light sampling, emission,
//                    BSDF sampling, Russian roulette, wave-ballot compaction of
//                    survivors into the other state buffer)
//   trace_any       BoundingVolumeHierarchy::any_intersect   bvh.rs:235-302
//   accumulate      `incoming_radiance += beta * radiance`   path.rs:102-129
//
// plus raygen (Integrator::render's sample loop + Camera::ray) and resolve
// (the per-pixel mean, integrators/mod.rs:172-182).  All floating-point work
// follows the reference's operation order; built with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "yk_device.h"
#include "yk_geom.h"
#include "yk_kernels.h"
#include "yk_path_state.h"
#include "yk_rng.h"
#include "yk_shade.h"
#include "yk_shade_queue.h"
#include "yk_wave.h"

namespace yk {

// ------------------------------------------------------------------ pixel table
// chunk-local pixel index -> pixel coordinates, tile-major / row-major in tile
// (the order Integrator::render visits them, integrators/mod.rs:145)
__global__ void k_pixel_table(const yk_tile* tiles, const uint32_t* tile_offset, uint32_t n_tiles, uint32_t n_pixels,
                              uint32_t* pixel_xy, const uint16_t* tile_sample, uint32_t* pixel_sample) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    uint32_t lo = 0, hi = n_tiles;  // last tile with offset <= i
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (tile_offset[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    yk_tile t = tiles[lo];
    uint32_t w = (uint32_t)t.x1 - t.x0;
    uint32_t r = i - tile_offset[lo];
    uint32_t x = t.x0 + r % w, y = t.y0 + r / w;
    pixel_xy[i] = x | (y << 16);
    if (tile_sample) pixel_sample[i] = tile_sample[lo];  // FilmTile.sample of the pixel's tile (accumulating film)
}

// the same for a chunk of ONE tile — the reference's per-tile Integrator::render call: the tile travels as a kernel argument
// (no upload, no host synchronisation for the staging buffer)
__global__ void k_pixel_table_one(yk_tile t, uint32_t n_pixels, uint32_t* pixel_xy, uint32_t tile_sample, uint32_t* pixel_sample) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    uint32_t w = (uint32_t)t.x1 - t.x0;
    pixel_xy[i] = (t.x0 + i % w) | ((t.y0 + i / w) << 16);
    if (pixel_sample) pixel_sample[i] = tile_sample;
}

// per-pixel part of the camera samples' sampler start (yk_rng.h, PixelSampler): (stream.lo, stream.hi, hash0, -)
__global__ void k_pixel_sampler(SamplerCfg cfg, const uint32_t* pixel_xy, uint32_t n_pixels, uint4* pixel_aux) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const uint32_t xy = pixel_xy[i];
    const PixelSampler ps = pixel_sampler(cfg, xy & 0xffffu, xy >> 16);
    pixel_aux[i] = make_uint4((unsigned)ps.stream, (unsigned)(ps.stream >> 32), ps.hash0, 0u);
}

// ------------------------------------------------------------------ raygen
// sampler.start_pixel_sample(p, sample_index, 0); p_film = p + get_2d();
// ray = camera.ray(p_film)     integrators/mod.rs:163-169, camera.rs:105-114
__device__ __forceinline__ void camera_ray(const DevCamera& cam, float fx, float fy, V3& o, V3& d) {
    V3 p_camera = xf_point(cam.r2c, V3{fx, fy, 0.0f});
    V3 dir = normalize(p_camera);
    o = xf_point(cam.c2w, V3{0.0f, 0.0f, 0.0f});
    d = xf_vector(cam.c2w, dir);
}

// `pixel_sample` != null: the accumulating film (integrators/mod.rs:146-161) — prm.spe passes of ONE sample per
// pixel whose global index is the tile's FilmTile.sample; otherwise all spp samples.
__global__ void k_raygen(DevCamera cam, RenderParams prm, const uint32_t* pixel_xy, const uint32_t* pixel_sample, uint64_t work0, uint32_t n,
                         PathBuffers out, float4* sample_buf, unsigned* count, float4* lean_origin, const uint4* pixel_aux) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (cancel_raised(prm.cancel)) return;  // *count stays zero (the batch's control block was cleared): every later kernel of the batch finds an empty queue
    if (i == 0) *count = n;
    if (i >= n) return;
    const uint32_t w = (uint32_t)(work0 + i);  // a chunk holds fewer than 2^32 samples (it indexes sample_buf)
    uint32_t pix, ks;
    split_sample_id(w, prm.spe, pix, ks);
    const uint32_t s = (pixel_sample ? pixel_sample[pix] : prm.sample_base) + ks;
    uint32_t xy = pixel_xy[pix];
    uint32_t px = xy & 0xffffu, py = xy >> 16;
    SamplerState st;
    float ux, uy;
    if (pixel_aux) {  // the pixel's share of the work was done once per pixel (k_pixel_sampler)
        const uint4 a = pixel_aux[pix];
        PixelSampler ps;
        ps.stream = (u64)a.x | ((u64)a.y << 32);
        ps.hash0 = a.z;
        st = sampler_start_camera(prm.sampler, ps, px, py, s, ux, uy);
    } else {
        st = sampler_start(prm.sampler, px, py, s, 0);
        sampler_get_2d(prm.sampler, st, ux, uy);
    }
    V3 o, d;
    camera_ray(cam, (float)px + ux, (float)py + uy, o, d);
    // lean (yk_device.h, YK_CTRL_CAM_O): one origin for all, throughput one, two sampler dimensions drawn
    path_store_camera(out, i, o, d, w, st, lean_origin, i == 0);
    // The Path integrator's first accumulate pass writes every sample of the batch (every camera ray hits or misses) and
    // starts from zero itself; only where no such pass follows does the slot have to be cleared here.
    if (prm.integrator != YK_INTEGRATOR_PATH || prm.max_depth == 0) sample_buf[w] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// Integrator::li entry: caller-supplied rays (yk_li)
__global__ void k_raygen_user(RenderParams prm, const float* ray_o, const float* ray_d, const uint16_t* pixel, const uint32_t* sample_index,
                              uint32_t dimension, uint32_t n, PathBuffers out, float4* sample_buf, uint32_t* pixel_xy, unsigned* count) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *count = n;
    if (i >= n) return;
    uint32_t px = pixel[2 * i], py = pixel[2 * i + 1];
    pixel_xy[i] = px | (py << 16);
    SamplerState st = sampler_start(prm.sampler, px, py, sample_index[i], dimension);
    if (prm.sampler.kind == 1) st.dimension = dimension;  // caller already consumed `dimension` draws
    path_store_camera(out, i, ld3(ray_o, i), ld3(ray_d, i), i, st, nullptr, false);
    if (prm.integrator != YK_INTEGRATOR_PATH || prm.max_depth == 0) sample_buf[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ------------------------------------------------------------------ shade
// Path::li_internal for one vertex of every active path (path.rs:89-169): the physics of the vertex is yk_shade.h, the
// window sort and the staging of shadow rays and survivors are yk_shade_queue.h; this kernel strings them together.
//
// Diagnostic builds only (tools/build_variant.sh prof -DYK_SHADE_PROFILE): per-wave cycle stamps around the stages of an
// iteration, summed into a device array (tools/micro/shade_profile.h).  The product build sees empty macros.
#ifdef YK_SHADE_PROFILE
#include "../../tools/micro/shade_profile.h"
#else
#define YK_PROF_DECL
#define YK_PROF_STAMP(k)
#define YK_PROF_FLUSH
#endif

template <int BLOCK, int CAP, int CAPQ>
__global__ __launch_bounds__(BLOCK, SHADE_MIN_WAVES) void k_shade(DevScene sc, RenderParams prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab,
                                                                  PathBuffers cur, PathBuffers nxt, BounceQueues q, ShadeArgs a,
                                                                  const float4* __restrict__ lean_origin) {
    static_assert(sizeof(ShadeStaging<CAP, CAPQ>) <= 53296, "k_shade: more LDS than the measured 53296 bytes per block (42 granules = 53760 cost the third block per CU)");
    __shared__ ShadeStaging<CAP, CAPQ> stg;
    // iterations per window: a full queue sorts win_max (<= SHADE_WIN) x 256 paths together; a queue too short to give every
    // resident block (`block_slots` of them on the device) a full window takes shorter ones, down to one iteration
    const unsigned win_iters = min(a.win_max, max(1u, *q.count / (BLOCK * a.block_slots)));
    ShadeQueue<BLOCK, CAP, CAPQ> sq(stg, q, nxt, sc, a.split_delta);
    const unsigned n = sq.begin(prm.cancel);
    // all lanes stay in the loops together so the ballots of the sort and the staging see whole waves
    const unsigned WIN = win_iters * BLOCK;  // paths per window
    const unsigned n_win = (n + WIN - 1) / WIN;
    YK_PROF_DECL
    for (unsigned w = blockIdx.x; w < n_win; w += gridDim.x) {
        const unsigned wbase = w * WIN;
        YK_PROF_STAMP(0)
        const unsigned n_sub = a.reorder ? sort_window<BLOCK>(stg, q.hit, wbase, win_iters, n) : plain_window<BLOCK>(wbase, win_iters, n);
        for (unsigned sub = 0; sub < n_sub; ++sub) {
            const unsigned i = wbase + window_offset<BLOCK>(stg, a.reorder, sub);
            const bool valid = i < n;
            YK_PROF_STAMP(1)
            sq.room_for_iteration();
            PathState ps = path_inert();
            SamplerState st = sampler_inert();
            PathVertex v = vertex_inert();
            bool hit = false;
            if (valid) {
                ps = path_load(cur, i, lean_origin);
                // film renders: sample_id = pixel*spp + sample ; yk_li: one table entry per ray
                st = path_sampler(prm, pixel_xy, sample_index_tab, ps);
                const int tri = q.hit[i];
                hit = tri >= 0;
                if (hit) vertex_setup(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, ps.o, ps.d, v);  // the leaf-order slot reported by the render-loop trace kernels
            }
            YK_PROF_STAMP(2)
            // next-event estimation over ALL lights (path.rs:102-119); two sampler dimensions are consumed per light whether
            // or not it contributes
            unsigned vword = 0u;
            for (unsigned l = 0; l < sq.nl; ++l) {
                NeeSample ne = nee_none();
                if (valid && hit) ne = vertex_light(sc, prm, st, l, v);
                sq.stage_shadow(ne, valid, i, l, vword);
            }
            sq.store_verdicts(valid, i, vword);
            YK_PROF_STAMP(3)
            bool alive = false;
            PathWords next = PathWords{make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
            if (valid) {
                unsigned kind = YK_PEND_MISS;
                RGB term = RGB{0, 0, 0};
                if (!hit) {
                    term = vertex_miss_term(sc, ps.beta);
                } else {
                    const VertexEnd e = vertex_finish(sc, prm, st, v, ps.beta, ps.bounces, ps.specular);
                    term = e.term;
                    kind = e.kind;
                    alive = e.alive;
                    if (e.sampled) {
                        ps.o = e.no;
                        ps.d = e.wi;
                        ps.dimension = st.dimension;
                        ps.rng = st.rng;
                        next = path_pack(ps);
                    }
                }
                q.pend[i] = pend_pack(term, kind, ps.sid - a.sid_base);
            }
            YK_PROF_STAMP(4)
            sq.stage_survivor(alive, next);
            YK_PROF_STAMP(5)
        }
        if (a.reorder) __syncthreads();  // the next window's sort overwrites `order`
    }
    YK_PROF_FLUSH
    sq.finish(a.shadow_counter);
}

// ------------------------------------------------------------------ accumulate
// radiance = fold over lights (in light order) of the unoccluded contributions,
// + beta*Le, clamp, then incoming_radiance += beta * radiance   (path.rs:102-129)
// `first`: the camera bounce — the sample's radiance so far is zero (raygen does not clear the slot: 0 + x == x bit for bit, a
// stored +0 included), so the slot is written without being read.
__global__ void k_accumulate(RenderParams prm, PathBuffers cur, BounceQueues q, unsigned nl, float4* sample_buf, unsigned first, unsigned sid_base) {
    const unsigned n = cancel_raised(prm.cancel) ? 0u : *q.count;  // an interrupted k_shade left pending terms unwritten: nothing of this bounce is read
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float4 p = q.pend[i];
        const unsigned kind = pend_kind(p);
        const unsigned sid = sid_base + pend_slot(p);
        RGB beta = RGB{1.0f, 1.0f, 1.0f};  // the throughput the vertex was entered with (one at the camera's); a miss adds its term as it is
        if (!first && !(kind & YK_PEND_MISS)) beta = path_beta(cur.thru[i]);
        RGB radiance = RGB{0.0f, 0.0f, 0.0f};
        if (!(kind & YK_PEND_MISS)) {
            const unsigned vs = YK_VIS_STRIDE(nl);
            const unsigned vword = vs == 4u ? reinterpret_cast<const unsigned*>(q.vis)[i] : 0u;  // the verdicts of up to four lights in one word
            for (unsigned l = 0; l < nl; ++l) {
                const unsigned slot = i * nl + l;
                const unsigned verdict = vs == 4u ? (vword >> (8u * l)) & 255u : (unsigned)q.vis[i * vs + l];
                if (verdict == 1u) {
                    float4 ct = q.shC[slot];
                    radiance = radiance + RGB{ct.x, ct.y, ct.z};
                }
            }
        }
        const RGB add = vertex_addend(prm, beta, radiance, RGB{p.x, p.y, p.z}, kind);
        // A vertex after the camera's that adds +-0 in every component leaves the slot as it is, bit for bit: the slot never
        // holds -0 (the first pass writes +0 + x, and a sum is -0 only when both operands are), so it is neither read nor
        // written.  Decided from the product itself: a NaN or an infinity in beta is no zero and goes through.  `L + add` is
        // the former `L + beta * radiance` bit for bit because the library is built with -ffp-contract=off (no fused multiply-add).
        if (!first && !(kind & YK_PEND_MISS) && is_black(add)) continue;
        RGB L = RGB{0.0f, 0.0f, 0.0f};
        if (!first) {
            const float4 acc = sample_buf[sid];
            L = RGB{acc.x, acc.y, acc.z};
        }
        L = L + add;
        sample_buf[sid] = make_float4(L.r, L.g, L.b, 0.0f);
    }
}

// ------------------------------------------------------------------ resolve
// color = sum of the pixel's samples in sample order; color /= spp
// (integrators/mod.rs:172-175); output tile-major like tile_pixels.
__global__ void k_resolve(const float4* sample_buf, uint32_t n_pixels, uint32_t spp, float* out_rgb) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    RGB color = RGB{0.0f, 0.0f, 0.0f};
    const float4* s = sample_buf + (size_t)p * spp;
    // the sum keeps the reference's sample order (integrators/mod.rs:172); the loads of a group
    // of eight are issued together so the serial adds do not wait for one load each
    uint32_t k = 0;
    for (; k + 8 <= spp; k += 8) {
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = s[k + j];
#pragma unroll
        for (int j = 0; j < 8; ++j) color = color + RGB{v[j].x, v[j].y, v[j].z};
    }
    for (; k < spp; ++k) {
        float4 v = s[k];
        color = color + RGB{v.x, v.y, v.z};
    }
    color = color / (float)spp;
    out_rgb[3 * (size_t)p + 0] = color.r;
    out_rgb[3 * (size_t)p + 1] = color.g;
    out_rgb[3 * (size_t)p + 2] = color.b;
}

// Accumulating film, `n_passes` passes rendered at once: the raw value of every (pass, pixel),
// pass-major — what n_passes calls of Integrator::render(accumulating = true) with
// FilmTile.sample, sample + 1, ... would have written (integrators/mod.rs:146-161).
__global__ void k_resolve_passes(const float4* sample_buf, uint32_t n_pixels, uint32_t n_passes, float* out_rgb, size_t pass_stride) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_pixels * n_passes) return;
    const uint32_t p = (uint32_t)(i / n_passes), k = (uint32_t)(i % n_passes);
    const float4 v = sample_buf[i];
    float* o = out_rgb + (size_t)k * pass_stride + 3 * (size_t)p;
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
}

// Film::update_tile on the device (film.rs:236-278): tile-major -> row-major film
__global__ void k_film_scatter(const uint32_t* pixel_xy, uint32_t n_pixels, const float* tile_rgb, uint32_t res_x, float* film_rgb, int accumulate,
                               uint32_t n_passes, size_t pass_stride) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    uint32_t xy = pixel_xy[p];
    size_t dst = (size_t)(xy >> 16) * res_x + (xy & 0xffffu);
    if (accumulate) {  // film.rs:260-272: *fc += c, one pass after the other
        float r = film_rgb[3 * dst + 0], g = film_rgb[3 * dst + 1], b = film_rgb[3 * dst + 2];
        for (uint32_t k = 0; k < n_passes; ++k) {
            const float* t = tile_rgb + (size_t)k * pass_stride + 3 * (size_t)p;
            r += t[0];
            g += t[1];
            b += t[2];
        }
        film_rgb[3 * dst + 0] = r;
        film_rgb[3 * dst + 1] = g;
        film_rgb[3 * dst + 2] = b;
        return;
    }
    film_rgb[3 * dst + 0] = tile_rgb[3 * (size_t)p + 0];
    film_rgb[3 * dst + 1] = tile_rgb[3 * (size_t)p + 1];
    film_rgb[3 * dst + 2] = tile_rgb[3 * (size_t)p + 2];
}

// ------------------------------------------------------------------ debug integrators
// BVHIntersections / GeometryNormals / ShadingNormals / ShadingUVs::li (bvh_heatmap.rs:25-40,
// geometry_normals.rs:24-33, shading_normals.rs, shading_uvs.rs: (uv.x, uv.y, 0) on a hit, black on a miss)
__global__ void k_debug_shade(DevScene sc, uint32_t integrator, PathBuffers cur, const int* hit_tri, const uint4* stats, uint32_t n,
                              float4* sample_buf) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 rd = cur.rayD[i];
    int tri = hit_tri[i];
    RGB c = RGB{0.0f, 0.0f, 0.0f};
    if (integrator == YK_INTEGRATOR_BVH_INTERSECTIONS) {
        uint4 s = stats[i];
        c = RGB{(float)s.x, (float)s.y, tri >= 0 ? (float)s.y : 0.0f};
    } else if (tri >= 0 && integrator == YK_INTEGRATOR_SHADING_UVS) {
        Surface sf = hit_surface_prim(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, f4_xyz(cur.rayO[i]), f4_xyz(rd), true);  // a sphere's uv also without image textures
        c = RGB{sf.u, sf.v, 0.0f};
    } else if (tri >= 0) {
        Surface sf = hit_surface_prim(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, f4_xyz(cur.rayO[i]), f4_xyz(rd));  // the normals integrators trace with the render-loop kernel: leaf-order slots
        V3 nn = integrator == YK_INTEGRATOR_GEOMETRY_NORMALS ? sf.n : sf.ns;
        c = RGB{nn.x, nn.y, nn.z} / 2.0f + 0.5f;
    }
    sample_buf[path_sample_id(rd)] = make_float4(c.r, c.g, c.b, 0.0f);
}

// The guide pass (yk_render_guides): the first-hit geometry of one camera ray per pixel as a yk_guide record — (ns, hit),
// (p, t) — at the pixel's place of a row-major res_x-wide film; a miss is an all-zero record.  One sample per pixel: the
// ray's sample id is its pixel's index in pixel_xy.
// IDS (yk_render_guides_ids): the same trace with the surface id beside the guide — ids[px] = (source shape, bits of b0, b1,
// b2), (YK_SURFACE_NONE, 0, 0, 0) on a miss; either output may then be null (a kernel argument: no lane disagrees).  The
// plain instantiation computes no ids and ignores `ids`.
template <bool IDS>
__global__ void k_guides(DevScene sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, float4* guides, uint4* ids) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 rd = cur.rayD[i];
    const uint32_t xy = pixel_xy[path_sample_id(rd)];
    const size_t px = (size_t)(xy >> 16) * res_x + (xy & 0xffffu);
    const int tri = hit_tri[i];
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    uint4 id = make_uint4(YK_SURFACE_NONE, 0u, 0u, 0u);
    if (tri >= 0) {
        float t = 0.0f;
        const Surface sf = hit_surface_prim(sc, (uint32_t)tri & YK_HIT_PRIM_MASK, f4_xyz(cur.rayO[i]), f4_xyz(rd), sc.texels != nullptr, &t, IDS ? &id : nullptr);
        a = make_float4(sf.ns.x, sf.ns.y, sf.ns.z, 1.0f);
        b = make_float4(sf.p.x, sf.p.y, sf.p.z, t);
    }
    if (!IDS || guides) {
        guides[2 * px] = a;
        guides[2 * px + 1] = b;
    }
    if (IDS && ids) ids[px] = id;
}

#ifdef YK_SHADE_PROFILE
}  // namespace yk
extern "C" int yk_debug_shade_profile(unsigned long long* out8, int reset) {
    unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)hipDeviceSynchronize();
    int rc = (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(yk::yk_shade_prof), sizeof(zero));
    if (reset) rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(yk::yk_shade_prof), zero, sizeof(zero));
    return rc;
}
namespace yk {
#endif

// ------------------------------------------------------------------ launchers
static inline unsigned blocks_for(size_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

void launch_pixel_table(hipStream_t s, const yk_tile* tiles, const uint32_t* tile_offset, uint32_t n_tiles, uint32_t n_pixels, uint32_t* pixel_xy,
                        const uint16_t* tile_sample, uint32_t* pixel_sample) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_pixel_table, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, s, tiles, tile_offset, n_tiles, n_pixels, pixel_xy, tile_sample,
                       pixel_sample);
}
void launch_pixel_table_one(hipStream_t s, const yk_tile& tile, uint32_t n_pixels, uint32_t* pixel_xy, uint32_t tile_sample, uint32_t* pixel_sample) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_pixel_table_one, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, s, tile, n_pixels, pixel_xy, tile_sample, pixel_sample);
}
void launch_pixel_sampler(hipStream_t s, const SamplerCfg& cfg, const uint32_t* pixel_xy, uint32_t n_pixels, uint4* pixel_aux) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_pixel_sampler, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, s, cfg, pixel_xy, n_pixels, pixel_aux);
}
void launch_raygen(hipStream_t s, const DevCamera& cam, const RenderParams& prm, const uint32_t* pixel_xy, const uint32_t* pixel_sample, uint64_t work0,
                   uint32_t n, PathBuffers out, float4* sample_buf, unsigned* count, float4* lean_origin, const uint4* pixel_aux) {
    hipLaunchKernelGGL(k_raygen, dim3(blocks_for(n, 256)), dim3(256), 0, s, cam, prm, pixel_xy, pixel_sample, work0, n, out, sample_buf, count, lean_origin, pixel_aux);
}
void launch_raygen_user(hipStream_t s, const RenderParams& prm, const float* o, const float* d, const uint16_t* pixel, const uint32_t* sample_index,
                        uint32_t dimension, uint32_t n, PathBuffers out, float4* sample_buf, uint32_t* pixel_xy, unsigned* ctrl) {
    hipLaunchKernelGGL(k_raygen_user, dim3(blocks_for(n, 256)), dim3(256), 0, s, prm, o, d, pixel, sample_index, dimension, n, out, sample_buf,
                       pixel_xy, ctrl);
}
void launch_shade(hipStream_t s, unsigned grid, const DevScene& sc, const RenderParams& prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab,
                  PathBuffers cur, PathBuffers nxt, const BounceQueues& q, unsigned split_delta, unsigned reorder, unsigned block_slots, unsigned sid_base,
                  const float4* lean_origin, unsigned long long* shadow_counter) {
    const ShadeArgs a{split_delta, reorder, (unsigned)SHADE_WIN, block_slots, sid_base, shadow_counter};
    hipLaunchKernelGGL((k_shade<256, SHADE_CAP, SHADE_CAPQ>), dim3(grid), dim3(256), 0, s, sc, prm, pixel_xy, sample_index_tab, cur, nxt, q, a, lean_origin);
}
void launch_accumulate(hipStream_t s, unsigned grid, const RenderParams& prm, PathBuffers cur, const BounceQueues& q, unsigned nl, float4* sample_buf,
                       unsigned first, unsigned sid_base) {
    hipLaunchKernelGGL(k_accumulate, dim3(grid), dim3(256), 0, s, prm, cur, q, nl, sample_buf, first, sid_base);
}
void launch_resolve(hipStream_t s, const float4* sample_buf, uint32_t n_pixels, uint32_t spp, float* out_rgb) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_resolve, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, s, sample_buf, n_pixels, spp, out_rgb);
}
void launch_resolve_passes(hipStream_t s, const float4* sample_buf, uint32_t n_pixels, uint32_t n_passes, float* out_rgb, size_t pass_stride) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_resolve_passes, dim3(blocks_for((size_t)n_pixels * n_passes, 256)), dim3(256), 0, s, sample_buf, n_pixels, n_passes, out_rgb, pass_stride);
}
void launch_film_scatter(hipStream_t s, const uint32_t* pixel_xy, uint32_t n_pixels, const float* tile_rgb, uint32_t res_x, float* film_rgb, int accumulate,
                         uint32_t n_passes, size_t pass_stride) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_film_scatter, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, s, pixel_xy, n_pixels, tile_rgb, res_x, film_rgb, accumulate, n_passes, pass_stride);
}
void launch_debug_shade(hipStream_t s, const DevScene& sc, uint32_t integrator, PathBuffers cur, const int* hit_tri, const uint4* stats, uint32_t n,
                        float4* sample_buf) {
    hipLaunchKernelGGL(k_debug_shade, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, integrator, cur, hit_tri, stats, n, sample_buf);
}
void launch_guides(hipStream_t s, const DevScene& sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, float4* guides) {
    hipLaunchKernelGGL(k_guides<false>, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, cur, hit_tri, n, pixel_xy, res_x, guides, (uint4*)nullptr);
}
void launch_guides_ids(hipStream_t s, const DevScene& sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, float4* guides, uint4* ids) {
    hipLaunchKernelGGL(k_guides<true>, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, cur, hit_tri, n, pixel_xy, res_x, guides, ids);
}

}  // namespace yk
