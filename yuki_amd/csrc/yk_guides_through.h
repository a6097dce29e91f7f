// yk_guides_through.h — guides through glass: the denoiser's records (yk_guide, yk_surface_id) of the surface a pixel SHOWS,
// not of the pane in front of it.  The first-hit pass (k_guides, yk_kernels.hip) describes the first hit of the pixel's centre
// ray; where that is glass, everything seen through the pane shares its normal and its plane, its albedo is "all ones" and
// its history lags.  Glass is the renderer's only delta material (two specular lobes; metal and glossy are microfacet), so
// the rule "write the features at the first non-specular hit" is small and exact.
//
// The reference has no such pass, so this file is the rule.  IEEE-754 binary32, round to nearest, every operation separate
// (-ffp-contract=off).  Per pixel (x, y): ray_0 = Camera::ray((x + 0.5, y + 0.5)) — the guide pass's ray — and k = 0.
//
//   1. Trace the closest hit of ray_k = (o_k, d_k) with the render loop's closest-hit kernel, t_max = inf.
//   2. Miss: the all-zero guide, the id (YK_SURFACE_NONE, 0, 0, 0), through = k.
//   3. Hit: sf = hit_surface_prim(scene, slot, o_k, d_k, scene has texels, &t_k, &id_k), the call of k_guides<true>.
//      T_0 = t_0;  T_k = T_{k-1} + t_k (one addition per interface, in this order).
//   4. Final record — the material is not glass, or k == max_through, or step 5 takes no lobe:
//        guide = (sf.ns, 1.0f, sf.p, T_k), id = id_k (the surface id of THIS hit), through = k.
//      For k == 0 that is k_guides<true>'s record bit for bit.
//   5. Glass and k < max_through (gt_continue below): the frame make_frame(sf.n, sf.ns, sf.dpdus) and the material record
//      as k_shade builds them, wo = -d_k.  The transmission lobe, bsdf_sample_specular(.., BX_TRANSMISSION), is taken unless
//      Kt is exactly (0, 0, 0) or the lobe answers BX_NONE (total internal reflection); otherwise the reflection lobe,
//      bsdf_sample_specular(.., BX_REFLECTION), unless Kr is exactly (0, 0, 0).  Neither: step 4.  Else
//        ray_{k+1} = (spawn_origin(sf.p, sf.n, wi), wi), wi as the lobe returns it (not renormalised, as Path continues),
//      k <- k + 1, step 1.
//
// max_through = 0 .. YK_GUIDES_THROUGH_MAX; at 0 the records are yk_render_guides_ids' byte for byte.
//
// On the device (yk_guides_through.hip, driven from the guide route of yk_render.cpp): raygen -> closest-hit trace ->
// k_guides_step, then max_through times closest-hit trace of the continuation queue -> k_guides_step, all on one stream and
// without a host read-back: a pass reads its ray count from the control word the step before it wrote.  A ray record
// carries what the next step needs in its two spare lanes: rayO.w = T_{k-1} (a float; the path flags the render loop keeps
// there mean nothing here and no traversal kernel reads the lane), rayD.w = the sample id, whose pixel-table entry is the pixel.
//
// Limits: one deterministic branch per interface — a pane's mirror image is not guided; the albedo behind
// tinted glass ignores Kt; p is the real position of the surface seen, not a virtual image, so reprojection and motion
// through refraction are approximate; metal and glossy are not followed; yk_multi scenes are not served.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_bsdf.h"
#include "yk_device.h"
#include "yk_geom.h"
#include "yk_math.h"

namespace yk {

// Step 5 at a hit `sf` of a ray with direction d: false — the record at this hit is final; true — (no, wi) is ray_{k+1}.
// Only wi of the lobe's sample is used: its f and pdf (Fresnel terms) are dead code here.
__device__ __forceinline__ bool gt_continue(const DevScene& sc, const Surface& sf, V3 d, V3& no, V3& wi) {
    const Material mat = sc.materials[sf.material];  // glass carries no texture: vertex_setup_material's texel fetch changes matte records only
    if (mat.kind != MK_GLASS) return false;
    const Frame fr = make_frame(sf.n, sf.ns, sf.dpdus);
    const V3 wo = -d;
    const bool kr_black = mat.a[0] == 0.0f && mat.a[1] == 0.0f && mat.a[2] == 0.0f;
    const bool kt_black = mat.b[0] == 0.0f && mat.b[1] == 0.0f && mat.b[2] == 0.0f;
    BsdfSample s = bsdf_sample_none();
    if (!kt_black) s = bsdf_sample_specular(mat, fr, wo, BX_TRANSMISSION);
    if (s.type == BX_NONE && !kr_black) s = bsdf_sample_specular(mat, fr, wo, BX_REFLECTION);
    if (s.type == BX_NONE) return false;
    wi = s.wi;
    no = spawn_origin(sf.p, sf.n, wi);
    return true;
}

// k_guides_step for pass k of the rays in `cur` whose hits are in hit_tri: *count rays (a device word; the launch covers
// n_max >= *count lanes, the rest exit).  Final records go to guides / ids / through at the ray's pixel of a res_x-wide
// row-major film (each may be null, a kernel argument); continuation rays are appended to `nxt` and counted in *next_count
// (zero before the launch).  last: k == max_through — every hit is final, nxt and next_count are not touched.
void launch_guides_step(hipStream_t s, const DevScene& sc, PathBuffers cur, PathBuffers nxt, const int* hit_tri, const unsigned* count, unsigned* next_count,
                        uint32_t n_max, uint32_t k, bool last, const uint32_t* pixel_xy, uint32_t res_x, float4* guides, uint4* ids, uint32_t* through);

}  // namespace yk
