// yk_albedo.h — textures under the denoiser: the first-hit albedo of every pixel and the two steps that take it out of the
// film before the à-trous filter (yk_denoise.h) and put it back afterwards.  A filter of radiance has to choose on a
// textured surface between blurring the texture (an open colour stop) and keeping the noise (a closed one); a filter of
// radiance / albedo does not: the texture is not in what it filters.
//
// The reference has neither pass, so this file is the rule.  Its arithmetic is yk_denoise.h's and yk_motion.h's:
//   - IEEE-754 binary32, round to nearest, every operation separate (-ffp-contract=off), divisions correctly rounded;
//   - a NaN that an operation PRODUCES is 0x7fc00000 (dn_canon); a value that is only copied keeps its bits.
// One text, two instances: the host instance (no context) and the kernels of yk_albedo.hip / yk_denoise.hip call
// al_pixel, al_mean_pixel, al_divisor, al_demodulate and al_remodulate and agree bit for bit.
//
// Limits:
//   - Sub-pixel texels and edges.  al_pixel's record is that of ONE ray through the pixel centre; where texels or edges
//     are smaller than a pixel the film averaged something else and the quotient is noisier than it should be.
//     al_mean_pixel (below) is the answer: the mean over an s x s grid of sub-pixel rays.  That grid is regular, not the
//     film's own samples, and an edge pixel between a matte and a non-matte surface mixes its albedo with ones.
//   - Glass, metal and glossy surfaces are not demodulated (their record is all ones), nor are textured spheres: a
//     sphere's uv needs the hit point and libm.
//   - yk_multi scenes are not served; the temporal history stays in radiance.
#pragma once
#include "../../include/yuki_hip.h"
#include "yk_denoise.h"
#include "yk_device.h"
#include "yk_geom.h"
#include "yk_math.h"

namespace yk {

// Everything about a call that does not depend on the pixel.  n_shapes = n_triangles + n_spheres; has_uvs: the scene has
// a uv array at all (two floats a vertex).
struct AlParams {
    uint32_t res_x, res_y;
    uint32_t n_triangles, n_shapes;
    uint32_t n_vertices, n_meshes, n_materials, n_textures;
    uint32_t has_uvs;
};

// Albedo, one pixel with surface id (shape, b0, b1, b2).  `sc` supplies indices, uvs, tri_mesh, tri_material, mesh_flags,
// materials, spheres, texels and tex_info — device pointers in k_albedo, host arrays in the host instance; nothing else of
// it is read.  out = (a, known), the cases in this order:
//   miss          shape == YK_SURFACE_NONE:            (1, 1, 1, 0);
//   out of range  shape >= n_shapes:                   (1, 1, 1, 0) — the index is never followed;
//   material      m = tri_material[shape] for a triangle, spheres[shape - n_triangles].material for a sphere;
//                 m outside materials[]:               (1, 1, 1, 0) — never followed;
//                 materials[m] not a matte (the device kinds MK_LAMBERT, MK_OREN_NAYAR, MK_BLACK are YK_MAT_MATTE):
//                                                      (1, 1, 1, 0);
//   untextured    tex == 0:                            (Kd as bits, 1);
//   sphere        textured, shape >= n_triangles:      (1, 1, 1, 0) — not handled;
//   triangle      textured:  uv = (uv0*b0 + uv1*b1) + uv2*b2 per component, products first, summed left to right, with
//                 uv0..2 the mesh's uvs at the triangle's indices or (0,0), (1,0), (1,1) where the mesh has none
//                 (triangle.rs:142-155); the record is (texture_eval(tex - 1, u, v) as bits, 1).  A texture index outside
//                 tex_info[] (creation refuses it) gives (1, 1, 1, 0), never followed.
// The gather is four hops (id -> material index, mesh, vertex indices -> material, mesh flags, uvs -> texture info ->
// texel).  Every index is clamped into its array and every load is issued whatever the case: a lane that is not a
// triangle asks for triangle 0, a lane without a texture for texture 0, and the case picks among the answers afterwards
// (why).  What a scene does not have at all (triangles, spheres, uvs, textures) is the same for every
// lane and is not loaded.
YK_HD void al_pixel(const AlParams& a, const DevScene& sc, uint32_t shape, float b0, float b1, float b2, float* out) {
    const bool live = shape != YK_SURFACE_NONE && shape < a.n_shapes;
    const bool tri = live && shape < a.n_triangles;
    const bool sph = live && !tri;
    // hop 1: what the shape points at
    int32_t m_tri = 0, m_sph = 0;
    uint32_t mesh = 0, i0 = 0, i1 = 0, i2 = 0;
    if (a.n_triangles != 0u) {
        const size_t t = tri ? (size_t)shape : (size_t)0;
        m_tri = sc.tri_material[t];
        mesh = sc.tri_mesh[t];
        i0 = sc.indices[3 * t];
        i1 = sc.indices[3 * t + 1];
        i2 = sc.indices[3 * t + 2];
    }
    if (a.n_shapes != a.n_triangles) {
        const size_t k = sph ? (size_t)(shape - a.n_triangles) : (size_t)0;
        m_sph = sc.spheres[k].material;
    }
    const uint32_t m = (uint32_t)(tri ? m_tri : m_sph);
    const bool m_ok = live && m < a.n_materials;
    // hop 2: the material, the mesh flags and the uvs
    const Material* mp = sc.materials + (m_ok ? m : 0u);
    const uint32_t kind = mp->kind, tex = mp->tex;
    const float kd0 = mp->a[0], kd1 = mp->a[1], kd2 = mp->a[2];
    const uint32_t mfl = sc.mesh_flags[mesh < a.n_meshes ? mesh : 0u];
    float u0x = 0.0f, u0y = 0.0f, u1x = 1.0f, u1y = 0.0f, u2x = 1.0f, u2y = 1.0f;
    if (a.has_uvs != 0u && a.n_vertices != 0u) {
        const size_t v0 = i0 < a.n_vertices ? i0 : 0u, v1 = i1 < a.n_vertices ? i1 : 0u, v2 = i2 < a.n_vertices ? i2 : 0u;
        const float l0x = sc.uvs[2 * v0], l0y = sc.uvs[2 * v0 + 1];
        const float l1x = sc.uvs[2 * v1], l1y = sc.uvs[2 * v1 + 1];
        const float l2x = sc.uvs[2 * v2], l2y = sc.uvs[2 * v2 + 1];
        if (mfl & YK_MESH_UVS) {
            u0x = l0x; u0y = l0y;
            u1x = l1x; u1y = l1y;
            u2x = l2x; u2y = l2y;
        }
    }
    const bool matte = m_ok && (kind == MK_LAMBERT || kind == MK_OREN_NAYAR || kind == MK_BLACK);
    const bool tex_ok = tex != 0u && tex - 1u < a.n_textures;
    const float pu0 = u0x * b0, pu1 = u1x * b1, pu2 = u2x * b2;
    const float pv0 = u0y * b0, pv1 = u1y * b1, pv2 = u2y * b2;
    const float u = (pu0 + pu1) + pu2;
    const float v = (pv0 + pv1) + pv2;
    // hops 3 and 4: the texture's info and the texel
    RGB tx = RGB{1.0f, 1.0f, 1.0f};
    if (a.n_textures != 0u) tx = texture_eval(sc, tex_ok ? tex - 1u : 0u, u, v);
    const bool plain = matte && tex == 0u;
    const bool textured = matte && tex_ok && tri;
    out[0] = plain ? kd0 : (textured ? tx.r : 1.0f);
    out[1] = plain ? kd1 : (textured ? tx.g : 1.0f);
    out[2] = plain ? kd2 : (textured ? tx.b : 1.0f);
    out[3] = (plain || textured) ? 1.0f : 0.0f;
}

// ---- the demodulated denoise (yk_denoise_albedo): yk_denoise's rule with a division before and a product after
//
// Divisor of one channel with albedo a:  a where a is finite and a >= YK_ALBEDO_FLOOR;  1 where a is NaN or infinite;
// YK_ALBEDO_FLOOR otherwise (0, -0, negative and tiny albedos: a dark texel does not blow the quotient up by more than
// 64).  `known` is not read: the records that are not demodulated are all ones.
YK_HD float al_divisor(float a) {
    if (a != a || a == __builtin_inff() || a == -__builtin_inff()) return 1.0f;
    return a >= YK_ALBEDO_FLOOR ? a : YK_ALBEDO_FLOOR;
}
// In: after dn_normalise each channel is divided by its divisor, once per pixel.  The iterations run on these colours, so
// sigma_color acts on demodulated radiance.
YK_HD void al_demodulate(const float* albedo, float* c) {
    c[0] = dn_canon(c[0] / al_divisor(albedo[0]));
    c[1] = dn_canon(c[1] / al_divisor(albedo[1]));
    c[2] = dn_canon(c[2] / al_divisor(albedo[2]));
}
// Out: the last iteration's sum(w * c_Q) / sum(w) (dn_pixel's output) times the pixel's OWN divisor.
YK_HD void al_remodulate(const float* albedo, float* c) {
    c[0] = dn_canon(c[0] * al_divisor(albedo[0]));
    c[1] = dn_canon(c[1] * al_divisor(albedo[1]));
    c[2] = dn_canon(c[2] * al_divisor(albedo[2]));
}
// iterations == 0 returns the normalised film, copied as bits: no division and no product.

// ---- the pixel-mean albedo (yk_albedo_mean): the mean of al_pixel over an s x s grid of sub-pixel rays
//
// Sub-samples.  Output pixel (x, y) of a res_x x res_y film covers the s x s block of pixels (s*x + i, s*y + j), i, j =
// 0..s-1, of the (s*res_x) x (s*res_y) film of the same view: the film of yk_camera_init with res = (s*res_x, s*res_y) and
// otherwise the same parameters, whose pixel-centre rays yk_render_guides_ids traces.  `ids_ss` holds that film's id
// records, row-major, s*a.res_x to a row; a.res_x and a.res_y are the OUTPUT film's.  1 <= s <= 8.
// Per sub-sample: al_pixel's record of its id, all six cases; an unknown one is (1, 1, 1, 0) and enters the sum as ones.
// Mean, per channel: the first value (j = 0, i = 0) as it is, then every further one added to it in binary32, j outer and
// i inner, left to right, every addition separate; then ONE correctly rounded division by (float)(s*s), and dn_canon of
// the quotient (a NaN the sum or the division produces is 0x7fc00000).  s == 1: no addition and no division — the one
// record is copied, bit for bit yk_surface_albedo's.
// known = 1.0f if any sub-sample is known, else 0.0f; s*s ones sum to s*s exactly and (float)(s*s) / (float)(s*s) is 1, so a
// block of unknown sub-samples comes out as (1, 1, 1, 0) exactly.
// The loop bounds are the same for every lane, every id index lies inside the film and al_pixel clamps the rest: no load
// stands under a per-lane branch.
// An id record as four words: one 16-byte load of the device's records (16-byte aligned), four fields of a host array's.
YK_HD uint4 al_id(const uint4* p) { return *p; }
YK_HD uint4 al_id(const yk_surface_id* p) { return make_uint4(p->shape, __builtin_bit_cast(uint32_t, p->b[0]), __builtin_bit_cast(uint32_t, p->b[1]), __builtin_bit_cast(uint32_t, p->b[2])); }
template <class Id> YK_HD void al_mean_pixel(const AlParams& a, const DevScene& sc, const Id* ids_ss, uint32_t x, uint32_t y, uint32_t s, float* out) {
    const size_t row = (size_t)s * a.res_x;  // records to a row of the large film
    float sum0 = 0.0f, sum1 = 0.0f, sum2 = 0.0f;
    bool any = false;
    for (uint32_t j = 0; j < s; ++j) {
        const Id* line = ids_ss + ((size_t)s * y + j) * row + (size_t)s * x;
        for (uint32_t i = 0; i < s; ++i) {
            const uint4 id = al_id(line + i);
            float rec[4];
            al_pixel(a, sc, id.x, __builtin_bit_cast(float, id.y), __builtin_bit_cast(float, id.z), __builtin_bit_cast(float, id.w), rec);
            const bool first = j == 0u && i == 0u;
            sum0 = first ? rec[0] : sum0 + rec[0];
            sum1 = first ? rec[1] : sum1 + rec[1];
            sum2 = first ? rec[2] : sum2 + rec[2];
            any = any || rec[3] != 0.0f;
        }
    }
    if (s != 1u) {
        const float n = (float)(s * s);
        sum0 = dn_canon(sum0 / n);
        sum1 = dn_canon(sum1 / n);
        sum2 = dn_canon(sum2 / n);
    }
    out[0] = sum0;
    out[1] = sum1;
    out[2] = sum2;
    out[3] = any ? 1.0f : 0.0f;
}

// The two device steps of the fused route (yk_render_albedo_mean), defined in yk_albedo.hip and driven band by band from
// yk_render.cpp.  launch_ids_band: k_guides_ids' id record of every traced camera ray of the rows [row0, row0 + rows) of a
// res_x-wide film, written at (y - row0) * res_x + x of a band buffer instead of at its place in the whole film.
void launch_ids_band(hipStream_t s, const DevScene& sc, PathBuffers cur, const int* hit_tri, uint32_t n, const uint32_t* pixel_xy, uint32_t res_x, uint32_t row0, uint32_t rows, uint4* ids);

}  // namespace yk
