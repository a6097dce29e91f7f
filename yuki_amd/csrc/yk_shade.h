// yk_shade.h — one vertex of Path::li_internal (integrators/path.rs:89-169) as three inline steps.
//
// `k_shade` (yk_kernels.hip) runs them once per bounce over every in-flight path — vertex_setup, vertex_light for every
// light, vertex_finish — and `k_accumulate` ends the vertex with vertex_accumulate once the any-hit verdicts are in.  The
// order is the reference's: two sampler dimensions per light whether or not it contributes, then the BSDF sample, then
// Russian roulette; every expression keeps its operation order.  (A per-lane kernel that took the last few paths of a
// batch to their end with the same four steps was measured and dropped: profiles/r02_tail_kernel_sweep.txt)
// `k_path_debug` (yk_trace.hip) runs the same steps one lane per sample for yk_li_debug.
#pragma once
#include "yk_device.h"
#include "yk_geom.h"
#include "yk_path_state.h"
#include "yk_rng.h"

namespace yk {

// what path.rs:89-101 has in hand after `scene.bvh.intersect`: the SurfaceInteraction and its Bsdf
struct PathVertex {
    Surface sf;
    Material mat;
    Frame fr;
    V3 wo;
};

// what a lane without a hit carries through the steps: it never reads the vertex, the defaults keep its registers defined
__device__ __forceinline__ PathVertex vertex_inert() {
    PathVertex v;
    v.sf.p = v.sf.n = v.sf.ns = v.sf.dpdus = v.sf.wo = V3{0, 0, 1};
    v.sf.material = 0;
    v.sf.area_light = -1;
    v.sf.u = v.sf.v = 0.0f;
    v.mat.kind = MK_BLACK;
    v.fr.s = v.fr.t = v.fr.n = v.fr.ng = V3{0, 0, 1};
    v.wo = V3{0, 0, 1};
    return v;
}

// the rest of the vertex once v.sf holds the surface: material (with its texture), shading frame, wo
__device__ __forceinline__ void vertex_setup_material(const DevScene& sc, V3 d, PathVertex& v) {
    v.mat = sc.materials[v.sf.material];
    if (v.mat.tex) {  // matte.rs:29-30: reflectance = kd.evaluate(si); no lobe when black
        RGB kd = texture_eval(sc, v.mat.tex - 1u, v.sf.u, v.sf.v);
        v.mat.a[0] = kd.r;
        v.mat.a[1] = kd.g;
        v.mat.a[2] = kd.b;
        if (is_black(kd)) v.mat.kind = MK_BLACK;
    }
    v.fr = make_frame(v.sf.n, v.sf.ns, v.sf.dpdus);
    v.wo = -d;
}
// `prim`: leaf-order slot of the primitive that was hit (what the render-loop traversal kernels report)
__device__ __forceinline__ void vertex_setup(const DevScene& sc, uint32_t prim, V3 o, V3 d, PathVertex& v) {
    v.sf = hit_surface_prim(sc, prim, o, d);
    vertex_setup_material(sc, d, v);
}

// next-event estimation towards light l (path.rs:102-119): draws its two sampler dimensions, and when the light
// contributes returns the contribution f * li * clamp(ns . l) / pdf and the shadow ray of its VisibilityTester.
// RAY_ALWAYS (k_path_debug): the shadow ray is also returned when the light has a visibility tester but f is black
// (`has_ray`; path.rs:103-113 records that ray although it traces nothing).
//
// A contribution that is +-0 in every component (the light behind the shading normal, or the vertex seen and lit from the
// back) is added by the reference after a trace, and c + (+-0) is c bit for bit (c starts at +0; a sum is -0 only when both
// operands are): with prm.nee_skip & YK_NEE_SKIP_ZERO the ray is not wanted.  It still counts as a shadow ray of the render
// (`zero`: the reference calls `unoccluded` for it), and RAY_ALWAYS still reports it.  A NaN or an infinity is no zero.
struct NeeSample {
    bool want;
    bool has_ray;  // RAY_ALWAYS only: nothing is to be traced (f was black, or the contribution zero); so / sd hold the tester's ray
    bool zero;     // the reference traces a ray here that adds +-0: not wanted, but reported
    RGB contrib;
    V3 so, sd;
    int al;  // the sampled area light (its own surface does not occlude, bvh.rs:269-280) or -1
};
// VisibilityTester::ray = p0.spawn_ray_to(p1), interaction.rs:44-59
#define YK_SHADOW_T_MAX 0.9999f  // its t_max
__device__ __forceinline__ void vertex_shadow_ray(const PathVertex& v, const LightSample& ls, V3& so, V3& sd) {
    V3 offset = v.sf.n * 0.001f;
    so = dot(ls.p1 - v.sf.p, v.sf.n) > 0.0f ? v.sf.p + offset : v.sf.p - offset;
    sd = ls.p1 - so;
}
// "no sample": the light does not contribute (also what a lane without a vertex stages: nothing)
__device__ __forceinline__ NeeSample nee_none() {
    NeeSample r;
    r.want = false;
    r.has_ray = false;
    r.zero = false;
    r.contrib = RGB{0, 0, 0};
    r.so = V3{0, 0, 0};
    r.sd = V3{0, 0, 1};
    r.al = -1;
    return r;
}
// The two sampler dimensions of a light (path.rs:102, whitted.rs:113): consumed whether or not the light contributes, and
// whether or not it reads them — only a light that does (light_reads_sample, yk_geom.h) has their values computed, the
// others get zeros.  The light is the same for the whole wave: no lane disagrees about the branch.
__device__ __forceinline__ void light_draw_2d(const SamplerCfg& c, SamplerState& st, const DevLight& L, float& ux, float& uy) {
    ux = uy = 0.0f;  // only defines the outputs of a skipped draw; what keeps caller and callee together is sample_light's own gate
    if (light_reads_sample(L.kind))
        sampler_get_2d(c, st, ux, uy);
    else
        sampler_skip_2d(c, st);
}
template <bool RAY_ALWAYS = false>
__device__ __forceinline__ NeeSample vertex_light(const DevScene& sc, const RenderParams& prm, SamplerState& st, unsigned l, const PathVertex& v) {
    NeeSample r = nee_none();
    float ux, uy;
    light_draw_2d(prm.sampler, st, sc.lights[l], ux, uy);
    LightSample ls = sample_light(sc.lights[l], (int)l, v.sf.p, ux, uy);
    if (!is_black(ls.li)) {
        RGB f = bsdf_f(v.mat, v.fr, v.sf.wo, ls.l);  // path.rs:105 uses si.wo
        if (ls.has_vis && !is_black(f)) {
            r.contrib = f * ls.li * rclamp(dot_nv(v.sf.ns, ls.l), 0.0f, 1.0f) / ls.pdf;
            vertex_shadow_ray(v, ls, r.so, r.sd);
            r.al = ls.area_light;
            r.zero = (prm.nee_skip & YK_NEE_SKIP_ZERO) && is_black(r.contrib);
            r.want = !r.zero;
            if (RAY_ALWAYS) r.has_ray = r.zero;
        } else if (RAY_ALWAYS && ls.has_vis) {
            vertex_shadow_ray(v, ls, r.so, r.sd);
            r.has_ray = true;
        }
    }
    return r;
}

// kind bits of the pending term: 1 = miss, 2 = emission term present, 4 = indirect clamp applies
#define YK_PEND_MISS 1u
#define YK_PEND_EMISSION 2u
#define YK_PEND_CLAMP 4u
// pend[i].w = kind << 29 | (sample slot - first slot of the batch); batches hold at most 2^29 paths (yk_context_set_option)
#define YK_PEND_KIND_SHIFT 29
#define YK_PEND_SID_MASK 0x1fffffffu
// the sample's slot travels with the term (as its offset in the batch): k_accumulate reads no path state for it
__device__ __forceinline__ float4 pend_pack(RGB term, unsigned kind, unsigned slot) {
    return make_float4(term.r, term.g, term.b, __uint_as_float((kind << YK_PEND_KIND_SHIFT) | slot));
}
__device__ __forceinline__ unsigned pend_kind(float4 p) { return __float_as_uint(p.w) >> YK_PEND_KIND_SHIFT; }
__device__ __forceinline__ unsigned pend_slot(float4 p) { return __float_as_uint(p.w) & YK_PEND_SID_MASK; }

// path.rs:155-160: incoming_radiance += beta * scene.background; break
__device__ __forceinline__ RGB vertex_miss_term(const DevScene& sc, RGB beta) { return beta * RGB{sc.background[0], sc.background[1], sc.background[2]}; }

// the rest of the vertex after the light loop (path.rs:121-169): emission term, BSDF sample, throughput, Russian roulette.
// In: beta / bounces / specular_bounce as they entered the vertex.  Out: the pending term and its kind bits; `alive` and
// the continuation (origin, direction, updated beta / bounces / specular flag) — the continuation state is written
// whenever the BSDF sample was usable, also when roulette or max_depth then end the path, as the wavefront stores it.
struct VertexEnd {
    RGB term;
    unsigned kind;
    bool alive, sampled;
    V3 no, wi;
    unsigned lobe;  // BxdfType of the BSDF sample when `sampled` (k_path_debug tags the next segment with it)
};
__device__ __forceinline__ VertexEnd vertex_finish(const DevScene& sc, const RenderParams& prm, SamplerState& st, const PathVertex& v, RGB& beta, unsigned& bounces,
                                                    bool& specular_bounce) {
    VertexEnd e;
    e.term = RGB{0, 0, 0};
    e.kind = 0;
    e.alive = false;
    e.sampled = false;
    e.no = V3{0, 0, 0};
    e.wi = V3{0, 0, 1};
    e.lobe = 0;
    if (bounces == 0 || specular_bounce) {  // path.rs:121-123
        RGB le = RGB{0, 0, 0};
        if (v.sf.area_light >= 0) {
            const DevLight& L = sc.lights[v.sf.area_light];
            le = dot_nv(v.sf.n, v.wo) > 0.0f ? RGB{L.i[0], L.i[1], L.i[2]} : RGB{0, 0, 0};  // rectangular_light.rs:75-81
        }
        e.term = beta * le;
        e.kind |= YK_PEND_EMISSION;
    }
    if (bounces > 0 && prm.has_clamp) e.kind |= YK_PEND_CLAMP;
    // path.rs:131-145
    float ux, uy;
    sampler_get_2d(prm.sampler, st, ux, uy);
    BsdfSample bs = bsdf_sample_f(v.mat, v.fr, v.wo, ux, uy);
    if (!(is_black(bs.f) || bs.pdf == 0.0f)) {
        specular_bounce = (bs.type & BX_SPECULAR) != 0;
        beta = beta * (bs.f * fabsf(dot_nv(bs.wi, v.sf.ns)) / bs.pdf);
        e.no = spawn_origin(v.sf.p, v.sf.n, bs.wi);
        e.wi = bs.wi;
        e.lobe = bs.type;
        e.alive = true;
        e.sampled = true;
        // Russian roulette, path.rs:162-169
        if (bounces > 3) {
            float q = rmax(1.0f - beta.g, 0.05f);
            if (sampler_get_1d(prm.sampler, st) < q)
                e.alive = false;
            else
                beta = beta * (RGB{1.0f, 1.0f, 1.0f} / (1.0f - q));
        }
        bounces += 1;
        if (!(bounces < prm.max_depth)) e.alive = false;  // while bounces < max_depth
    }
    return e;
}

// `incoming_radiance += beta * radiance` of one vertex (path.rs:102-129), the fold a vertex ends with: `radiance` holds
// the unoccluded light contributions summed in light order; `beta` is the throughput the vertex was ENTERED with.
// vertex_addend is what the vertex adds to the sample, vertex_accumulate the sum.
__device__ __forceinline__ RGB vertex_addend(const RenderParams& prm, RGB beta, RGB radiance, RGB term, unsigned kind) {
    if (kind & YK_PEND_MISS) return term;
    if (kind & YK_PEND_EMISSION) radiance = radiance + term;
    if (kind & YK_PEND_CLAMP) radiance = rgb_min(radiance, RGB{1.0f, 1.0f, 1.0f} * prm.clamp);
    return beta * radiance;
}
__device__ __forceinline__ RGB vertex_accumulate(const RenderParams& prm, RGB L, RGB beta, RGB radiance, RGB term, unsigned kind) {
    return L + vertex_addend(prm, beta, radiance, term, kind);
}

}  // namespace yk
