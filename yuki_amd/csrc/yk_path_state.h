// yk_path_state.h — what a lane carries from one bounce to the next, and the only code that knows how it is packed.
//
// HBM layout of the path state (PathBuffers, ping-pong, compacted every bounce by `k_shade`): four arrays of 16-byte
// words, so every lane moves one dwordx4 and a wave one contiguous KiB ("SoA of float4"):
//
//     rayO[i] = (o.x, o.y, o.z, bits(flags))        flags: bounces | specular<<8
//     rayD[i] = (d.x, d.y, d.z, bits(sample_id))    sample_id = index into sample_buf
//     thru[i] = (beta.r, beta.g, beta.b, bits(sampler dimension))
//     rngs[i] = (state.lo, state.hi, inc.lo, inc.hi)          PCG32 stream of the pixel
//
// The lean camera bounce (yk_device.h, YK_CTRL_CAM_O) stores rayD and rngs only: one origin for all, throughput one, the
// camera sample's two dimensions drawn.  The stage entry points and yk_li read and write the same four arrays.
#pragma once
#include "yk_device.h"
#include "yk_math.h"
#include "yk_rng.h"

namespace yk {

struct PathState {
    V3 o, d;
    RGB beta;
    unsigned bounces;
    bool specular;  // the last BSDF sample was a specular lobe
    unsigned sid;   // sample id
    unsigned dimension;
    Pcg rng;
};
// the four 16-byte words of a PathState
struct PathWords {
    float4 O, D, T;
    uint4 R;
};

__device__ __forceinline__ uint4 pcg_pack(const Pcg& r) { return make_uint4((unsigned)r.state, (unsigned)(r.state >> 32), (unsigned)r.inc, (unsigned)(r.inc >> 32)); }
__device__ __forceinline__ Pcg pcg_unpack(uint4 w) {
    Pcg r;
    r.state = (u64)w.x | ((u64)w.y << 32);
    r.inc = (u64)w.z | ((u64)w.w << 32);
    return r;
}

// what a kernel that needs one field reads: one 16-byte load, not four
__device__ __forceinline__ unsigned path_sample_id(float4 rayD_word) { return __float_as_uint(rayD_word.w); }
__device__ __forceinline__ RGB path_beta(float4 thru_word) { return RGB{thru_word.x, thru_word.y, thru_word.z}; }
// the origin word of ray i: rayO == null on the lean camera bounce, every ray starts at *lean_origin
__device__ __forceinline__ float4 path_origin_word(const float4* __restrict__ rayO, unsigned i, const float4* __restrict__ lean_origin) {
    return rayO ? rayO[i] : *lean_origin;
}

__device__ __forceinline__ PathState path_unpack(float4 O, float4 D, float4 T, uint4 R) {
    PathState s;
    s.o = V3{O.x, O.y, O.z};
    s.d = V3{D.x, D.y, D.z};
    s.beta = path_beta(T);
    const unsigned flags = __float_as_uint(O.w);
    s.bounces = flags & 0xffu;
    s.specular = (flags >> 8) & 1u;
    s.sid = path_sample_id(D);
    s.dimension = __float_as_uint(T.w);
    s.rng = pcg_unpack(R);
    return s;
}
__device__ __forceinline__ PathState path_load(const PathBuffers& b, unsigned i) { return path_unpack(b.rayO[i], b.rayD[i], b.thru[i], b.rngs[i]); }
// `lean_origin` != null (a kernel argument: a wave-uniform branch): the lean camera bounce
__device__ __forceinline__ PathState path_load(const PathBuffers& b, unsigned i, const float4* __restrict__ lean_origin) {
    float4 O, T;
    const float4 D = b.rayD[i];
    if (lean_origin) {
        O = *lean_origin;
        T = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(2u));
    } else {
        O = b.rayO[i];
        T = b.thru[i];
    }
    return path_unpack(O, D, T, b.rngs[i]);
}

__device__ __forceinline__ PathWords path_pack(const PathState& s) {
    PathWords w;
    w.O = make_float4(s.o.x, s.o.y, s.o.z, __uint_as_float((s.bounces & 0xffu) | (s.specular ? 0x100u : 0u)));
    w.D = make_float4(s.d.x, s.d.y, s.d.z, __uint_as_float(s.sid));
    w.T = make_float4(s.beta.r, s.beta.g, s.beta.b, __uint_as_float(s.dimension));
    w.R = pcg_pack(s.rng);
    return w;
}
__device__ __forceinline__ void path_store(const PathBuffers& b, unsigned i, const PathWords& w) {
    b.rayO[i] = w.O;
    b.rayD[i] = w.D;
    b.thru[i] = w.T;
    b.rngs[i] = w.R;
}
// a camera ray as raygen leaves it: no bounce yet, throughput one.  `lean_origin` != null: the lean camera bounce — the
// origin goes there once (lane `first`), rayO and thru are not stored
__device__ __forceinline__ void path_store_camera(const PathBuffers& b, unsigned i, V3 o, V3 d, unsigned sid, const SamplerState& st, float4* lean_origin,
                                                  bool first) {
    PathState s;
    s.o = o;
    s.d = d;
    s.beta = RGB{1.0f, 1.0f, 1.0f};
    s.bounces = 0;
    s.specular = false;
    s.sid = sid;
    s.dimension = st.dimension;
    s.rng = st.rng;
    const PathWords w = path_pack(s);
    if (lean_origin) {
        if (first) *lean_origin = w.O;
        b.rayD[i] = w.D;
        b.rngs[i] = w.R;
    } else {
        path_store(b, i, w);
    }
}

// a lane without a path: never stored, the defaults keep its registers defined
__device__ __forceinline__ PathState path_inert() {
    PathState s;
    s.o = V3{0, 0, 0};
    s.d = V3{0, 0, 1};
    s.beta = RGB{0, 0, 0};
    s.bounces = 0;
    s.specular = false;
    s.sid = 0;
    s.dimension = 0;
    s.rng.state = 0;
    s.rng.inc = 1;
    return s;
}
__device__ __forceinline__ SamplerState sampler_inert() {
    SamplerState st;
    st.rng.state = 0;
    st.rng.inc = 1;
    st.px = st.py = st.sample_index = st.dimension = 0;
    return st;
}

// The sampler state a path carries: the PCG32 stream, the next dimension and the sample id, whose pixel-table entry gives
// the pixel and the sample index.
__device__ __forceinline__ SamplerState path_sampler(const RenderParams& prm, const uint32_t* pixel_xy, const uint32_t* sample_index_tab, const PathState& s) {
    SamplerState st;
    st.rng = s.rng;
    st.dimension = s.dimension;
    uint32_t pix, ks;  // entry of the pixel table and sample within it (yk_device.h: RenderParams::spe)
    split_sample_id(s.sid, prm.spe, pix, ks);
    const uint32_t xy = pixel_xy[pix];
    st.px = xy & 0xffffu;
    st.py = xy >> 16;
    st.sample_index = (sample_index_tab ? sample_index_tab[pix] : prm.sample_base) + ks;
    return st;
}

}  // namespace yk
