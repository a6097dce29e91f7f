// The rule of yk_scene_transform (yuki_amd/csrc/yk_scene_transform.h) over random triangle soups on heap arrays of exactly
// their size: under AddressSanitizer nothing reads or writes past an array, under UBSan nothing in the arithmetic is
// undefined.  Checks on the way: the table vertex -> mesh against a brute-force search over the triangles, with unreferenced
// and shared vertices; a record that equals the identity (with -0 entries) gives the rest pose's BITS — negative zeros, NaN
// payloads and infinities included — and never reads world_to_rest (which is poisoned); a moved record gives xf_point /
// xf_normal recomputed here from the statement, with the w == 1 test; a vertex of no mesh, or of a mesh out of range, keeps
// its bits; the kinds, the flag flip and each refusal bit with the precedence of refusal(); and the tree cost against a
// long double sum, 0 for a root without area, 1 for a single leaf of one shape.
// Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tests/cpp/transform_rule.cpp -o /tmp/transform_rule && /tmp/transform_rule
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_scene_transform.h"
using namespace yk;
using namespace yk::xfm;

static uint32_t lcg_state = 20261021u;
static uint32_t lcg() { return lcg_state = lcg_state * 1664525u + 1013904223u; }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) { return __builtin_bit_cast(uint32_t, f); }
static bool same3(V3 a, V3 b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

static void identity(float* m) {
    for (int k = 0; k < 16; ++k) m[k] = (k % 5) == 0 ? 1.0f : 0.0f;
}

static int table_against_brute_force() {
    int bad = 0;
    for (int round = 0; round < 200; ++round) {
        const uint32_t nv = 1u + lcg() % 40u, nt = lcg() % 30u, nm = 1u + lcg() % 4u;
        std::vector<uint32_t> idx(3 * (size_t)nt), tm(nt), vm(2 * (size_t)nv);
        for (auto& i : idx) i = lcg() % nv;
        for (auto& m : tm) m = lcg() % nm;
        for (uint32_t v = 0; v < nv; ++v) {
            vm[2 * (size_t)v] = XF_NO_MESH;
            vm[2 * (size_t)v + 1] = 0u;
        }
        for (uint32_t t = 0; t < nt; ++t)
            for (int k = 0; k < 3; ++k) table_add(vm.data(), idx[3 * (size_t)t + k], tm[t]);
        for (uint32_t v = 0; v < nv; ++v) {
            uint32_t lo = XF_NO_MESH, hi = 0u;
            bool used = false;
            for (uint32_t t = 0; t < nt; ++t)
                for (int k = 0; k < 3; ++k)
                    if (idx[3 * (size_t)t + k] == v) {
                        used = true;
                        if (tm[t] < lo) lo = tm[t];
                        if (tm[t] > hi) hi = tm[t];
                    }
            if (vm[2 * (size_t)v] != lo || vm[2 * (size_t)v + 1] != hi) ++bad;
            if (vertex_shared(vm[2 * (size_t)v], vm[2 * (size_t)v + 1]) != (used && lo != hi)) ++bad;
            if (!used && vm[2 * (size_t)v] != XF_NO_MESH) ++bad;
        }
    }
    std::printf("the table against a search: bad = %d\n", bad);
    return bad;
}

static int vertex_rule() {
    int bad = 0;
    const float pool[] = {-0.0f, 0.0f, __builtin_nanf("0x1234"), __builtin_inff(), -__builtin_inff(), 1e30f, -7.5f, 0.1f};
    for (int round = 0; round < 400; ++round) {
        const uint32_t nm = 1u + lcg() % 5u;
        std::vector<float> rec(XF_RECORD_FLOATS * (size_t)nm);
        std::vector<uint32_t> kinds(nm);
        for (uint32_t m = 0; m < nm; ++m) {
            float* r = rec.data() + XF_RECORD_FLOATS * (size_t)m;
            const uint32_t what = lcg() % 4u;
            identity(r);
            identity(r + 16);
            if (what == 0u) {  // the identity, some zeros negative, the inverse poisoned: it is never read
                for (int k = 0; k < 16; ++k)
                    if ((k % 5) != 0 && lcg() % 2u) r[k] = -0.0f;
                for (int k = 16; k < 32; ++k) r[k] = __builtin_nanf("");
            } else {
                for (int k = 0; k < 12; ++k) r[k] = 4.0f * unit() - 2.0f;
                for (int k = 16; k < 28; ++k) r[k] = 4.0f * unit() - 2.0f;
                if (what == 2u) r[15] = 2.0f;                 // w = 2: the division
                if (what == 3u) r[12] = 0.25f * unit();       // a projective row
            }
            uint32_t flag;
            kinds[m] = mesh_kind(r, false, &flag);
            if ((what == 0u) != (kinds[m] == 0u) || flag != 0u) ++bad;
            if (what != 0u && ((kinds[m] & XF_FLIPS) != 0u) != inp::swaps_handedness(r)) ++bad;
            if (mesh_flags_of(YK_MESH_SWAPS | 1u, kinds[m]) != ((kinds[m] & XF_FLIPS) ? 1u : (YK_MESH_SWAPS | 1u))) ++bad;
        }
        for (int v = 0; v < 64; ++v) {
            const V3 p{lcg() % 4u ? 8.0f * unit() - 4.0f : pool[lcg() % 8u], lcg() % 4u ? 8.0f * unit() - 4.0f : pool[lcg() % 8u], lcg() % 4u ? 8.0f * unit() - 4.0f : pool[lcg() % 8u]};
            const uint32_t pick = lcg() % (nm + 2u);
            const uint32_t mesh = pick < nm ? pick : (pick == nm ? XF_NO_MESH : nm);  // none, or out of range: the rest bits
            const V3 q = vertex_point(rec.data(), kinds.data(), nm, mesh, p), n = vertex_normal(rec.data(), kinds.data(), nm, mesh, p);
            if (mesh >= nm || kinds[mesh] == 0u) {
                if (!same3(q, p) || !same3(n, p) || vertex_moves(kinds.data(), nm, mesh)) ++bad;
                continue;
            }
            const float* r = rec.data() + XF_RECORD_FLOATS * (size_t)mesh;
            float row[4];
            for (int k = 0; k < 4; ++k) {
                float s = r[4 * k] * p.x;
                s = s + r[4 * k + 1] * p.y;
                s = s + r[4 * k + 2] * p.z;
                row[k] = s + r[4 * k + 3];
            }
            const V3 want = row[3] == 1.0f ? V3{row[0], row[1], row[2]} : V3{row[0] / row[3], row[1] / row[3], row[2] / row[3]};
            const float* ri = r + 16;
            const V3 want_n{ri[0] * p.x + ri[4] * p.y + ri[8] * p.z, ri[1] * p.x + ri[5] * p.y + ri[9] * p.z, ri[2] * p.x + ri[6] * p.y + ri[10] * p.z};
            // a NaN the arithmetic produces may differ in its sign: compare those as NaNs
            const auto eq = [](float a, float b) { return (a != a && b != b) || bits(a) == bits(b); };
            if (!eq(q.x, want.x) || !eq(q.y, want.y) || !eq(q.z, want.z) || !eq(n.x, want_n.x) || !eq(n.y, want_n.y) || !eq(n.z, want_n.z)) ++bad;
            const bool nf = !std::isfinite(q.x) || !std::isfinite(q.y) || !std::isfinite(q.z);
            if (point_not_finite(q) != nf) ++bad;
        }
    }
    std::printf("the per-vertex rule: bad = %d\n", bad);
    return bad;
}

static int refusals() {
    int bad = 0;
    float r[XF_RECORD_FLOATS];
    uint32_t flag;
    identity(r);
    identity(r + 16);
    if (mesh_kind(r, true, &flag) != 0u || flag != 0u) ++bad;  // a lit mesh that stays
    r[3] = 1.0f;
    if (mesh_kind(r, true, &flag) != XF_MOVED || flag != XF_BAD_LIT) ++bad;
    if (mesh_kind(r, false, &flag) != XF_MOVED || flag != 0u) ++bad;
    r[0] = -1.0f;
    if (mesh_kind(r, false, &flag) != (XF_MOVED | XF_FLIPS) || flag != 0u) ++bad;
    for (int k = 0; k < XF_RECORD_FLOATS; ++k)
        for (float v : {__builtin_nanf(""), __builtin_inff(), -__builtin_inff()}) {
            float s[XF_RECORD_FLOATS];
            std::memcpy(s, r, sizeof(s));
            s[k] = v;
            (void)mesh_kind(s, true, &flag);
            if (flag != (XF_BAD_MATRIX | XF_BAD_LIT)) ++bad;
        }
    identity(r);  // rest_to_world the identity: the inverse is not tested either
    r[20] = __builtin_nanf("");
    if (mesh_kind(r, false, &flag) != 0u || flag != 0u) ++bad;
    for (uint32_t f = 1u; f < 16u; ++f) {
        const char* want = (f & 1u) ? "transforms: matrix entry not finite" : (f & 2u) ? "transforms: a mesh that carries an area light cannot move" : (f & 4u) ? "transforms: vertex shared by two meshes" : "points: coordinate not finite";
        if (std::strcmp(refusal(f), want) != 0) ++bad;
    }
    std::printf("kinds and refusals: bad = %d\n", bad);
    return bad;
}

static int cost() {
    int bad = 0;
    for (int round = 0; round < 200; ++round) {
        const size_t n = 1u + lcg() % 300u;
        std::vector<uint32_t> nodes(8 * n);
        long double interior = 0.0L, leaf = 0.0L;
        for (size_t i = 0; i < n; ++i) {
            float lo[3], hi[3];
            for (int k = 0; k < 3; ++k) {
                lo[k] = 20.0f * unit() - 10.0f;
                hi[k] = lo[k] + 5.0f * unit();
            }
            const bool is_leaf = lcg() % 2u;
            const uint32_t count = 1u + lcg() % 4u;
            for (int k = 0; k < 3; ++k) {
                nodes[8 * i + k] = bits(lo[k]);
                nodes[8 * i + 3 + k] = bits(hi[k]);
            }
            nodes[8 * i + 6] = lcg();
            nodes[8 * i + 7] = (is_leaf ? 1u << 24 : 0u) | ((lcg() % 3u) << 16) | count;
            const long double dx = (long double)hi[0] - lo[0], dy = (long double)hi[1] - lo[1], dz = (long double)hi[2] - lo[2];
            const long double a = 2.0L * (dx * dy + dy * dz + dz * dx);
            (is_leaf ? leaf : interior) += is_leaf ? a * count : a;
        }
        const double got = tree_cost(nodes.data(), n), root = node_area(nodes.data(), 0u);
        const long double want = root > 0.0 ? (interior + leaf) / (long double)root : 0.0L;
        if (!(std::fabs((double)(got - want)) <= (double)n * 0x1p-51 * (double)want)) ++bad;
    }
    uint32_t one[8] = {bits(0.0f), bits(0.0f), bits(0.0f), bits(1.0f), bits(2.0f), bits(3.0f), 0u, (1u << 24) | 1u};
    if (tree_cost(one, 1) != 1.0) ++bad;  // a single leaf of one shape
    one[3] = one[4] = one[5] = bits(0.0f);
    if (tree_cost(one, 1) != 0.0) ++bad;  // a root without area
    if (tree_cost(one, 0) != 0.0) ++bad;
    std::printf("the tree cost: bad = %d\n", bad);
    return bad;
}

int main() {
    const int bad = table_against_brute_force() + vertex_rule() + refusals() + cost();
    std::printf("transform rule: bad = %d\n", bad);
    return bad != 0;
}
