// The pixel-mean albedo rule (yuki_amd/csrc/yk_albedo.h, al_mean_pixel) on arrays as short as they can be — one triangle,
// one material, one mesh, one 1 x 1 texture, and id films of exactly (s*res_x) * (s*res_y) records, all on the heap — under
// ids that are out of range, for s = 1 and s = 3: the mean of the constant records comes back and, under AddressSanitizer,
// nothing past an array is read (the last block of the last row ends at the last record).  Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tools/asan/albedo_mean_rule.cpp -o /tmp/albedo_mean_rule && /tmp/albedo_mean_rule
#include <cstdio>
#include <cstring>
#include <vector>
#include "yk_albedo.h"
using namespace yk;
int main() {
    std::vector<uint32_t> indices{0, 1, 2}, tri_mesh{0}, mesh_flags{0};
    std::vector<int32_t> tri_material{0};
    std::vector<Material> mats(1);
    std::memset(mats.data(), 0, sizeof(Material));
    mats[0].kind = MK_LAMBERT; mats[0].a[0] = 0.25f; mats[0].a[1] = 0.5f; mats[0].a[2] = 0.75f;
    DevScene sc{};
    sc.indices = indices.data(); sc.tri_mesh = tri_mesh.data(); sc.tri_material = tri_material.data();
    sc.mesh_flags = mesh_flags.data(); sc.materials = mats.data();
    const uint32_t shapes[] = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    const uint32_t res_x = 3, res_y = 2;
    int bad = 0;
    for (uint32_t s : {1u, 3u}) {
        AlParams a{}; a.res_x = res_x; a.res_y = res_y; a.n_triangles = 1; a.n_shapes = 1; a.n_vertices = 3; a.n_meshes = 1; a.n_materials = 1; a.n_textures = 0; a.has_uvs = 0;
        const size_t n_ss = (size_t)s * res_x * s * res_y;
        // every record out of range but one per block, at a place that moves from block to block
        std::vector<yk_surface_id> ids(n_ss);
        for (size_t k = 0; k < n_ss; ++k) ids[k] = yk_surface_id{shapes[1 + k % 6], {0.3f, 0.3f, 0.4f}};
        for (uint32_t y = 0; y < res_y; ++y)
            for (uint32_t x = 0; x < res_x; ++x) {
                const uint32_t place = (x + 2 * y) % (s * s);
                ids[((size_t)s * y + place / s) * (s * res_x) + (size_t)s * x + place % s].shape = 0u;
            }
        for (uint32_t y = 0; y < res_y; ++y)
            for (uint32_t x = 0; x < res_x; ++x) {
                float r[4];
                al_mean_pixel(a, sc, ids.data(), x, y, s, r);
                const float n = (float)(s * s);
                // s*s - 1 ones and one Kd, in some order: every partial sum is exact here (quarters below 16)
                const float want[3] = {((n - 1.0f) + 0.25f) / n, ((n - 1.0f) + 0.5f) / n, ((n - 1.0f) + 0.75f) / n};
                if (r[3] != 1.0f || r[0] != want[0] || r[1] != want[1] || r[2] != want[2]) ++bad;
                std::printf("s %u pixel (%u, %u) -> %g %g %g %g\n", s, x, y, r[0], r[1], r[2], r[3]);
            }
        // all out of range: (1, 1, 1, 0) exactly
        for (size_t k = 0; k < n_ss; ++k) ids[k].shape = shapes[1 + k % 6];
        for (uint32_t y = 0; y < res_y; ++y)
            for (uint32_t x = 0; x < res_x; ++x) {
                float r[4];
                al_mean_pixel(a, sc, ids.data(), x, y, s, r);
                if (r[0] != 1.0f || r[1] != 1.0f || r[2] != 1.0f || r[3] != 0.0f) ++bad;
            }
        // material and texture indices out of range under the mean, NaN and infinite barycentrics
        tri_material[0] = 7;
        for (size_t k = 0; k < n_ss; ++k) ids[k] = yk_surface_id{0u, {__builtin_nanf(""), 1e30f, -__builtin_inff()}};
        float r[4];
        al_mean_pixel(a, sc, ids.data(), res_x - 1, res_y - 1, s, r);
        if (r[3] != 0.0f || r[0] != 1.0f) ++bad;
        tri_material[0] = 0;
        std::vector<float4> texels{make_float4(0.1f, 0.2f, 0.3f, 0.0f)};
        std::vector<uint4> info{make_uint4(0, 1, 1, 0)};
        sc.texels = texels.data(); sc.tex_info = info.data(); a.n_textures = 1;
        mats[0].tex = 1;
        al_mean_pixel(a, sc, ids.data(), res_x - 1, res_y - 1, s, r);
        if (r[3] != 1.0f || (s == 1u && r[0] != 0.1f)) ++bad;
        mats[0].tex = 9;
        al_mean_pixel(a, sc, ids.data(), res_x - 1, res_y - 1, s, r);
        if (r[3] != 0.0f) ++bad;
        mats[0].tex = 0;
        sc.texels = nullptr; sc.tex_info = nullptr;
    }
    std::printf("bad = %d\n", bad);
    return bad;
}
