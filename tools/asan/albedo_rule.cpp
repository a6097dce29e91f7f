// The albedo rule (yuki_amd/csrc/yk_albedo.h, al_pixel) on arrays as short as they can be — one triangle, one material, one
// mesh, one 1 x 1 texture, all on the heap — under ids, material indices and texture indices that are out of range: the
// constant record comes back and, under AddressSanitizer, nothing past an array is read.  Stand-alone, host only:
//   cd yuki_amd/csrc && hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I. \
//       ../../tools/asan/albedo_rule.cpp -o /tmp/albedo_rule && /tmp/albedo_rule
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
    AlParams a{}; a.res_x = 1; a.res_y = 1; a.n_triangles = 1; a.n_shapes = 1; a.n_vertices = 3; a.n_meshes = 1; a.n_materials = 1; a.n_textures = 0; a.has_uvs = 0;
    const uint32_t shapes[] = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    int bad = 0;
    for (uint32_t s : shapes) {
        float r[4];
        al_pixel(a, sc, s, 0.3f, 0.3f, 0.4f, r);
        const bool want_known = s == 0u;
        if ((r[3] == 1.0f) != want_known || (!want_known && (r[0] != 1.0f || r[1] != 1.0f || r[2] != 1.0f))) ++bad;
        std::printf("shape %08x -> %g %g %g %g\n", s, r[0], r[1], r[2], r[3]);
    }
    // a material index out of range and a textured scene with a texture index out of range
    tri_material[0] = 7;
    float r[4];
    al_pixel(a, sc, 0u, 0.3f, 0.3f, 0.4f, r);
    if (r[3] != 0.0f) ++bad;
    tri_material[0] = -1;
    al_pixel(a, sc, 0u, 0.3f, 0.3f, 0.4f, r);
    if (r[3] != 0.0f) ++bad;
    tri_material[0] = 0;
    std::vector<float4> texels{make_float4(0.1f, 0.2f, 0.3f, 0.0f)};
    std::vector<uint4> info{make_uint4(0, 1, 1, 0)};
    sc.texels = texels.data(); sc.tex_info = info.data(); a.n_textures = 1;
    mats[0].tex = 1;
    al_pixel(a, sc, 0u, 0.3f, 0.3f, 0.4f, r);
    if (r[3] != 1.0f || r[0] != 0.1f) ++bad;
    mats[0].tex = 9;
    al_pixel(a, sc, 0u, __builtin_nanf(""), 1e30f, -__builtin_inff(), r);
    if (r[3] != 0.0f) ++bad;
    std::printf("bad = %d\n", bad);
    return bad;
}
