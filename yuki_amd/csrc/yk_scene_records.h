// yk_scene_records.h — the host layout of a scene's device records, a function of its input: creation fills
// it from the description, a host-route update from what it fetched; the device layout is held against it byte for byte.
#pragma once
#include <cstdint>
#include <vector>

#include "yk_device.h"
#include "yk_host.h"

// The context's "top_nodes" and "wide_bvh" as they stood when the scene was created: both layouts read this copy, at
// creation and at every update (yk_scene::UpdateState).
struct LayoutOptions {
    int64_t top_nodes = 0, wide_bvh = 0;
};

// Everything the host layout reads.  All arrays are host memory and borrowed for the call.
struct HostLayoutInput {
    const yk::HostBvh* bvh = nullptr;  // nodes, shape order and depth
    uint64_t n_interior = 0;
    const uint32_t* indices = nullptr;
    const float *points = nullptr, *normals = nullptr, *uvs = nullptr;  // normals, uvs: NULL where the scene has none
    const int32_t *tri_material = nullptr, *tri_area_light = nullptr;   // tri_area_light: -1 where there is none
    const uint32_t *tri_mesh = nullptr, *mesh_flags = nullptr;          // mesh_flags: YK_MESH_* per mesh
    uint32_t n_triangles = 0;
    const int32_t* sphere_material = nullptr;  // one material index per sphere
    const uint8_t* mat_kind = nullptr;         // device BSDF kind (MK_*) per material
    LayoutOptions opt;
};

// The seven record arrays in the order of YK_RECORDS_*, and the two words of the layout's head that only the layout knows.
struct SceneRecords {
    std::vector<yk::DevNode> nodes;
    std::vector<yk::DevNode4> nodes4;
    std::vector<yk::DevNode> top, top_any;
    std::vector<float4> tris;
    std::vector<uint4> prim_shade;
    std::vector<float4> prim_attr;
    uint32_t root_ref = 0;
    bool wide_auto = false;
};

SceneRecords layout_records_host(const HostLayoutInput& in);
