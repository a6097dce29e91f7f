// yk_scene.cpp — scene description -> the reference's BVH (host) -> device records -> one copy per device.
// (yk_scene_create, bvh.rs:39-115 via yk_host.cpp; the record layouts are in yk_device.h and DESIGN.md §3.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "yk_internal.h"
#include "yk_scene_layout.h"
#include "yk_scene_update.h"

template <class T> static yk_status upload(yk_context* ctx, DevBuf& buf, const T* src, size_t count) {
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    HIP_TRY(ctx, buf.ensure(bytes));
    if (count) HIP_TRY(ctx, hipMemcpy(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return YK_OK;
}

Material make_material(const yk_material_desc& m) {
    Material r;
    std::memset(&r, 0, sizeof(r));
    for (int k = 0; k < 3; ++k) {
        r.a[k] = m.a[k];
        r.b[k] = m.b[k];
    }
    const bool remap = (m.flags & YK_MAT_FLAG_REMAP) != 0;
    const bool textured = m.kind == YK_MAT_MATTE && (m.flags & YK_MAT_FLAG_TEXTURED_A) != 0;
    r.tex = textured ? m.a_texture + 1u : 0u;
    switch (m.kind) {
        case YK_MAT_MATTE: {  // matte.rs:27-39 (a textured Kd is tested for black per hit)
            if (!textured && m.a[0] == 0.0f && m.a[1] == 0.0f && m.a[2] == 0.0f) {
                r.kind = MK_BLACK;
            } else if (m.c == 0.0f) {
                r.kind = MK_LAMBERT;
            } else {  // oren_nayar.rs:20-27
                r.kind = MK_OREN_NAYAR;
                float sigma2 = m.c * m.c;
                r.c = 1.0f - (sigma2 / (2.0f * (sigma2 + 0.33f)));
                r.d = 0.45f * sigma2 / (sigma2 + 0.09f);
            }
            break;
        }
        case YK_MAT_GLASS:
            r.kind = MK_GLASS;
            r.c = m.c;
            break;
        case YK_MAT_METAL: {  // metal.rs:39-50, trowbridge_reitz.rs:15-20
            r.kind = MK_METAL;
            float roughness = remap ? roughness_to_alpha(m.c) : m.c;
            r.c = rmax(roughness, 0.001f);
            break;
        }
        default: {  // glossy.rs:37-49
            r.kind = MK_GLOSSY;
            float roughness = remap ? roughness_to_alpha(m.c) : m.c;
            r.c = rmax(roughness * roughness, 0.001f);
            break;
        }
    }
    return r;
}

DevLight make_light(const yk_light_desc& l) {
    DevLight d;
    std::memset(&d, 0, sizeof(d));
    d.kind = l.kind;
    for (int k = 0; k < 3; ++k) {
        d.p[k] = l.p[k];
        d.i[k] = l.i[k];
    }
    d.cos_total_width = l.cos_total_width;
    d.cos_falloff_start = l.cos_falloff_start;
    std::memcpy(d.w2l, l.world_to_light, 64);
    std::memcpy(d.s2w, l.sample_to_world, 64);
    V3 n = xf_normal(l.sample_to_world_inv, V3{0.0f, -1.0f, 0.0f});  // rectangular_light.rs:48
    d.n[0] = n.x;
    d.n[1] = n.y;
    d.n[2] = n.z;
    d.area = l.area;
    return d;
}

// Every device buffer a scene owns.  The first seven are its record buffers, in the order of YK_RECORDS_*.
static std::array<DevBuf*, 22> scene_buffers(yk_scene* s) {
    return {&s->nodes,    &s->nodes4,       &s->top_nodes,      &s->top_nodes_any, &s->tris,      &s->prim_shade, &s->prim_attr, &s->indices, &s->points,  &s->normals,    &s->uvs,
            &s->tri_mesh, &s->tri_material, &s->tri_area_light, &s->mesh_flags,    &s->materials, &s->lights,     &s->spheres,   &s->texels,  &s->tex_info, &s->tree_nodes, &s->tree_order};
}
static const DevBuf& record_buffer(const yk_scene* s, uint32_t which) { return *scene_buffers(const_cast<yk_scene*>(s))[which]; }

void set_record_layout(yk_scene* s, size_t n_interior, size_t n_wide, size_t n_top, size_t n_top_any, size_t n_shapes, bool has_attr, uint32_t root_ref, bool wide_auto) {
    yk_scene_layout_info& li = s->layout;
    li.root_ref = root_ref;
    li.n_top = (uint32_t)n_top;
    li.n_top_any = (uint32_t)n_top_any;
    li.wide = n_wide ? 1u : 0u;
    li.wide_auto = wide_auto ? 1u : 0u;
    s->record_bytes[YK_RECORDS_NODES] = std::max<size_t>(n_interior, 1) * sizeof(DevNode);
    s->record_bytes[YK_RECORDS_NODES4] = n_wide * sizeof(DevNode4);
    s->record_bytes[YK_RECORDS_TOP] = n_top * sizeof(DevNode);
    s->record_bytes[YK_RECORDS_TOP_ANY] = n_top_any * sizeof(DevNode);
    s->record_bytes[YK_RECORDS_TRIS] = 3 * n_shapes * sizeof(float4);
    s->record_bytes[YK_RECORDS_PRIM_SHADE] = n_shapes * sizeof(uint4);
    s->record_bytes[YK_RECORDS_PRIM_ATTR] = has_attr ? 4 * n_shapes * sizeof(float4) : 0;
}

// Everything yk_scene_create derives from a scene description on the host (yk_internal.h).
struct SceneImage {
    std::shared_ptr<const HostBvh> bvh;
    std::shared_ptr<HostBvh> bvh_mut;  // the same tree, writable: its arrays are filled late when the builder left them in HBM
    // "scene_layout" = 1 (single-device scenes): the records below dn .. prim_attr stay empty and yk_upload_scene_image lays them
    // out on the device — from dtree, where the device builder left the tree (tree_on_device), or from an upload of the host tree
    bool device_layout = false, tree_on_device = false, order_applied = false;  // order_applied: the caller's shape order went into dtree.order
    uint32_t layout_reason = 0;  // YK_LAYOUT_REASON_*: why a device layout that was asked for is not attempted
    DeviceTree dtree;
    ~SceneImage() { dtree.release(); }
    const yk_scene_desc* d = nullptr;  // BORROWED: the caller's arrays (indices, points, normals, uvs, tri_material) are uploaded straight
                                       // from the description, so an image is only valid inside the call that built it
    uint32_t n_triangles = 0, n_spheres = 0, n_lights = 0, n_delta_lights = 0;
    yk_scene_info info;  // host part: node counts, bounds, build time
    yk_bvh_build_info build_info;
    bool has_device_records = false, wide_auto = false;  // wide_auto, root_ref: of the host layout
    uint32_t root_ref = 0;
    std::vector<DevNode> dn, top, top_any;
    std::vector<DevNode4> dn4;
    std::vector<float4> tris, texels, prim_attr;
    std::vector<uint4> prim_shade, tex_info;
    std::vector<uint32_t> mesh_flags, tri_mesh, mat_kind;  // mat_kind: device BSDF kind (MK_*) per material
    std::vector<int32_t> tri_al;
    std::vector<uint8_t> shape_kind;  // source shape -> BSDF kind (yk_scene::shape_kind)
    std::vector<Material> mats;
    std::vector<DevSphere> spheres;
    std::vector<DevLight> lights;
};

static void layout_records_host(const yk_context* ctx, SceneImage* s);

// ---- the steps of yk_build_scene_image, in its order
// arrays_on_host false (yk_scene_create_device): the large arrays are device pointers; the two loops over the triangles are
// left to k_check_geometry, which runs after everything here has passed
static yk_status check_description(yk_context* ctx, const yk_scene_desc* d, bool arrays_on_host = true) {
    if ((uint64_t)d->n_triangles + d->n_spheres == 0) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "empty scene");
    if (d->n_triangles && (!d->points || !d->indices)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "missing geometry arrays");
    if (d->max_shapes_in_node == 0 || d->max_shapes_in_node > 65535u || d->split_method > 2) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad BVH settings");
    for (uint32_t i = 0; arrays_on_host && i < d->n_triangles; ++i) {
        for (int k = 0; k < 3; ++k)
            if (d->indices[3 * i + k] >= d->n_vertices) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "vertex index out of range");
        if (d->tri_mesh && d->tri_mesh[i] >= d->n_meshes) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "mesh index out of range");
        if (d->tri_material && (d->tri_material[i] < 0 || (uint32_t)d->tri_material[i] >= d->n_materials))
            return fail(ctx, YK_ERR_INVALID_ARGUMENT, "material index out of range");
        if (d->tri_area_light && d->tri_area_light[i] >= (int32_t)d->n_lights) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "light index out of range");
    }
    if ((d->n_spheres && !d->spheres) || (d->n_materials && !d->materials) || (d->n_lights && !d->lights) || (d->n_meshes && !d->meshes))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "a count is non-zero but its array is NULL");
    if (d->tri_area_light && arrays_on_host)  // Triangle.area_light is Option<Arc<RectangularLight>> (triangle.rs:22): -1 or a rectangular light
        for (uint32_t i = 0; i < d->n_triangles; ++i) {
            const int32_t al = d->tri_area_light[i];
            if (al < -1 || (al >= 0 && d->lights[al].kind != YK_LIGHT_RECT)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "tri_area_light must be -1 or index a rectangular light");
        }
    for (uint32_t k = 0; k < d->n_spheres; ++k)
        if (d->spheres[k].material < 0 || (uint32_t)d->spheres[k].material >= d->n_materials) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "sphere material out of range");
    for (uint32_t m = 0; m < d->n_materials; ++m)
        if ((d->materials[m].flags & YK_MAT_FLAG_TEXTURED_A) && d->materials[m].kind == YK_MAT_MATTE && d->materials[m].a_texture >= d->n_textures)
            return fail(ctx, YK_ERR_INVALID_ARGUMENT, "material texture index out of range");
    if (d->n_materials >= (1u << 26)) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^26 materials");
    for (uint32_t t = 0; t < d->n_textures; ++t)
        if (!d->textures || !d->textures[t].rgb || d->textures[t].width == 0 || d->textures[t].height == 0 || d->textures[t].width >= (1u << 24) ||
            d->textures[t].height >= (1u << 24))
            return fail(ctx, YK_ERR_INVALID_ARGUMENT, "bad texture");
    if (d->n_triangles && (!d->tri_material || d->n_materials == 0 || d->n_meshes == 0))
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, "triangles need materials and meshes");
    for (uint32_t m = 0; m < d->n_meshes; ++m) {
        if (d->meshes[m].has_normals && !d->normals) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "mesh has_normals without a normals array");
        if (d->meshes[m].has_uvs && !d->uvs) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "mesh has_uvs without a uvs array");
    }
    return YK_OK;
}

// Sphere::world_bound (sphere.rs:121-123)
static ShapeBounds sphere_bound(const yk_sphere_desc& sp) {
    const float r = sp.radius;
    const float lo[3] = {-r, -r, -r}, hi[3] = {r, r, r};
    const float big = 3.40282347e+38f;
    ShapeBounds b = {{big, big, big}, {-big, -big, -big}};
    const int corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};  // transform.rs:194-206
    for (int c = 0; c < 8; ++c) {
        V3 q = xf_point(sp.object_to_world, V3{corner[c][0] ? hi[0] : lo[0], corner[c][1] ? hi[1] : lo[1], corner[c][2] ? hi[2] : lo[2]});
        const float qq[3] = {q.x, q.y, q.z};
        for (int k = 0; k < 3; ++k) {
            b.bmin[k] = rmin(b.bmin[k], qq[k]);
            b.bmax[k] = rmax(b.bmax[k], qq[k]);
        }
    }
    return b;
}
// world bounds of every shape — Triangle::world_bound (triangle.rs:229-235), Sphere::world_bound — in the caller's shape
// order when there is one
static yk_status shape_bounds(yk_context* ctx, const yk_scene_desc* d, std::vector<ShapeBounds>& sb) {
    sb.assign((size_t)d->n_triangles + d->n_spheres, ShapeBounds());
    for (uint32_t i = 0; i < d->n_triangles; ++i) {
        const float* p0 = d->points + 3 * (size_t)d->indices[3 * i];
        const float* p1 = d->points + 3 * (size_t)d->indices[3 * i + 1];
        const float* p2 = d->points + 3 * (size_t)d->indices[3 * i + 2];
        for (int k = 0; k < 3; ++k) {
            sb[i].bmin[k] = rmin(rmin(p0[k], p1[k]), p2[k]);
            sb[i].bmax[k] = rmax(rmax(p0[k], p1[k]), p2[k]);
        }
    }
    for (uint32_t i = 0; i < d->n_spheres; ++i) sb[(size_t)d->n_triangles + i] = sphere_bound(d->spheres[i]);
    if (d->shape_order) {  // the caller's Scene.shapes order (a permutation of all shapes)
        std::vector<uint8_t> seen(sb.size(), 0);
        std::vector<ShapeBounds> ordered(sb.size());
        for (size_t i = 0; i < sb.size(); ++i) {
            const uint32_t src = d->shape_order[i];
            if (src >= sb.size() || seen[src]) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "shape_order is not a permutation of the shapes");
            seen[src] = 1;
            ordered[i] = sb[src];
        }
        sb.swap(ordered);
    }
    return YK_OK;
}

// the tree into s->bvh_mut (or, "scene_layout" = 1 and the device builder, into s->dtree), who built it and how long it took
static yk_status build_tree(yk_context* ctx, const yk_scene_desc* d, const std::vector<ShapeBounds>& sb, bool device_builder_allowed, SceneImage* s) {
    double t0 = now_seconds();
    // Who builds the tree: the host recursion unless the context's "bvh_builder" asks for the device or the environment
    // (YK_BVH_BUILDER=levels, YK_BVH_SMALL_RANGE=n; next to YK_BVH_THREADS) for the host instance of the level algorithm.
    // A level builder that refuses leaves its reason in the build info and the recursion builds the same tree.
    yk_bvh_build_info& bi = s->build_info;
    std::memset(&bi, 0, sizeof(bi));
    bool built = false;
    const char* env_builder = std::getenv("YK_BVH_BUILDER");
    if (ctx && ctx->bvh_builder == 1 && device_builder_allowed) {
        built = build_bvh_device(ctx, sb, d->max_shapes_in_node, d->split_method, (uint32_t)ctx->bvh_small_range, *s->bvh_mut, bi, s->device_layout ? &s->dtree : nullptr);
        s->tree_on_device = built && s->device_layout;
    } else if (env_builder && std::strcmp(env_builder, "levels") == 0) {
        const char* e = std::getenv("YK_BVH_SMALL_RANGE");
        built = build_bvh_levels(sb, d->max_shapes_in_node, d->split_method, e ? (uint32_t)std::max(0, std::atoi(e)) : (uint32_t)YK_BVH_SMALL_RANGE, *s->bvh_mut, bi);
    }
    if (!built) {
        bi.builder = YK_BVH_BUILDER_HOST;
        build_bvh(sb, d->max_shapes_in_node, d->split_method, *s->bvh_mut);
    }
    s->info.build_seconds = now_seconds() - t0;
    if (d->shape_order && !s->tree_on_device)  // leaf order -> position in Scene.shapes -> source shape (a tree in HBM: the layout applies it there)
        for (uint32_t& o : s->bvh_mut->shape_order) o = d->shape_order[o];
    if (s->bvh_mut->split_failed || (s->tree_on_device ? s->dtree.n_nodes == 0 : s->bvh_mut->nodes.empty())) return fail(ctx, YK_ERR_BVH_BUILD, "BVH split failed (reference: assert_ne!(mid, start))");
    return YK_OK;
}

static void fill_scene_info(SceneImage* s) {
    const HostBvh* bvh = s->bvh.get();
    s->info.max_leaf_shapes = bvh->max_leaf_shapes;
    s->info.tree_depth = bvh->depth;
    yk_bvh_node root;  // a tree in HBM: the builder's counters and node 0; a binary tree of n nodes has (n - 1) / 2 interior ones
    std::memcpy(&root, s->tree_on_device ? (const void*)s->dtree.root_words : (const void*)bvh->nodes.data(), sizeof(root));
    s->info.n_nodes = s->tree_on_device ? s->dtree.n_nodes : bvh->nodes.size();
    s->info.n_shapes = s->tree_on_device ? s->dtree.n_shapes : bvh->shape_order.size();
    s->info.n_interior = s->tree_on_device ? (s->dtree.n_nodes - 1u) / 2u : (uint64_t)std::count_if(bvh->nodes.begin(), bvh->nodes.end(), [](const yk_bvh_node& n) { return !n.is_leaf; });
    for (int k = 0; k < 3; ++k) {
        s->info.bounds_min[k] = root.bmin[k];
        s->info.bounds_max[k] = root.bmax[k];
    }
}

// the small tables of the device scene, from the description's host tables alone; the host layout reads mat_kind and mesh_flags
static yk_status small_tables(yk_context* ctx, const yk_scene_desc* d, SceneImage* s) {
    s->mats.resize(std::max<uint32_t>(d->n_materials, 1));
    s->mat_kind.assign(s->mats.size(), 0u);
    for (uint32_t m = 0; m < d->n_materials; ++m) {
        s->mats[m] = make_material(d->materials[m]);
        s->mat_kind[m] = s->mats[m].kind & 7u;
    }
    s->mesh_flags.assign(std::max<uint32_t>(d->n_meshes, 1), 0);
    for (uint32_t m = 0; m < d->n_meshes; ++m)
        s->mesh_flags[m] = (d->meshes[m].has_normals ? YK_MESH_NORMALS : 0u) | (d->meshes[m].has_uvs ? YK_MESH_UVS : 0u) | (d->meshes[m].swaps_handedness ? YK_MESH_SWAPS : 0u);
    s->spheres.resize(std::max<uint32_t>(d->n_spheres, 1));
    for (uint32_t k = 0; k < d->n_spheres; ++k) {
        DevSphere& o = s->spheres[k];
        std::memcpy(o.o2w, d->spheres[k].object_to_world, 64);
        std::memcpy(o.w2o, d->spheres[k].world_to_object, 64);
        o.radius = d->spheres[k].radius;
        o.material = d->spheres[k].material;
        const float* m = o.o2w;  // Transform::swaps_handedness, transform.rs:85-91
        float det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8]) + m[2] * (m[4] * m[9] - m[5] * m[8]);
        o.swaps_handedness = det < 0.0f ? 1u : 0u;
        o.pad = 0;
    }
    s->lights.resize(std::max<uint32_t>(d->n_lights, 1));
    for (uint32_t l = 0; l < d->n_lights; ++l) s->lights[l] = make_light(d->lights[l]);
    for (uint32_t t = 0; t < d->n_textures; ++t) {
        const yk_texture_desc& td = d->textures[t];
        s->tex_info.push_back(make_uint4((unsigned)s->texels.size(), td.width, td.height, 0u));
        const size_t n = (size_t)td.width * td.height;
        if (s->texels.size() + n > 0xffffffffull) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^32 texels");
        for (size_t k = 0; k < n; ++k) s->texels.push_back(make_float4(td.rgb[3 * k], td.rgb[3 * k + 1], td.rgb[3 * k + 2], 0.0f));
    }
    return YK_OK;
}
// ... and what is derived from the per-triangle arrays on the host
static yk_status host_tables(yk_context* ctx, const yk_scene_desc* d, SceneImage* s) {
    yk_status st = small_tables(ctx, d, s);
    if (st != YK_OK) return st;
    s->shape_kind.resize(s->info.n_shapes);
    for (uint32_t i = 0; i < d->n_triangles; ++i) s->shape_kind[i] = (uint8_t)s->mat_kind[d->tri_material[i]];
    for (uint32_t k = 0; k < d->n_spheres; ++k) s->shape_kind[(size_t)d->n_triangles + k] = (uint8_t)s->mat_kind[d->spheres[k].material];
    s->tri_mesh.assign(d->n_triangles, 0);
    if (d->tri_mesh) std::memcpy(s->tri_mesh.data(), d->tri_mesh, sizeof(uint32_t) * d->n_triangles);
    s->tri_al.assign(d->n_triangles, -1);
    if (d->tri_area_light) std::memcpy(s->tri_al.data(), d->tri_area_light, sizeof(int32_t) * d->n_triangles);
    return YK_OK;
}

// Host half of yk_scene_create: validation, BoundingVolumeHierarchy::new (bvh.rs:39-115) and — when `ctx` is given (its
// "top_nodes" / "wide_bvh" options apply) — the device records laid out from the tree.
yk_status yk_build_scene_image(yk_context* ctx, const yk_scene_desc* d, std::shared_ptr<SceneImage>& out, bool device_builder_allowed) try {
    if (!d) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene description");
    out.reset();
    yk_status st = check_description(ctx, d);
    if (st != YK_OK) return st;

    std::shared_ptr<SceneImage> img = std::make_shared<SceneImage>();
    SceneImage* s = img.get();
    s->bvh = s->bvh_mut = std::make_shared<HostBvh>();
    s->d = d;
    s->device_layout = ctx && ctx->scene_layout == 1 && device_builder_allowed;
    s->layout_reason = ctx && ctx->scene_layout == 1 && !device_builder_allowed ? (uint32_t)YK_LAYOUT_REASON_MULTI : 0u;
    s->n_triangles = d->n_triangles;
    s->n_spheres = d->n_spheres;
    s->n_lights = d->n_lights;
    for (uint32_t l = 0; l < d->n_lights; ++l) s->n_delta_lights += d->lights[l].kind != YK_LIGHT_RECT ? 1u : 0u;
    std::memset(&s->info, 0, sizeof(s->info));

    std::vector<ShapeBounds> sb;
    if ((st = shape_bounds(ctx, d, sb)) != YK_OK || (st = build_tree(ctx, d, sb, device_builder_allowed, s)) != YK_OK) return st;
    fill_scene_info(s);
    if (ctx) {  // device records (a host-only scene — ctx == NULL — stops at the tree)
        if (s->info.n_nodes > YK_REF_INDEX_MAX || s->info.n_shapes > YK_REF_INDEX_MAX) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^28 BVH nodes or shapes");
        if ((st = host_tables(ctx, d, s)) != YK_OK) return st;
        if (!s->device_layout) layout_records_host(ctx, s);
        s->has_device_records = true;
    }
    out = img;
    return YK_OK;
} YK_CATCH(ctx)

// The device records from the host tree (s->bvh with its arrays): the sequential loops the device layout
// (yk_scene_layout.hip) is held against, in three sections.
// DevNode per interior node, the root ref and the two tree tops
static void layout_nodes_host(const yk_context* ctx, SceneImage* s) {
    const std::vector<yk_bvh_node>& nodes = s->bvh->nodes;
    const uint64_t n_interior = s->info.n_interior;
    // interior index of each reference node = number of interior nodes before it
    std::vector<uint32_t> interior_index(nodes.size());
    uint32_t cnt = 0;
    for (size_t i = 0; i < nodes.size(); ++i) {
        interior_index[i] = cnt;
        if (!nodes[i].is_leaf) ++cnt;
    }
    auto ref_of = [&](uint32_t idx) -> uint32_t { return nodes[idx].is_leaf ? (YK_LEAF_BIT | nodes[idx].a) : interior_index[idx]; };
    std::vector<DevNode>& dn = s->dn;
    dn.assign(std::max<size_t>(n_interior, 1), DevNode());
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (nodes[i].is_leaf) continue;
        const yk_bvh_node& c0 = nodes[i + 1];
        const yk_bvh_node& c1 = nodes[nodes[i].a];
        DevNode& o = dn[interior_index[i]];
        o.q0 = make_float4(c0.bmin[0], c0.bmin[1], c0.bmin[2], c0.bmax[0]);
        o.q1 = make_float4(c0.bmax[1], c0.bmax[2], c1.bmin[0], c1.bmin[1]);
        o.q2 = make_float4(c1.bmin[2], c1.bmax[0], c1.bmax[1], c1.bmax[2]);
        o.q3 = make_uint4(ref_of((uint32_t)i + 1), ref_of(nodes[i].a) | ((uint32_t)nodes[i].axis << YK_AXIS_SHIFT), 0u, 0u);
    }
    // top of the tree, breadth first, for the LDS-resident copies (YK_TOP_BIT refs).  Two sets: the closest-hit kernels
    // keep 8-byte stack entries (ref, entry distance) in LDS and have room for trace_top_nodes() nodes beside them; the
    // any-hit kernel's entries are a bare ref (4 bytes), which leaves room for trace_top_nodes_any() — more than twice as many.
    auto build_top = [&](size_t cap, std::vector<DevNode>& top) {
        top.clear();
        if (nodes[0].is_leaf || cap == 0) return;
        std::vector<uint32_t> order;  // reference node indices, breadth first
        std::vector<uint32_t> top_id(nodes.size(), 0xffffffffu);
        order.push_back(0);
        top_id[0] = 0;
        for (size_t q = 0; q < order.size() && order.size() < cap; ++q) {
            const uint32_t P = order[q];
            for (uint32_t c : {P + 1, nodes[P].a}) {
                if (!nodes[c].is_leaf && order.size() < cap) {
                    top_id[c] = (uint32_t)order.size();
                    order.push_back(c);
                }
            }
        }
        for (uint32_t P : order) {
            DevNode t = dn[interior_index[P]];
            const uint32_t c0 = P + 1, c1 = nodes[P].a;
            if (top_id[c0] != 0xffffffffu) t.q3.x = YK_TOP_BIT | top_id[c0];
            if (top_id[c1] != 0xffffffffu) t.q3.y = YK_TOP_BIT | top_id[c1] | ((uint32_t)nodes[P].axis << YK_AXIS_SHIFT);
            top.push_back(t);
        }
    };
    build_top((size_t)std::min<int64_t>(ctx->top_nodes, trace_top_nodes()), s->top);
    build_top((size_t)std::min<int64_t>(ctx->top_nodes, trace_top_nodes_any()), s->top_any);
    s->root_ref = ref_of(0);
}

static void layout_wide_host(const yk_context* ctx, SceneImage* s) {
    const HostBvh* bvh = s->bvh.get();
    const std::vector<yk_bvh_node>& nodes = bvh->nodes;
    const uint64_t n_interior = s->info.n_interior;
    // 4-wide collapse (DevNode4): one node per reference interior node reached at even depth
    // below the root.  Built only while the traversal stack of the collapsed tree is
    // guaranteed to fit (the reference asserts on its own stack depth, bvh.rs:172-174).
    std::vector<DevNode4>& dn4 = s->dn4;
    const bool wide = ctx->wide_bvh != 0 && !nodes[0].is_leaf && bvh->depth <= 64;
    s->wide_auto = wide && ctx->wide_bvh == 2;
    if (wide) {
        dn4.reserve(n_interior / 2 + 1);
        struct Todo {
            uint32_t binary;  // reference node index of P
            uint32_t slot;    // DevNode4 index to fill
        };
        std::vector<Todo> stack;
        dn4.emplace_back();
        stack.push_back(Todo{0u, 0u});
        while (!stack.empty()) {
            const Todo td = stack.back();
            stack.pop_back();
            const uint32_t P = td.binary, A = P + 1, B = nodes[P].a;
            uint32_t child[4] = {YK_REF_NONE, YK_REF_NONE, YK_REF_NONE, YK_REF_NONE};  // reference node index per slot
            if (nodes[A].is_leaf) {
                child[0] = A;
            } else {
                child[0] = A + 1;
                child[1] = nodes[A].a;
            }
            if (nodes[B].is_leaf) {
                child[2] = B;
            } else {
                child[2] = B + 1;
                child[3] = nodes[B].a;
            }
            float box[4][6] = {};
            uint32_t ref[4];
            for (int k = 0; k < 4; ++k) {
                ref[k] = YK_REF_NONE;
                if (child[k] == YK_REF_NONE) continue;
                const yk_bvh_node& c = nodes[child[k]];
                for (int a = 0; a < 3; ++a) {
                    box[k][a] = c.bmin[a];
                    box[k][3 + a] = c.bmax[a];
                }
                if (c.is_leaf) {
                    ref[k] = YK_LEAF_BIT | c.a;
                } else {
                    ref[k] = (uint32_t)dn4.size();
                    dn4.emplace_back();
                }
            }
            // children are expanded so that the first visited subtree (for a positive ray) follows in memory
            for (int k = 3; k >= 0; --k)
                if (ref[k] != YK_REF_NONE && !(ref[k] & YK_LEAF_BIT)) stack.push_back(Todo{child[k], ref[k]});
            DevNode4& o = dn4[td.slot];
            o.q0 = make_float4(box[0][0], box[0][1], box[0][2], box[0][3]);
            o.q1 = make_float4(box[0][4], box[0][5], box[1][0], box[1][1]);
            o.q2 = make_float4(box[1][2], box[1][3], box[1][4], box[1][5]);
            o.q3 = make_float4(box[2][0], box[2][1], box[2][2], box[2][3]);
            o.q4 = make_float4(box[2][4], box[2][5], box[3][0], box[3][1]);
            o.q5 = make_float4(box[3][2], box[3][3], box[3][4], box[3][5]);
            o.q6 = make_uint4(ref[0], ref[1], ref[2], ref[3]);
            const uint32_t axA = nodes[A].is_leaf ? 0u : nodes[A].axis, axB = nodes[B].is_leaf ? 0u : nodes[B].axis;
            o.q7 = make_uint4((uint32_t)nodes[P].axis | (axA << 2) | (axB << 4), 0u, 0u, 0u);
        }
    }
}

// tris / prim_shade / prim_attr in leaf order
static void layout_prims_host(SceneImage* s) {
    const yk_scene_desc* d = s->d;
    const HostBvh* bvh = s->bvh.get();
    const std::vector<uint32_t>& mat_kind = s->mat_kind;
    const size_t np = bvh->shape_order.size();
    std::vector<float4>& tris = s->tris;
    tris.assign(3 * np, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    std::vector<uint4>& prim_shade = s->prim_shade;
    prim_shade.assign(np, make_uint4(0u, 0u, 0u, 0u));
    std::vector<uint8_t> last(np, 0);
    for (const yk_bvh_node& n : bvh->nodes)
        if (n.is_leaf) last[(size_t)n.a + n.count - 1] = 1;
    for (size_t p = 0; p < np; ++p) {
        uint32_t src = bvh->shape_order[p];
        if (src >= d->n_triangles) {  // sphere: only the source index and the flags are read
            uint32_t none = 0xffffffffu, fl = (last[p] ? YK_PRIM_LAST : 0u) | YK_PRIM_SPHERE | (mat_kind[d->spheres[src - d->n_triangles].material] << YK_PRIM_KIND_SHIFT);
            float w0, w1, w2;
            std::memcpy(&w0, &none, 4);
            std::memcpy(&w1, &src, 4);
            std::memcpy(&w2, &fl, 4);
            tris[3 * p + 0] = make_float4(0.0f, 0.0f, 0.0f, w0);
            tris[3 * p + 1] = make_float4(0.0f, 0.0f, 0.0f, w1);
            tris[3 * p + 2] = make_float4(0.0f, 0.0f, 0.0f, w2);
            prim_shade[p] = make_uint4(0u, 0u, 0u, ((uint32_t)d->spheres[src - d->n_triangles].material << 6) | (mat_kind[d->spheres[src - d->n_triangles].material] << 3));
            continue;
        }
        const float* p0 = d->points + 3 * (size_t)d->indices[3 * src];
        const float* p1 = d->points + 3 * (size_t)d->indices[3 * src + 1];
        const float* p2 = d->points + 3 * (size_t)d->indices[3 * src + 2];
        int al = d->tri_area_light ? d->tri_area_light[src] : -1;
        uint32_t alb = (uint32_t)al, lastb = (last[p] ? YK_PRIM_LAST : 0u) | (mat_kind[d->tri_material[src]] << YK_PRIM_KIND_SHIFT);
        float w0, w1, w2;
        std::memcpy(&w0, &alb, 4);
        std::memcpy(&w1, &src, 4);
        std::memcpy(&w2, &lastb, 4);
        tris[3 * p + 0] = make_float4(p0[0], p0[1], p0[2], w0);
        tris[3 * p + 1] = make_float4(p1[0], p1[1], p1[2], w1);
        tris[3 * p + 2] = make_float4(p2[0], p2[1], p2[2], w2);
        const uint32_t mfl = s->mesh_flags[s->tri_mesh[src]];
        prim_shade[p] = make_uint4(d->indices[3 * src], d->indices[3 * src + 1], d->indices[3 * src + 2],
                                   ((uint32_t)d->tri_material[src] << 6) | (mat_kind[d->tri_material[src]] << 3) | mfl);
    }
    if (d->normals || d->uvs) {  // leaf-order copy of the per-vertex normals / uvs (yk_device.h: DevScene::prim_attr)
        s->prim_attr.assign(4 * np, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        for (size_t p = 0; p < np; ++p) {
            const uint32_t src = bvh->shape_order[p];
            if (src >= d->n_triangles) continue;
            const uint32_t mfl = s->mesh_flags[s->tri_mesh[src]];
            float nrm[3][3] = {}, uv[3][2] = {};
            for (int k = 0; k < 3; ++k) {
                const size_t vi = d->indices[3 * (size_t)src + k];
                if (mfl & YK_MESH_NORMALS)
                    for (int c = 0; c < 3; ++c) nrm[k][c] = d->normals[3 * vi + c];
                if (mfl & YK_MESH_UVS)
                    for (int c = 0; c < 2; ++c) uv[k][c] = d->uvs[2 * vi + c];
            }
            s->prim_attr[4 * p + 0] = make_float4(nrm[0][0], nrm[0][1], nrm[0][2], uv[0][0]);
            s->prim_attr[4 * p + 1] = make_float4(nrm[1][0], nrm[1][1], nrm[1][2], uv[0][1]);
            s->prim_attr[4 * p + 2] = make_float4(nrm[2][0], nrm[2][1], nrm[2][2], uv[1][0]);
            s->prim_attr[4 * p + 3] = make_float4(uv[1][1], uv[2][0], uv[2][1], 0.0f);
        }
    }
}

static void layout_records_host(const yk_context* ctx, SceneImage* s) {
    layout_nodes_host(ctx, s);
    layout_wide_host(ctx, s);
    layout_prims_host(s);
}

// 32-byte nodes and shape order from HBM into the host tree (no-op for buffers that are not there)
static yk_status fetch_tree(int device, const DevBuf& d_nodes, const DevBuf& d_order, uint32_t n_nodes, uint32_t n_shapes, HostBvh& out) {
    if (!d_nodes.p || !d_order.p || !out.nodes.empty()) return YK_OK;
    (void)hipSetDevice(device);
    std::vector<yk_bvh_node> nodes(n_nodes);
    std::vector<uint32_t> order(n_shapes);
    if (hipMemcpy(nodes.data(), d_nodes.p, (size_t)n_nodes * sizeof(yk_bvh_node), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(order.data(), d_order.p, (size_t)n_shapes * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return YK_ERR_DEVICE;
    }
    out.nodes.swap(nodes);
    out.shape_order.swap(order);
    return YK_OK;
}

const HostBvh* scene_host_tree(const yk_scene* s) {
    if (!s || !s->bvh) return nullptr;
    std::lock_guard<std::mutex> lock(s->tree_mu);  // a device-route update makes the copy stale again (yk_scene_update)
    if (s->bvh_lazy && !s->tree_fetched.load() &&
        fetch_tree(s->device, s->tree_nodes, s->tree_order, (uint32_t)s->info.n_nodes, (uint32_t)s->info.n_shapes, *s->bvh_lazy) == YK_OK)
        s->tree_fetched.store(1u);
    return s->tree_fetched.load() ? s->bvh.get() : nullptr;
}

// "scene_layout" = 1: the tree to HBM unless the builder left it there, the two small tables, the layout kernels
// (yk_scene_layout.hip).  The scene's own arrays (indices .. spheres) are uploaded already.  Returns YK_LAYOUT_REASON_*.
static uint32_t layout_on_device(yk_context* ctx, SceneImage* img, yk_scene* s) {
    const yk_scene_desc* d = img->d;
    DeviceTree& tree = img->dtree;
    double t0 = now_seconds();
    DevBuf d_mat_kind, d_user;
    struct Free {
        DevBuf &a, &b;
        ~Free() {
            a.release();
            b.release();
        }
    } free_tables{d_mat_kind, d_user};
    auto put = [&](DevBuf& buf, const void* src, size_t bytes) -> uint32_t {
        hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
        if (e == hipSuccess && bytes) e = hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) return YK_LAYOUT_REASON_NONE;
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? YK_LAYOUT_REASON_OUT_OF_MEMORY : YK_LAYOUT_REASON_DEVICE_ERROR;
    };
    uint32_t r;
    std::vector<uint8_t> kinds(img->mat_kind.begin(), img->mat_kind.end());
    if ((r = put(d_mat_kind, kinds.data(), kinds.size())) != 0) return r;
    if (img->tree_on_device) {
        if (d->shape_order && (r = put(d_user, d->shape_order, (size_t)tree.n_shapes * 4)) != 0) return r;
    } else {  // a host-built tree: its nodes, their depths (children follow their parent in the array) and the final order
        const HostBvh& bvh = *img->bvh;
        const std::vector<uint32_t> depth = lay::node_depths(reinterpret_cast<const uint32_t*>(bvh.nodes.data()), bvh.nodes.size());
        tree.n_nodes = (uint32_t)bvh.nodes.size();
        tree.n_shapes = (uint32_t)bvh.shape_order.size();
        std::memcpy(tree.root_words, bvh.nodes.data(), 32);
        if ((r = put(tree.nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(yk_bvh_node))) != 0 || (r = put(tree.depth, depth.data(), depth.size() * 4)) != 0 ||
            (r = put(tree.order, bvh.shape_order.data(), bvh.shape_order.size() * 4)) != 0)
            return r;
    }
    s->layout.seconds_upload = now_seconds() - t0;
    t0 = now_seconds();
    r = layout_scene_device(ctx, s, tree, img->tree_on_device && d->shape_order ? d_user.as<uint32_t>() : nullptr, d_mat_kind.as<uint8_t>(), d->normals || d->uvs, img->bvh->depth, &img->order_applied);
    s->layout.seconds_layout = now_seconds() - t0;
    if (r != YK_LAYOUT_REASON_NONE) return r;
    if (img->tree_on_device) {  // the host copy of the arrays is made when something asks for it (scene_host_tree)
        std::swap(s->tree_nodes, tree.nodes);
        std::swap(s->tree_order, tree.order);
        std::swap(s->upd.depth, tree.depth);  // kept for the scene's updates
        s->bvh_lazy = img->bvh_mut;
        s->tree_fetched.store(0u);
    }
    tree.release();
    return YK_LAYOUT_REASON_NONE;
}

// The DevScene the kernels are handed, from the scene's buffers, its layout info and the description's scalars.
static void bind_device_scene(yk_scene* s, const yk_scene_desc* d) {
    const yk_scene_layout_info& li = s->layout;
    DevScene& ds = s->dev;
    ds.nodes = s->nodes.as<DevNode>();
    ds.nodes4 = li.wide ? s->nodes4.as<DevNode4>() : nullptr;
    s->wide_auto = li.wide_auto != 0;
    ds.top_nodes = s->top_nodes.as<DevNode>();
    ds.n_top = li.n_top;
    ds.top_nodes_any = s->top_nodes_any.as<DevNode>();
    ds.n_top_any = li.n_top_any;
    ds.tris = s->tris.as<float4>();
    ds.prim_shade = s->prim_shade.as<uint4>();
    ds.prim_attr = s->record_bytes[YK_RECORDS_PRIM_ATTR] ? s->prim_attr.as<float4>() : nullptr;
    ds.spheres = d->n_spheres ? s->spheres.as<DevSphere>() : nullptr;
    ds.n_triangles = d->n_triangles;
    ds.root_ref = li.root_ref;
    for (int k = 0; k < 3; ++k) {  // node 0's box
        ds.root_bmin[k] = s->info.bounds_min[k];
        ds.root_bmax[k] = s->info.bounds_max[k];
        ds.background[k] = d->background[k];
    }
    ds.indices = s->indices.as<uint32_t>();
    ds.points = s->points.as<float>();
    ds.normals = s->normals.as<float>();
    ds.uvs = s->uvs.as<float>();
    ds.tri_mesh = s->tri_mesh.as<uint32_t>();
    ds.tri_material = s->tri_material.as<int32_t>();
    ds.tri_area_light = s->tri_area_light.as<int32_t>();
    ds.mesh_flags = s->mesh_flags.as<uint32_t>();
    ds.materials = s->materials.as<Material>();
    ds.lights = s->lights.as<DevLight>();
    ds.n_lights = d->n_lights;
    ds.texels = d->n_textures ? s->texels.as<float4>() : nullptr;
    ds.tex_info = d->n_textures ? s->tex_info.as<uint4>() : nullptr;
    s->on_device = true;
    for (DevBuf* b : scene_buffers(s)) s->info.device_bytes += b->bytes;
}

// What an update needs of the description after creation (yk_scene::UpdateState).
static void init_update_state(const yk_context* ctx, yk_scene* s, const yk_scene_desc* d, const std::vector<uint32_t>& mat_kind) {
    yk_scene::UpdateState& u = s->upd;
    u.n_vertices = d->n_vertices;
    u.has_normals = d->normals != nullptr;
    u.has_uvs = d->uvs != nullptr;
    u.top_nodes = ctx ? ctx->top_nodes : 0;
    u.wide_bvh = ctx ? ctx->wide_bvh : 0;
    u.mat_kind.assign(mat_kind.begin(), mat_kind.end());
    u.sphere_bounds.resize(6 * (size_t)d->n_spheres);
    for (uint32_t k = 0; k < d->n_spheres; ++k) {
        const ShapeBounds b = sphere_bound(d->spheres[k]);
        for (int a = 0; a < 3; ++a) {
            u.sphere_bounds[6 * (size_t)k + a] = b.bmin[a];
            u.sphere_bounds[6 * (size_t)k + 3 + a] = b.bmax[a];
        }
    }
    if (!ctx && d->n_triangles) u.host_indices.assign(d->indices, d->indices + 3 * (size_t)d->n_triangles);
}

// Device half: one copy of the image in the HBM of ctx's device.
yk_status yk_upload_scene_image(yk_context* ctx, const std::shared_ptr<SceneImage>& img, yk_scene** out) try {
    if (!out) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!img || !img->bvh) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene image");
    yk_scene* s = new yk_scene();
    struct SceneGuard {  // frees the half-built scene on every early return and on an exception
        yk_scene* s;
        ~SceneGuard() {
            if (s) yk_scene_destroy(s);
        }
    } guard{s};
    s->device = ctx ? ctx->device : -1;
    s->bvh = img->bvh;
    s->n_triangles = img->n_triangles;
    s->n_spheres = img->n_spheres;
    s->n_lights = img->n_lights;
    s->n_delta_lights = img->n_delta_lights;
    s->info = img->info;
    s->build_info = img->build_info;
    s->shape_kind = img->shape_kind;
    init_update_state(ctx, s, img->d, img->mat_kind);
    if (ctx) {
        if (!img->has_device_records) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "scene image was built without device records");
        const yk_scene_desc* d = img->d;
        (void)hipSetDevice(ctx->device);
        double u0 = now_seconds();
        yk_status st;
#define UP(buf, ptr, n) \
    if ((st = upload(ctx, s->buf, ptr, n)) != YK_OK) return st;
        UP(indices, d->indices, 3 * (size_t)d->n_triangles);
        UP(points, d->points, 3 * (size_t)d->n_vertices);
        UP(normals, d->normals, d->normals ? 3 * (size_t)d->n_vertices : 0);
        UP(uvs, d->uvs, d->uvs ? 2 * (size_t)d->n_vertices : 0);
        UP(tri_mesh, img->tri_mesh.data(), img->tri_mesh.size());
        UP(tri_material, d->tri_material, (size_t)d->n_triangles);
        UP(tri_area_light, img->tri_al.data(), img->tri_al.size());
        UP(mesh_flags, img->mesh_flags.data(), img->mesh_flags.size());
        UP(materials, img->mats.data(), img->mats.size());
        UP(lights, img->lights.data(), img->lights.size());
        UP(spheres, img->spheres.data(), img->spheres.size());
        UP(texels, img->texels.data(), img->texels.size());
        UP(tex_info, img->tex_info.data(), img->tex_info.size());
        yk_scene_layout_info& li = s->layout;
        li.reason = img->layout_reason;
        if (img->device_layout) {  // the records from the tree in HBM; whatever fails there leaves its reason and the host lays them out
            li.reason = layout_on_device(ctx, img.get(), s);
            if (li.reason == YK_LAYOUT_REASON_NONE) {
                li.layout = YK_LAYOUT_DEVICE;
            } else {
                yk_status fs = fetch_tree(ctx->device, img->dtree.nodes, img->dtree.order, img->dtree.n_nodes, img->dtree.n_shapes, *img->bvh_mut);
                if (fs != YK_OK) return fail(ctx, fs, "the device layout failed and the tree could not be copied back for the host layout");
                if (img->tree_on_device && d->shape_order && !img->order_applied)
                    for (uint32_t& o : img->bvh_mut->shape_order) o = d->shape_order[o];
                img->tree_on_device = false;
                img->dtree.release();
                layout_records_host(ctx, img.get());
            }
        }
        if (li.layout == YK_LAYOUT_HOST) {
            UP(nodes, img->dn.data(), img->dn.size());
            UP(nodes4, img->dn4.data(), img->dn4.size());
            UP(top_nodes, img->top.data(), img->top.size());
            UP(top_nodes_any, img->top_any.data(), img->top_any.size());
            UP(tris, img->tris.data(), img->tris.size());
            UP(prim_shade, img->prim_shade.data(), img->prim_shade.size());
            UP(prim_attr, img->prim_attr.data(), img->prim_attr.size());
            set_record_layout(s, s->info.n_interior, img->dn4.size(), img->top.size(), img->top_any.size(), s->info.n_shapes, d->normals || d->uvs, img->root_ref, img->wide_auto);
        }
#undef UP
        bind_device_scene(s, d);
        s->info.upload_seconds = now_seconds() - u0;
    }
    guard.s = nullptr;
    *out = s;
    return YK_OK;
} YK_CATCH(ctx)

const std::vector<uint8_t>* scene_shape_kind(const yk_scene* s) {
    if (!s) return nullptr;
    if (s->shape_kind_lazy)
        std::call_once(s->kind_once, [s] {
            std::vector<int32_t> mat(s->n_triangles);
            (void)hipSetDevice(s->device);
            if (s->n_triangles && hipMemcpy(mat.data(), s->tri_material.p, (size_t)s->n_triangles * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                return;
            }
            std::vector<uint8_t> kinds((size_t)s->n_triangles + s->n_spheres);
            for (uint32_t i = 0; i < s->n_triangles; ++i) kinds[i] = s->lazy_mat_kind[(uint32_t)mat[i]];
            for (uint32_t k = 0; k < s->n_spheres; ++k) kinds[(size_t)s->n_triangles + k] = s->lazy_sphere_kind[k];
            s->shape_kind.swap(kinds);
            s->kind_fetched.store(1u);
        });
    return s->kind_fetched.load() ? &s->shape_kind : nullptr;
}

// ------------------------------------------------------------------ yk_scene_create_device
// The same scene from large arrays that are in HBM already ("Input from device memory"): the per-triangle
// checks, the permutation test and the shape bounds run as kernels (yk_scene_input.hip), the builder starts from bounds
// it finds in HBM and the layout reads the scene's own device-to-device copies.

// every non-NULL large array is device memory of ctx's device, and its allocation reaches as far as its count says
static yk_status check_device_arrays(yk_context* ctx, const yk_scene_desc* d) {
    const size_t nv = d->n_vertices, nt = d->n_triangles, ns = nt + d->n_spheres;
    const struct {
        const char* name;
        const void* p;
        size_t bytes;
    } arrays[] = {{"points", d->points, 12 * nv},          {"normals", d->normals, 12 * nv},          {"uvs", d->uvs, 8 * nv},
                  {"indices", d->indices, 12 * nt},        {"tri_mesh", d->tri_mesh, 4 * nt},         {"tri_material", d->tri_material, 4 * nt},
                  {"tri_area_light", d->tri_area_light, 4 * nt}, {"shape_order", d->shape_order, 4 * ns}};
    for (const auto& a : arrays) {
        if (!a.p) continue;
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof(at));
        const hipError_t e = hipPointerGetAttributes(&at, a.p);
        if (e != hipSuccess) (void)hipGetLastError();
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != ctx->device) return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(a.name) + " is not device memory of this context's device");
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, const_cast<void*>(a.p)) != hipSuccess) {
            (void)hipGetLastError();
        } else if (reinterpret_cast<const char*>(a.p) + a.bytes > reinterpret_cast<const char*>(base) + size) {
            return fail(ctx, YK_ERR_INVALID_ARGUMENT, std::string(a.name) + " is shorter than its count says");
        }
    }
    return YK_OK;
}

// The device route.  *fall_back: the builder or the layout refused and the caller builds the scene by the host path — *refused
// then holds the builder's info with its reason (reason 0: it was the layout); any other failure is final.
static yk_status create_scene_on_device(yk_context* ctx, const yk_scene_desc* d, hipStream_t st, yk_scene** out, bool* fall_back, yk_bvh_build_info* refused) {
    *fall_back = false;
    std::memset(refused, 0, sizeof(*refused));
    const uint32_t nt = d->n_triangles, N = nt + d->n_spheres;
    yk_scene* s = new yk_scene();
    struct SceneGuard {
        yk_scene* s;
        ~SceneGuard() {
            if (s) yk_scene_destroy(s);
        }
    } guard{s};
    s->device = ctx->device;
    s->n_triangles = nt;
    s->n_spheres = d->n_spheres;
    s->n_lights = d->n_lights;
    for (uint32_t l = 0; l < d->n_lights; ++l) s->n_delta_lights += d->lights[l].kind != YK_LIGHT_RECT ? 1u : 0u;
    std::memset(&s->info, 0, sizeof(s->info));
    std::memset(&s->build_info, 0, sizeof(s->build_info));
    const double u0 = now_seconds();

    // the scene's own copies; a missing tri_mesh reads as zeros, a missing tri_area_light as -1
    auto own = [&](DevBuf& buf, const void* src, size_t bytes, int fill) -> hipError_t {
        hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
        if (e != hipSuccess || bytes == 0) return e;
        return src ? hipMemcpyAsync(buf.p, src, bytes, hipMemcpyDeviceToDevice, st) : hipMemsetAsync(buf.p, fill, bytes, st);
    };
    HIP_TRY(ctx, own(s->indices, d->indices, 12 * (size_t)nt, 0));
    HIP_TRY(ctx, own(s->points, d->points, 12 * (size_t)d->n_vertices, 0));
    HIP_TRY(ctx, own(s->normals, d->normals, d->normals ? 12 * (size_t)d->n_vertices : 0, 0));
    HIP_TRY(ctx, own(s->uvs, d->uvs, d->uvs ? 8 * (size_t)d->n_vertices : 0, 0));
    HIP_TRY(ctx, own(s->tri_mesh, d->tri_mesh, 4 * (size_t)nt, 0));
    HIP_TRY(ctx, own(s->tri_material, d->tri_material, 4 * (size_t)nt, 0));
    HIP_TRY(ctx, own(s->tri_area_light, d->tri_area_light, 4 * (size_t)nt, 0xff));

    SceneImage img;  // the small tables, and the tree while it waits for the layout
    std::memset(&img.info, 0, sizeof(img.info));
    yk_status rc = small_tables(ctx, d, &img);
    if (rc != YK_OK) return rc;
    std::vector<uint8_t> light_kind(std::max<uint32_t>(d->n_lights, 1), 0), mat_kind(img.mat_kind.begin(), img.mat_kind.end());
    init_update_state(ctx, s, d, img.mat_kind);
    for (uint32_t l = 0; l < d->n_lights; ++l) light_kind[l] = (uint8_t)d->lights[l].kind;
    std::vector<ShapeBounds> sphere_b(std::max<uint32_t>(d->n_spheres, 1));
    for (uint32_t k = 0; k < d->n_spheres; ++k) sphere_b[k] = sphere_bound(d->spheres[k]);

    DevScratch tmp;
    inp::CheckWords* d_words = nullptr;
    uint8_t *d_light_kind = nullptr, *d_mat_kind = nullptr;
    uint32_t *d_seen = nullptr, *d_user = nullptr;
    float *d_sphere_b = nullptr, *d_sb = nullptr;
    if (!tmp.get(d_words, 1) || !tmp.get(d_light_kind, light_kind.size()) || !tmp.get(d_mat_kind, mat_kind.size()) || !tmp.get(d_sphere_b, 6 * sphere_b.size()) || !tmp.get(d_sb, 6 * (size_t)N) ||
        (d->shape_order && (!tmp.get(d_seen, ((size_t)N + 31) / 32) || !tmp.get(d_user, N))))
        return fail(ctx, YK_ERR_OUT_OF_MEMORY, "no device memory for the scene's input stage");
    HIP_TRY(ctx, hipMemcpyAsync(d_light_kind, light_kind.data(), light_kind.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_mat_kind, mat_kind.data(), mat_kind.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_sphere_b, sphere_b.data(), sphere_b.size() * sizeof(ShapeBounds), hipMemcpyHostToDevice, st));
    if (d->shape_order) HIP_TRY(ctx, hipMemcpyAsync(d_user, d->shape_order, 4 * (size_t)N, hipMemcpyDeviceToDevice, st));

    // the checks, on the scene's copies; their words are read before any kernel follows an index
    inp::Geometry g;
    g.indices = s->indices.as<uint32_t>();
    g.tri_mesh = d->tri_mesh ? s->tri_mesh.as<uint32_t>() : nullptr;
    g.tri_material = s->tri_material.as<int32_t>();
    g.tri_area_light = d->tri_area_light ? s->tri_area_light.as<int32_t>() : nullptr;
    g.n_triangles = nt;
    g.n_vertices = d->n_vertices;
    g.n_meshes = d->n_meshes;
    g.n_materials = d->n_materials;
    g.n_lights = d->n_lights;
    inp::CheckWords words;
    HIP_TRY(ctx, enqueue_geometry_checks(st, g, d_light_kind, d_user, N, d_seen, d_words));
    HIP_TRY(ctx, hipMemcpyAsync(&words, d_words, sizeof(words), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (words.first != inp::kNoFailure) {
        static const char* const what[4] = {"vertex index out of range", "mesh index out of range", "material index out of range", "light index out of range"};
        return fail(ctx, YK_ERR_INVALID_ARGUMENT, what[words.first & 3u]);
    }
    if (words.light != inp::kNoFailure) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "tri_area_light must be -1 or index a rectangular light");
    if (words.order_bad) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "shape_order is not a permutation of the shapes");

    // bounds and tree
    const double t0 = now_seconds();
    HIP_TRY(ctx, enqueue_shape_bounds(st, s->points.as<float>(), s->indices.as<uint32_t>(), d_user, d_sphere_b, nt, N, d_sb, d_words));
    HIP_TRY(ctx, hipMemcpyAsync(&words.non_finite, &d_words->non_finite, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (words.non_finite) {  // a NaN that rmin / rmax dropped from its bound included (yk_scene_input.h)
        refused->small_range = (uint32_t)ctx->bvh_small_range;
        refused->reason = YK_BVH_REASON_NON_FINITE;
        *fall_back = true;
        return YK_OK;
    }
    img.bvh = img.bvh_mut = std::make_shared<HostBvh>();
    img.tree_on_device = true;
    if (!build_bvh_device(ctx, nullptr, d_sb, N, d->max_shapes_in_node, d->split_method, (uint32_t)ctx->bvh_small_range, *img.bvh_mut, s->build_info, &img.dtree)) {
        *refused = s->build_info;
        *fall_back = true;
        return YK_OK;
    }
    img.info.build_seconds = now_seconds() - t0;
    if (img.bvh->split_failed || img.dtree.n_nodes == 0) return fail(ctx, YK_ERR_BVH_BUILD, "BVH split failed (reference: assert_ne!(mid, start))");
    fill_scene_info(&img);
    if (img.info.n_nodes > YK_REF_INDEX_MAX || img.info.n_shapes > YK_REF_INDEX_MAX) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^28 BVH nodes or shapes");
    s->info = img.info;

    // small tables, records
    if ((rc = upload(ctx, s->mesh_flags, img.mesh_flags.data(), img.mesh_flags.size())) != YK_OK || (rc = upload(ctx, s->materials, img.mats.data(), img.mats.size())) != YK_OK ||
        (rc = upload(ctx, s->lights, img.lights.data(), img.lights.size())) != YK_OK || (rc = upload(ctx, s->spheres, img.spheres.data(), img.spheres.size())) != YK_OK ||
        (rc = upload(ctx, s->texels, img.texels.data(), img.texels.size())) != YK_OK || (rc = upload(ctx, s->tex_info, img.tex_info.data(), img.tex_info.size())) != YK_OK)
        return rc;
    const double l0 = now_seconds();
    bool order_applied = false;
    if (layout_scene_device(ctx, s, img.dtree, d_user, d_mat_kind, d->normals || d->uvs, img.bvh->depth, &order_applied) != YK_LAYOUT_REASON_NONE) {
        *fall_back = true;
        return YK_OK;
    }
    s->layout.layout = YK_LAYOUT_DEVICE;
    s->layout.seconds_layout = now_seconds() - l0;
    std::swap(s->tree_nodes, img.dtree.nodes);  // the host copy of the tree is made when something asks for it (scene_host_tree)
    std::swap(s->tree_order, img.dtree.order);
    std::swap(s->upd.depth, img.dtree.depth);  // kept for the scene's updates
    s->bvh = img.bvh;
    s->bvh_lazy = img.bvh_mut;
    s->tree_fetched.store(0u);
    s->lazy_mat_kind.swap(mat_kind);  // ... and so is the shape -> kind table (scene_shape_kind)
    s->lazy_sphere_kind.resize(d->n_spheres);
    for (uint32_t k = 0; k < d->n_spheres; ++k) s->lazy_sphere_kind[k] = s->lazy_mat_kind[(uint32_t)d->spheres[k].material];
    s->shape_kind_lazy = true;
    s->kind_fetched.store(0u);
    bind_device_scene(s, d);
    s->info.upload_seconds = now_seconds() - u0;
    guard.s = nullptr;
    *out = s;
    return YK_OK;
}

// The builder or the layout refused: the geometry goes to the host once and the host path builds the scene with the
// device layout asked for.  Where the builder refused, the host recursion builds the tree and the build info keeps the
// refusal (`refused`, with its reason); where the layout failed, the builder is asked again and the layout falls back
// as it does for host input.
static yk_status create_scene_from_host_copy(yk_context* ctx, const yk_scene_desc* d, hipStream_t st, const yk_bvh_build_info& refused, yk_scene** out) {
    const size_t nv = d->n_vertices, nt = d->n_triangles, ns = nt + d->n_spheres;
    std::vector<float> points(3 * nv), normals(d->normals ? 3 * nv : 0), uvs(d->uvs ? 2 * nv : 0);
    std::vector<uint32_t> indices(3 * nt), tri_mesh(d->tri_mesh ? nt : 0), order(d->shape_order ? ns : 0);
    std::vector<int32_t> tri_material(nt), tri_al(d->tri_area_light ? nt : 0);
    yk_scene_desc h = *d;
    auto fetch = [&](auto& v, const void* src) -> hipError_t { return v.empty() ? hipSuccess : hipMemcpyAsync(v.data(), src, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost, st); };
    HIP_TRY(ctx, fetch(points, d->points));
    HIP_TRY(ctx, fetch(normals, d->normals));
    HIP_TRY(ctx, fetch(uvs, d->uvs));
    HIP_TRY(ctx, fetch(indices, d->indices));
    HIP_TRY(ctx, fetch(tri_mesh, d->tri_mesh));
    HIP_TRY(ctx, fetch(tri_material, d->tri_material));
    HIP_TRY(ctx, fetch(tri_al, d->tri_area_light));
    HIP_TRY(ctx, fetch(order, d->shape_order));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    h.points = points.data();
    h.normals = d->normals ? normals.data() : nullptr;
    h.uvs = d->uvs ? uvs.data() : nullptr;
    h.indices = indices.data();
    h.tri_mesh = d->tri_mesh ? tri_mesh.data() : nullptr;
    h.tri_material = tri_material.data();
    h.tri_area_light = d->tri_area_light ? tri_al.data() : nullptr;
    h.shape_order = d->shape_order ? order.data() : nullptr;
    struct Options {  // this entry point always asks for the device builder and layout
        yk_context* ctx;
        int64_t builder, layout;
        ~Options() {
            ctx->bvh_builder = builder;
            ctx->scene_layout = layout;
        }
    } restore{ctx, ctx->bvh_builder, ctx->scene_layout};
    ctx->bvh_builder = refused.reason ? 0 : 1;
    ctx->scene_layout = 1;
    std::shared_ptr<SceneImage> img;
    yk_status rc = yk_build_scene_image(ctx, &h, img);
    if (rc != YK_OK || (rc = yk_upload_scene_image(ctx, img, out)) != YK_OK) return rc;
    if (refused.reason) {  // who built the tree is the host path's answer, why is the refusal's
        const uint32_t builder = (*out)->build_info.builder;
        (*out)->build_info = refused;
        (*out)->build_info.builder = builder;
    }
    return YK_OK;
}


// ------------------------------------------------------------------ yk_scene_update
// Update in place: the rule is yk_scene_update.h's, the device route yk_scene_update.hip's; here are the
// host route and the entry points.

static bool all_finite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        if (upd::not_finite_bits(u)) return false;
    }
    return true;
}

// what the kernels are handed, after either route rewrote the records
static void rebind_records(yk_scene* s) {
    const yk_scene_layout_info& li = s->layout;
    DevScene& ds = s->dev;
    ds.nodes = s->nodes.as<DevNode>();
    ds.nodes4 = li.wide ? s->nodes4.as<DevNode4>() : nullptr;
    s->wide_auto = li.wide_auto != 0;
    ds.top_nodes = s->top_nodes.as<DevNode>();
    ds.n_top = li.n_top;
    ds.top_nodes_any = s->top_nodes_any.as<DevNode>();
    ds.n_top_any = li.n_top_any;
    ds.tris = s->tris.as<float4>();
    ds.prim_shade = s->prim_shade.as<uint4>();
    ds.prim_attr = s->record_bytes[YK_RECORDS_PRIM_ATTR] ? s->prim_attr.as<float4>() : nullptr;
    ds.root_ref = li.root_ref;
    for (int k = 0; k < 3; ++k) {
        ds.root_bmin[k] = s->info.bounds_min[k];
        ds.root_bmax[k] = s->info.bounds_max[k];
    }
}

// The host route: yk_bvh_refit on a copy of the host tree, layout_records_host, an upload of the arrays and the records.
// `points` (and `normals`, may be NULL) are host arrays that have passed the finite test.  ctx NULL: a host-only scene.
static yk_status update_scene_host(yk_context* ctx, yk_scene* s, const float* points, const float* normals) {
    yk_scene::UpdateState& u = s->upd;
    const size_t nt = s->n_triangles, ns = s->n_spheres, nv = u.n_vertices;
    const HostBvh* old = scene_host_tree(s);
    if (!old) return fail(ctx, YK_ERR_DEVICE, "the scene's tree could not be copied back from the device");
    double t0 = now_seconds();
    if (ctx) (void)hipSetDevice(ctx->device);
    auto fetch = [&](auto& v, const DevBuf& src) -> hipError_t { return v.empty() ? hipSuccess : hipMemcpy(v.data(), src.p, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost); };
    std::vector<uint32_t> fetched_indices(ctx ? 3 * nt : 0);
    if (ctx) HIP_TRY(ctx, fetch(fetched_indices, s->indices));
    const uint32_t* indices = ctx ? fetched_indices.data() : u.host_indices.data();
    std::vector<float> sb(6 * (nt + ns));  // per source shape
    for (size_t i = 0; i < nt; ++i) {
        float b[6];
        (void)inp::tri_bound(points, indices, (uint32_t)i, b);
        std::memcpy(&sb[6 * i], b, sizeof(b));
    }
    std::copy(u.sphere_bounds.begin(), u.sphere_bounds.end(), sb.begin() + 6 * nt);
    std::shared_ptr<HostBvh> tree = std::make_shared<HostBvh>(*old);  // never through a tree that may be shared
    yk_status rc = yk_bvh_refit(tree->nodes.data(), tree->nodes.size(), tree->shape_order.data(), nt + ns, sb.data());
    if (rc != YK_OK) return fail(ctx, rc, "the scene's tree does not fit its shapes");
    u.info.seconds_boxes = now_seconds() - t0;
    t0 = now_seconds();
    if (ctx) {
        // the description's arrays as the host layout reads them: the new points and normals, everything else from the scene
        std::vector<float> old_normals(u.has_normals && !normals ? 3 * nv : 0), uvs(u.has_uvs ? 2 * nv : 0);
        std::vector<uint32_t> tri_mesh(nt), mesh_flags(s->mesh_flags.bytes / 4);
        std::vector<int32_t> tri_material(nt), tri_al(nt);
        std::vector<DevSphere> dev_spheres(ns);
        HIP_TRY(ctx, fetch(old_normals, s->normals));
        HIP_TRY(ctx, fetch(uvs, s->uvs));
        HIP_TRY(ctx, fetch(tri_mesh, s->tri_mesh));
        HIP_TRY(ctx, fetch(mesh_flags, s->mesh_flags));
        HIP_TRY(ctx, fetch(tri_material, s->tri_material));
        HIP_TRY(ctx, fetch(tri_al, s->tri_area_light));
        HIP_TRY(ctx, fetch(dev_spheres, s->spheres));
        std::vector<yk_sphere_desc> spheres(ns);
        for (size_t k = 0; k < ns; ++k) {
            std::memset(&spheres[k], 0, sizeof(spheres[k]));
            spheres[k].material = dev_spheres[k].material;
        }
        yk_scene_desc d;
        std::memset(&d, 0, sizeof(d));
        d.n_triangles = (uint32_t)nt;
        d.n_spheres = (uint32_t)ns;
        d.n_vertices = (uint32_t)nv;
        d.points = points;
        d.normals = normals ? normals : (u.has_normals ? old_normals.data() : nullptr);
        d.uvs = u.has_uvs ? uvs.data() : nullptr;
        d.indices = indices;
        d.tri_material = tri_material.data();
        d.tri_area_light = tri_al.data();
        d.spheres = spheres.data();
        SceneImage img;
        std::memset(&img.info, 0, sizeof(img.info));
        img.bvh = tree;
        img.d = &d;
        img.info.n_interior = s->info.n_interior;
        img.mat_kind.assign(u.mat_kind.begin(), u.mat_kind.end());
        img.mesh_flags.swap(mesh_flags);
        img.tri_mesh.swap(tri_mesh);
        {
            struct Options {  // the records as creation laid them out, whatever the context's options say today
                yk_context* ctx;
                int64_t top_nodes, wide_bvh;
                ~Options() {
                    ctx->top_nodes = top_nodes;
                    ctx->wide_bvh = wide_bvh;
                }
            } restore{ctx, ctx->top_nodes, ctx->wide_bvh};
            ctx->top_nodes = u.top_nodes;
            ctx->wide_bvh = u.wide_bvh;
            layout_records_host(ctx, &img);
        }
        if ((rc = upload(ctx, s->points, points, 3 * nv)) != YK_OK || (normals && (rc = upload(ctx, s->normals, normals, 3 * nv)) != YK_OK) ||
            (rc = upload(ctx, s->nodes, img.dn.data(), img.dn.size())) != YK_OK || (rc = upload(ctx, s->nodes4, img.dn4.data(), img.dn4.size())) != YK_OK ||
            (rc = upload(ctx, s->top_nodes, img.top.data(), img.top.size())) != YK_OK || (rc = upload(ctx, s->top_nodes_any, img.top_any.data(), img.top_any.size())) != YK_OK ||
            (rc = upload(ctx, s->tris, img.tris.data(), img.tris.size())) != YK_OK || (rc = upload(ctx, s->prim_shade, img.prim_shade.data(), img.prim_shade.size())) != YK_OK ||
            (rc = upload(ctx, s->prim_attr, img.prim_attr.data(), img.prim_attr.size())) != YK_OK)
            return rc;
        if (s->tree_nodes.p)  // the tree a later device-route update starts from
            HIP_TRY(ctx, hipMemcpy(s->tree_nodes.p, tree->nodes.data(), tree->nodes.size() * sizeof(yk_bvh_node), hipMemcpyHostToDevice));
        set_record_layout(s, s->info.n_interior, img.dn4.size(), img.top.size(), img.top_any.size(), s->info.n_shapes, u.has_normals || u.has_uvs, img.root_ref, img.wide_auto);
    }
    for (int k = 0; k < 3; ++k) {
        s->info.bounds_min[k] = tree->nodes[0].bmin[k];
        s->info.bounds_max[k] = tree->nodes[0].bmax[k];
    }
    {
        std::lock_guard<std::mutex> lock(s->tree_mu);
        s->bvh = tree;
        s->bvh_lazy.reset();
        s->tree_fetched.store(1u);
    }
    if (ctx) rebind_records(s);
    u.info.seconds_records = now_seconds() - t0;
    return YK_OK;
}

// everything the context has enqueued: renders of the scene that were enqueued before the update finish on the old geometry
static yk_status drain_context(yk_context* ctx) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (WorkSet& w : ctx->ws) {
        if (w.stream && w.stream != ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(w.stream));
        if (w.side) HIP_TRY(ctx, hipStreamSynchronize(w.side));
    }
    return YK_OK;
}

// The device route on device arrays; where it fails, the arrays go to the host once (h_points / h_normals when the caller
// has them there already) and the host route rewrites the scene.
static yk_status update_scene(yk_context* ctx, yk_scene* s, const float* d_points, const float* d_normals, const float* h_points, const float* h_normals) {
    yk_scene::UpdateState& u = s->upd;
    bool not_finite = false;
    const uint32_t reason = update_scene_device(ctx, s, d_points, d_normals, &not_finite);
    if (not_finite) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "points: coordinate not finite");
    if (reason == YK_LAYOUT_REASON_NONE) {  // the host copy of the tree is stale: the next reader fetches the refitted one
        std::lock_guard<std::mutex> lock(s->tree_mu);
        std::shared_ptr<HostBvh> fresh = std::make_shared<HostBvh>();
        fresh->max_leaf_shapes = s->bvh->max_leaf_shapes;
        fresh->depth = s->bvh->depth;
        fresh->split_failed = s->bvh->split_failed;
        s->bvh = s->bvh_lazy = fresh;
        s->tree_fetched.store(0u);
        rebind_records(s);
        u.info.route = YK_UPDATE_ROUTE_DEVICE;
        u.info.reason = YK_LAYOUT_REASON_NONE;
        return YK_OK;
    }
    (void)hipGetLastError();
    const size_t n = 3 * (size_t)u.n_vertices;
    std::vector<float> points(h_points ? 0 : n), normals(d_normals && !h_normals ? n : 0);
    if (!h_points) HIP_TRY(ctx, hipMemcpy(points.data(), d_points, n * 4, hipMemcpyDeviceToHost));
    if (d_normals && !h_normals) HIP_TRY(ctx, hipMemcpy(normals.data(), d_normals, n * 4, hipMemcpyDeviceToHost));
    if (!h_points) h_points = points.data();
    if (d_normals && !h_normals) h_normals = normals.data();
    if (!all_finite(h_points, n)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "points: coordinate not finite");
    const yk_status rc = update_scene_host(ctx, s, h_points, h_normals);
    u.info.route = YK_UPDATE_ROUTE_HOST;
    u.info.reason = reason;
    return rc;
}

// the arguments both entry points refuse alike
static yk_status check_update(yk_context* ctx, const yk_scene* s, const float* points, const float* normals) {
    if (!s) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene");
    if (!points) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null points");
    if (normals && !s->upd.has_normals) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "normals given for a scene created without normals");
    if (ctx ? (!s->on_device || s->device != ctx->device) : s->on_device) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "scene was not created on this context's device");
    return YK_OK;
}

static void finish_update(yk_scene* s, double t_begin) {
    s->upd.info.n_updates += 1;
    s->upd.info.seconds_total = now_seconds() - t_begin;
}

extern "C" {

yk_status yk_scene_create(yk_context* ctx, const yk_scene_desc* d, yk_scene** out) {
    std::unique_lock<std::recursive_mutex> yk_lock_;
    if (ctx) yk_lock_ = std::unique_lock<std::recursive_mutex>(ctx->mu);
    if (!d || !out) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene description");
    *out = nullptr;
    std::shared_ptr<SceneImage> img;
    yk_status st = yk_build_scene_image(ctx, d, img);
    if (st != YK_OK) return st;
    return yk_upload_scene_image(ctx, img, out);
}

yk_status yk_scene_create_device(yk_context* ctx, const yk_scene_desc* d, void* stream, yk_scene** out) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    if (!d || !out) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene description");
    *out = nullptr;
    yk_status rc = check_description(ctx, d, false);  // everything that reads host tables only
    if (rc != YK_OK) return rc;
    if ((uint64_t)d->n_triangles + d->n_spheres > YK_REF_INDEX_MAX) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^28 BVH nodes or shapes");
    (void)hipSetDevice(ctx->device);
    if ((rc = check_device_arrays(ctx, d)) != YK_OK) return rc;
    hipStream_t st = ctx->stream;
    if (stream) {  // the caller's arrays are complete where its stream stands now
        HIP_TRY(ctx, hipEventRecord(ctx->ev_in, (hipStream_t)stream));
        HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_in, 0));
    }
    bool fall_back = false;
    yk_bvh_build_info refused;
    rc = create_scene_on_device(ctx, d, st, out, &fall_back, &refused);
    if (rc != YK_OK || !fall_back) {
        if (rc != YK_OK) (void)hipStreamSynchronize(st);  // the caller may free its arrays on return
        return rc;
    }
    return create_scene_from_host_copy(ctx, d, st, refused, out);
} YK_CATCH(ctx)

yk_status yk_scene_update(yk_context* ctx, yk_scene* s, const float* points, const float* normals) try {
    std::unique_lock<std::recursive_mutex> yk_lock_;
    if (ctx) yk_lock_ = std::unique_lock<std::recursive_mutex>(ctx->mu);
    const double t_begin = now_seconds();
    yk_status rc = check_update(ctx, s, points, normals);
    if (rc != YK_OK) return rc;
    yk_scene::UpdateState& u = s->upd;
    const size_t n = 3 * (size_t)u.n_vertices;
    if (!all_finite(points, n)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "points: coordinate not finite");
    u.info.seconds_check = now_seconds() - t_begin;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        if ((rc = drain_context(ctx)) != YK_OK) return rc;
    }
    if (ctx && s->layout.layout == YK_LAYOUT_DEVICE) {  // the arrays go up and the device route runs
        DevScratch tmp;
        float *d_points = nullptr, *d_normals = nullptr;
        if (tmp.get(d_points, n) && (!normals || tmp.get(d_normals, n)) && hipMemcpy(d_points, points, n * 4, hipMemcpyHostToDevice) == hipSuccess &&
            (!normals || hipMemcpy(d_normals, normals, n * 4, hipMemcpyHostToDevice) == hipSuccess)) {
            rc = update_scene(ctx, s, d_points, d_normals, points, normals);
        } else {
            (void)hipGetLastError();
            rc = update_scene_host(ctx, s, points, normals);
            u.info.route = YK_UPDATE_ROUTE_HOST;
            u.info.reason = YK_LAYOUT_REASON_OUT_OF_MEMORY;
        }
    } else {
        rc = update_scene_host(ctx, s, points, normals);
        u.info.route = YK_UPDATE_ROUTE_HOST;
        u.info.reason = YK_LAYOUT_REASON_NONE;
    }
    if (rc == YK_OK) finish_update(s, t_begin);
    return rc;
} YK_CATCH(ctx)

yk_status yk_scene_update_device(yk_context* ctx, yk_scene* s, const float* d_points, const float* d_normals, void* stream) try {
    if (!ctx) return YK_ERR_INVALID_ARGUMENT;
    YK_LOCK(ctx);
    const double t_begin = now_seconds();
    yk_status rc = check_update(ctx, s, d_points, d_normals);
    if (rc != YK_OK) return rc;
    (void)hipSetDevice(ctx->device);
    yk_scene_desc d;  // the pointer checks of yk_scene_create_device, with its messages
    std::memset(&d, 0, sizeof(d));
    d.n_vertices = s->upd.n_vertices;
    d.points = d_points;
    d.normals = d_normals;
    if ((rc = check_device_arrays(ctx, &d)) != YK_OK) return rc;
    if (stream) {  // the caller's arrays are complete where its stream stands now
        HIP_TRY(ctx, hipEventRecord(ctx->ev_in, (hipStream_t)stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
    }
    if ((rc = drain_context(ctx)) != YK_OK) return rc;
    rc = update_scene(ctx, s, d_points, d_normals, nullptr, nullptr);
    if (rc == YK_OK) finish_update(s, t_begin);
    return rc;
} YK_CATCH(ctx)

yk_status yk_scene_get_update_info(const yk_scene* s, yk_scene_update_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->upd.info;
    return YK_OK;
}

void yk_scene_destroy(yk_scene* s) {
    if (!s) return;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    for (DevBuf* b : scene_buffers(s)) b->release();
    for (DevBuf* b : {&s->upd.depth, &s->upd.list, &s->upd.sphere_b, &s->upd.mat_kind_d, &s->upd.words}) b->release();
    delete s;
}

yk_status yk_scene_get_info(const yk_scene* s, yk_scene_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->info;
    return YK_OK;
}

yk_status yk_scene_get_build_info(const yk_scene* s, yk_bvh_build_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->build_info;
    return YK_OK;
}

yk_status yk_scene_export_bvh(const yk_scene* s, yk_bvh_node* nodes, uint32_t* shape_order) {
    if (!s) return YK_ERR_INVALID_ARGUMENT;
    const HostBvh* bvh = scene_host_tree(s);
    if (!bvh) return YK_ERR_DEVICE;
    if (nodes) std::memcpy(nodes, bvh->nodes.data(), bvh->nodes.size() * sizeof(yk_bvh_node));
    if (shape_order) std::memcpy(shape_order, bvh->shape_order.data(), bvh->shape_order.size() * sizeof(uint32_t));
    return YK_OK;
}

yk_status yk_scene_get_layout_info(const yk_scene* s, yk_scene_layout_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->layout;
    out->tree_fetched = s->tree_fetched.load();
    return YK_OK;
}

yk_status yk_scene_read_records(const yk_scene* s, uint32_t which, void* out, size_t cap_bytes, size_t* n_bytes) {
    if (!s || !s->on_device || which > YK_RECORDS_PRIM_ATTR || !n_bytes) return YK_ERR_INVALID_ARGUMENT;
    const DevBuf& buf = record_buffer(s, which);
    const size_t bytes = s->record_bytes[which];
    *n_bytes = bytes;
    if (!out) return YK_OK;
    if (cap_bytes < bytes || buf.bytes < bytes) return YK_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(s->device);
    if (bytes && hipMemcpy(out, buf.p, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return YK_ERR_DEVICE;
    }
    return YK_OK;
}

}  // extern "C"
