// yk_scene.cpp — a scene's creation, one pipeline (the record layouts are in yk_device.h):
//   inputs   a tree (the reference's BVH, bvh.rs:39-115 via yk_host.cpp, or the device builder's), the geometry, the small
//            tables and the LayoutOptions captured at creation — from a description, from arrays in HBM, or from the scene
//   layout   layout_records_host (yk_scene_records.cpp) + upload_records, or layout_scene_device (yk_scene_layout.hip)
//   bind     bind_records, at creation (inside bind_device_scene) and after a change in place
// Which builder and which layout is an argument (SceneBuild); nothing here writes a context option.
// Also here: the getters, scene_host_tree and scene_host_arrays.  yk_scene_change.cpp changes a live scene through the same calls.
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

// a scene under construction: destroyed (yk_scene_destroy) on every early return and on an exception, released into *out at the end
typedef std::unique_ptr<yk_scene, void (*)(yk_scene*)> ScenePtr;

// the counts a scene keeps of its description
static void set_scene_counts(yk_scene* s, const yk_scene_desc* d) {
    s->n_triangles = d->n_triangles;
    s->n_spheres = d->n_spheres;
    s->n_lights = d->n_lights;
    s->n_materials = d->n_materials;
    s->n_meshes = d->n_meshes;
    s->n_textures = d->n_textures;
    for (uint32_t l = 0; l < d->n_lights; ++l) s->n_delta_lights += d->lights[l].kind != YK_LIGHT_RECT ? 1u : 0u;
    s->upd.light_kind.resize(d->n_lights);  // an edit in place keeps every light's kind
    for (uint32_t l = 0; l < d->n_lights; ++l) s->upd.light_kind[l] = (uint8_t)d->lights[l].kind;
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

DevSphere make_sphere(const yk_sphere_desc& sp) {
    DevSphere o;
    std::memcpy(o.o2w, sp.object_to_world, 64);
    std::memcpy(o.w2o, sp.world_to_object, 64);
    o.radius = sp.radius;
    o.material = sp.material;
    o.swaps_handedness = inp::swaps_handedness(o.o2w) ? 1u : 0u;
    o.pad = 0;
    return o;
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

// The inputs of the pipeline as creation derives them from a scene description on the host (yk_internal.h): the tree, the
// small tables, the options the records are laid out with and — host layout — the records themselves.
struct SceneImage {
    std::shared_ptr<const HostBvh> bvh;
    std::shared_ptr<HostBvh> bvh_mut;  // the same tree, writable: its arrays are filled late when the builder left them in HBM
    // a device layout (single-device scenes): `rec` stays empty and yk_upload_scene_image lays the records out on the
    // device — from dtree, where the device builder left the tree (tree_on_device), or from an upload of the host tree
    bool device_layout = false, tree_on_device = false, order_applied = false;  // order_applied: the caller's shape order went into dtree.order
    uint32_t layout_reason = 0;  // YK_LAYOUT_REASON_*: why a device layout that was asked for is not attempted
    DeviceTree dtree;
    ~SceneImage() { dtree.release(); }
    const yk_scene_desc* d = nullptr;  // BORROWED: the caller's arrays (indices, points, normals, uvs, tri_material) are uploaded straight
                                       // from the description, so an image is only valid inside the call that built it
    yk_scene_info info;  // host part: node counts, bounds, build time
    yk_bvh_build_info build_info;
    LayoutOptions opt;  // the context's, captured when the image is built
    bool has_device_records = false;
    SceneRecords rec;  // of the host layout
    std::vector<float4> texels;
    std::vector<uint4> tex_info;
    std::vector<uint32_t> mesh_flags, tri_mesh;
    std::vector<uint8_t> mat_kind;  // device BSDF kind (MK_*) per material
    std::vector<int32_t> tri_al;
    std::vector<uint8_t> shape_kind;  // source shape -> BSDF kind (yk_scene::shape_kind)
    std::vector<Material> mats;
    std::vector<DevSphere> spheres;
    std::vector<DevLight> lights;
};

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

// Sphere::world_bound (sphere.rs:121-123): the rule is inp::sphere_bound's (yk_scene_input.h)
static ShapeBounds sphere_bound(const yk_sphere_desc& sp) {
    float six[6];
    inp::sphere_bound(sp.object_to_world, sp.radius, six);
    ShapeBounds b;
    std::memcpy(&b, six, sizeof(b));
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
static yk_status build_tree(yk_context* ctx, const yk_scene_desc* d, const std::vector<ShapeBounds>& sb, bool device_builder, SceneImage* s) {
    double t0 = now_seconds();
    // Who builds the tree: the host recursion unless the caller asks for the device builder or the environment
    // (YK_BVH_BUILDER=levels, YK_BVH_SMALL_RANGE=n; next to YK_BVH_THREADS) for the host instance of the level algorithm.
    // A level builder that refuses leaves its reason in the build info and the recursion builds the same tree.
    yk_bvh_build_info& bi = s->build_info;
    std::memset(&bi, 0, sizeof(bi));
    bool built = false;
    const char* env_builder = std::getenv("YK_BVH_BUILDER");
    if (ctx && device_builder) {
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
        s->mat_kind[m] = (uint8_t)(s->mats[m].kind & 7u);
    }
    s->mesh_flags.assign(std::max<uint32_t>(d->n_meshes, 1), 0);
    for (uint32_t m = 0; m < d->n_meshes; ++m)
        s->mesh_flags[m] = (d->meshes[m].has_normals ? YK_MESH_NORMALS : 0u) | (d->meshes[m].has_uvs ? YK_MESH_UVS : 0u) | (d->meshes[m].swaps_handedness ? YK_MESH_SWAPS : 0u);
    s->spheres.resize(std::max<uint32_t>(d->n_spheres, 1));
    for (uint32_t k = 0; k < d->n_spheres; ++k) s->spheres[k] = make_sphere(d->spheres[k]);
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
    for (uint32_t i = 0; i < d->n_triangles; ++i) s->shape_kind[i] = s->mat_kind[d->tri_material[i]];
    for (uint32_t k = 0; k < d->n_spheres; ++k) s->shape_kind[(size_t)d->n_triangles + k] = s->mat_kind[d->spheres[k].material];
    s->tri_mesh.assign(d->n_triangles, 0);
    if (d->tri_mesh) std::memcpy(s->tri_mesh.data(), d->tri_mesh, sizeof(uint32_t) * d->n_triangles);
    s->tri_al.assign(d->n_triangles, -1);
    if (d->tri_area_light) std::memcpy(s->tri_al.data(), d->tri_area_light, sizeof(int32_t) * d->n_triangles);
    return YK_OK;
}

// The host layout of an image: its input from the description and the image's own tables.
static void layout_image_host(SceneImage* s) {
    const yk_scene_desc* d = s->d;
    std::vector<int32_t> sphere_material(d->n_spheres);
    for (uint32_t k = 0; k < d->n_spheres; ++k) sphere_material[k] = d->spheres[k].material;
    HostLayoutInput in;
    in.bvh = s->bvh.get();
    in.n_interior = s->info.n_interior;
    in.indices = d->indices;
    in.points = d->points;
    in.normals = d->normals;
    in.uvs = d->uvs;
    in.tri_material = d->tri_material;
    in.tri_area_light = s->tri_al.data();
    in.tri_mesh = s->tri_mesh.data();
    in.mesh_flags = s->mesh_flags.data();
    in.n_triangles = d->n_triangles;
    in.sphere_material = sphere_material.data();
    in.mat_kind = s->mat_kind.data();
    in.opt = s->opt;
    s->rec = layout_records_host(in);
}

// Host half of yk_scene_create: validation, BoundingVolumeHierarchy::new (bvh.rs:39-115) and — when `ctx` is given (its
// "top_nodes" / "wide_bvh" options are captured here) — the small tables and, unless the device lays out, the records.
yk_status yk_build_scene_image(yk_context* ctx, const yk_scene_desc* d, std::shared_ptr<SceneImage>& out, const SceneBuild& what) try {
    if (!d) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene description");
    out.reset();
    yk_status st = check_description(ctx, d);
    if (st != YK_OK) return st;

    std::shared_ptr<SceneImage> img = std::make_shared<SceneImage>();
    SceneImage* s = img.get();
    s->bvh = s->bvh_mut = std::make_shared<HostBvh>();
    s->d = d;
    s->device_layout = ctx && what.device_layout;
    s->layout_reason = ctx ? what.layout_reason : 0u;
    if (ctx) s->opt = LayoutOptions{ctx->top_nodes, ctx->wide_bvh};
    std::memset(&s->info, 0, sizeof(s->info));

    std::vector<ShapeBounds> sb;
    if ((st = shape_bounds(ctx, d, sb)) != YK_OK || (st = build_tree(ctx, d, sb, what.device_builder, s)) != YK_OK) return st;
    fill_scene_info(s);
    if (ctx) {  // device records (a host-only scene — ctx == NULL — stops at the tree)
        if (s->info.n_nodes > YK_REF_INDEX_MAX || s->info.n_shapes > YK_REF_INDEX_MAX) return fail(ctx, YK_ERR_UNSUPPORTED, "more than 2^28 BVH nodes or shapes");
        if ((st = host_tables(ctx, d, s)) != YK_OK) return st;
        if (!s->device_layout) layout_image_host(s);
        s->has_device_records = true;
    }
    out = img;
    return YK_OK;
} YK_CATCH(ctx)

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

yk_status scene_host_arrays(yk_context* ctx, const yk_scene* s, uint32_t mask, const std::string& who, HostArrays& out) {
    const size_t nt = s->n_triangles, nv = s->upd.n_vertices;
    if (!s->on_device) {
        const yk_scene::HostCopy& h = s->host;
        if ((mask & HOST_INDICES) && h.indices.size() != 3 * nt) return fail(ctx, YK_ERR_INVALID_ARGUMENT, who + "the scene has no vertex indices");
        if ((mask & HOST_POINTS) && nt && h.points.size() != 3 * nv) return fail(ctx, YK_ERR_INVALID_ARGUMENT, who + "the scene has no vertices on the host");
        if ((mask & HOST_SPHERES) && h.spheres.size() < s->n_spheres) return fail(ctx, YK_ERR_INVALID_ARGUMENT, who + "the scene has no sphere table");
        out.arrays = &h;
        return YK_OK;
    }
    (void)hipSetDevice(s->device);
    yk_scene::HostCopy& h = out.fetched;
    out.arrays = &h;
    const auto get = [mask](uint32_t bit, auto& v, size_t count, const DevBuf& b) -> hipError_t {
        const size_t bytes = count * sizeof(v[0]);
        if (!(mask & bit) || bytes == 0) return hipSuccess;
        if (!b.p || b.bytes < bytes) return hipErrorInvalidValue;
        v.resize(count);
        return hipMemcpy(v.data(), b.p, bytes, hipMemcpyDeviceToHost);
    };
    HIP_TRY(ctx, get(HOST_INDICES, h.indices, 3 * nt, s->indices));
    HIP_TRY(ctx, get(HOST_POINTS, h.points, 3 * nv, s->points));
    HIP_TRY(ctx, get(HOST_NORMALS, h.normals, s->upd.has_normals ? 3 * nv : 0, s->normals));
    HIP_TRY(ctx, get(HOST_UVS, h.uvs, s->upd.has_uvs ? 2 * nv : 0, s->uvs));
    HIP_TRY(ctx, get(HOST_TRI_MESH, h.tri_mesh, nt, s->tri_mesh));
    HIP_TRY(ctx, get(HOST_TRI_MATERIAL, h.tri_material, nt, s->tri_material));
    HIP_TRY(ctx, get(HOST_TRI_AREA_LIGHT, h.tri_area_light, nt, s->tri_area_light));
    HIP_TRY(ctx, get(HOST_MESH_FLAGS, h.mesh_flags, std::max<uint32_t>(s->n_meshes, 1), s->mesh_flags));
    HIP_TRY(ctx, get(HOST_MATERIALS, h.materials, std::max<uint32_t>(s->n_materials, 1), s->materials));
    HIP_TRY(ctx, get(HOST_SPHERES, h.spheres, std::max<uint32_t>(s->n_spheres, 1), s->spheres));
    HIP_TRY(ctx, get(HOST_TEXTURES, h.tex_info, s->n_textures, s->tex_info));
    size_t n_texels = 0;
    for (const uint4& t : h.tex_info) n_texels = std::max(n_texels, (size_t)t.x + (size_t)t.y * t.z);
    HIP_TRY(ctx, get(HOST_TEXTURES, h.texels, n_texels, s->texels));
    return YK_OK;
}

hipError_t upload_host_tree(const HostBvh& bvh, DeviceTree& tree) {
    const std::vector<uint32_t> depth = lay::node_depths(reinterpret_cast<const uint32_t*>(bvh.nodes.data()), bvh.nodes.size());  // children follow their parent in the array
    tree.n_nodes = (uint32_t)bvh.nodes.size();
    tree.n_shapes = (uint32_t)bvh.shape_order.size();
    std::memcpy(tree.root_words, bvh.nodes.data(), 32);
    hipError_t e = put_host_array(tree.nodes, bvh.nodes.data(), bvh.nodes.size() * sizeof(yk_bvh_node));
    if (e == hipSuccess) e = put_host_array(tree.depth, depth.data(), depth.size() * 4);
    if (e == hipSuccess) e = put_host_array(tree.order, bvh.shape_order.data(), bvh.shape_order.size() * 4);
    return e;
}

void adopt_device_tree(yk_scene* s, DeviceTree& tree, const std::shared_ptr<HostBvh>& lazy) {
    std::swap(s->tree_nodes, tree.nodes);
    std::swap(s->tree_order, tree.order);
    std::swap(s->upd.depth, tree.depth);  // kept for the scene's updates
    if (lazy) {  // the host copy of the arrays is made when something asks for it (scene_host_tree)
        s->bvh_lazy = lazy;
        s->tree_fetched.store(0u);
    }
}

// The device layout of an image: the tree to HBM unless the builder left it there, the two small tables, the layout kernels
// (yk_scene_layout.hip).  The scene's own arrays (indices .. spheres) are uploaded already.  Returns YK_LAYOUT_REASON_*.
static uint32_t layout_on_device(yk_context* ctx, SceneImage* img, yk_scene* s) {
    const yk_scene_desc* d = img->d;
    DeviceTree& tree = img->dtree;
    double t0 = now_seconds();
    const bool user_order = img->tree_on_device && d->shape_order;  // a host-built tree's order has it applied already
    DevScratch tmp;
    uint8_t* d_mat_kind = nullptr;
    uint32_t* d_user = nullptr;
    if (!tmp.get(d_mat_kind, img->mat_kind.size()) || (user_order && !tmp.get(d_user, tree.n_shapes))) return layout_reason_of(tmp.err);
    hipError_t e = hipMemcpy(d_mat_kind, img->mat_kind.data(), img->mat_kind.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && user_order) e = hipMemcpy(d_user, d->shape_order, (size_t)tree.n_shapes * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !img->tree_on_device) e = upload_host_tree(*img->bvh, tree);
    if (e != hipSuccess) return layout_reason_of(e);
    s->layout.seconds_upload = now_seconds() - t0;
    t0 = now_seconds();
    const uint32_t r = layout_scene_device(ctx, s, tree, d_user, d_mat_kind, d->normals || d->uvs, img->bvh->depth, &img->order_applied);
    s->layout.seconds_layout = now_seconds() - t0;
    if (r != YK_LAYOUT_REASON_NONE) return r;
    if (img->tree_on_device) adopt_device_tree(s, tree, img->bvh_mut);
    tree.release();
    return YK_LAYOUT_REASON_NONE;
}

yk_status upload_records(yk_context* ctx, yk_scene* s, const SceneRecords& r) {
    yk_status st;
    if ((st = upload(ctx, s->nodes, r.nodes.data(), r.nodes.size())) != YK_OK || (st = upload(ctx, s->nodes4, r.nodes4.data(), r.nodes4.size())) != YK_OK ||
        (st = upload(ctx, s->top_nodes, r.top.data(), r.top.size())) != YK_OK || (st = upload(ctx, s->top_nodes_any, r.top_any.data(), r.top_any.size())) != YK_OK ||
        (st = upload(ctx, s->tris, r.tris.data(), r.tris.size())) != YK_OK || (st = upload(ctx, s->prim_shade, r.prim_shade.data(), r.prim_shade.size())) != YK_OK ||
        (st = upload(ctx, s->prim_attr, r.prim_attr.data(), r.prim_attr.size())) != YK_OK)
        return st;
    // prim_attr is 4 * n_shapes records where the scene has normals or uvs and empty otherwise; a scene has at least one shape
    set_record_layout(s, s->info.n_interior, r.nodes4.size(), r.top.size(), r.top_any.size(), s->info.n_shapes, !r.prim_attr.empty(), r.root_ref, r.wide_auto);
    return YK_OK;
}

void bind_records(yk_scene* s) {
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
    for (int k = 0; k < 3; ++k) {  // node 0's box
        ds.root_bmin[k] = s->info.bounds_min[k];
        ds.root_bmax[k] = s->info.bounds_max[k];
    }
}

// The DevScene the kernels are handed: the records, then the scene's own arrays and the description's scalars.
static void bind_device_scene(yk_scene* s, const yk_scene_desc* d) {
    bind_records(s);
    DevScene& ds = s->dev;
    ds.spheres = d->n_spheres ? s->spheres.as<DevSphere>() : nullptr;
    ds.n_triangles = d->n_triangles;
    for (int k = 0; k < 3; ++k) ds.background[k] = d->background[k];
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

// What a change in place needs of the description after creation (yk_scene::UpdateState).
static void init_update_state(yk_scene* s, const yk_scene_desc* d, const LayoutOptions& opt, const std::vector<uint8_t>& mat_kind) {
    yk_scene::UpdateState& u = s->upd;
    u.n_vertices = d->n_vertices;
    u.has_normals = d->normals != nullptr;
    u.has_uvs = d->uvs != nullptr;
    u.opt = opt;
    u.mat_kind = mat_kind;
    u.sphere_bounds.resize(6 * (size_t)d->n_spheres);  // bmin, bmax per sphere: a ShapeBounds is those six floats
    for (uint32_t k = 0; k < d->n_spheres; ++k) {
        const ShapeBounds b = sphere_bound(d->spheres[k]);
        std::memcpy(&u.sphere_bounds[6 * (size_t)k], &b, sizeof(b));
    }
}

// Device half: one copy of the image in the HBM of ctx's device.
yk_status yk_upload_scene_image(yk_context* ctx, const std::shared_ptr<SceneImage>& img, yk_scene** out) try {
    if (!out) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (!img || !img->bvh) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene image");
    ScenePtr guard(new yk_scene(), yk_scene_destroy);
    yk_scene* s = guard.get();
    s->device = ctx ? ctx->device : -1;
    s->bvh = img->bvh;
    set_scene_counts(s, img->d);
    s->info = img->info;
    s->build_info = img->build_info;
    s->shape_kind = img->shape_kind;
    init_update_state(s, img->d, img->opt, img->mat_kind);
    if (!ctx) {  // a host-only scene keeps its arrays (yk_scene::HostCopy)
        const yk_scene_desc* d = img->d;
        SceneImage tables;
        yk_status st = small_tables(nullptr, d, &tables);
        if (st != YK_OK) return st;
        yk_scene::HostCopy& h = s->host;
        h.mesh_flags.swap(tables.mesh_flags);
        h.materials.swap(tables.mats);
        h.spheres.swap(tables.spheres);
        h.texels.swap(tables.texels);
        h.tex_info.swap(tables.tex_info);
        h.tri_mesh.assign(d->n_triangles, 0);
        if (d->tri_mesh) std::memcpy(h.tri_mesh.data(), d->tri_mesh, sizeof(uint32_t) * d->n_triangles);
        if (d->n_triangles) h.tri_material.assign(d->tri_material, d->tri_material + d->n_triangles);
        h.tri_area_light.assign(d->n_triangles, -1);  // what yk_scene_transform tests: a mesh that carries an area light does not move
        if (d->tri_area_light) std::memcpy(h.tri_area_light.data(), d->tri_area_light, sizeof(int32_t) * d->n_triangles);
        if (d->uvs) h.uvs.assign(d->uvs, d->uvs + 2 * (size_t)d->n_vertices);
        if (d->n_triangles) h.indices.assign(d->indices, d->indices + 3 * (size_t)d->n_triangles);
        if (d->n_triangles) h.points.assign(d->points, d->points + 3 * (size_t)d->n_vertices);
    }
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
                layout_image_host(img.get());
            }
        }
#undef UP
        if (li.layout == YK_LAYOUT_HOST && (st = upload_records(ctx, s, img->rec)) != YK_OK) return st;
        bind_device_scene(s, d);
        s->info.upload_seconds = now_seconds() - u0;
    }
    *out = guard.release();
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

yk_status check_device_arrays(yk_context* ctx, std::initializer_list<DeviceArray> arrays) {
    for (const DeviceArray& a : arrays) {
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

yk_status wait_for_caller_stream(yk_context* ctx, void* stream) {
    if (!stream) return YK_OK;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_in, (hipStream_t)stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
    return YK_OK;
}

// The device route.  *fall_back: the builder or the layout refused and the caller builds the scene by the host path — *refused
// then holds the builder's info with its reason (reason 0: it was the layout); any other failure is final.
static yk_status create_scene_on_device(yk_context* ctx, const yk_scene_desc* d, hipStream_t st, yk_scene** out, bool* fall_back, yk_bvh_build_info* refused) {
    *fall_back = false;
    std::memset(refused, 0, sizeof(*refused));
    const uint32_t nt = d->n_triangles, N = nt + d->n_spheres;
    ScenePtr guard(new yk_scene(), yk_scene_destroy);
    yk_scene* s = guard.get();
    s->device = ctx->device;
    set_scene_counts(s, d);
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
    std::vector<uint8_t> light_kind(std::max<uint32_t>(d->n_lights, 1), 0);
    std::vector<uint8_t>& mat_kind = img.mat_kind;
    init_update_state(s, d, LayoutOptions{ctx->top_nodes, ctx->wide_bvh}, mat_kind);
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
    s->bvh = img.bvh;
    adopt_device_tree(s, img.dtree, img.bvh_mut);
    s->lazy_mat_kind.swap(mat_kind);  // the shape -> kind table is made when something asks for it, too (scene_shape_kind)
    s->lazy_sphere_kind.resize(d->n_spheres);
    for (uint32_t k = 0; k < d->n_spheres; ++k) s->lazy_sphere_kind[k] = s->lazy_mat_kind[(uint32_t)d->spheres[k].material];
    s->shape_kind_lazy = true;
    s->kind_fetched.store(0u);
    bind_device_scene(s, d);
    s->info.upload_seconds = now_seconds() - u0;
    *out = guard.release();
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
    yk_scene_desc h = *d;  // the caller's description, its large arrays repointed at the host copies
    auto fetch = [&](auto& v, auto& field) -> hipError_t {
        const void* src = field;
        field = v.empty() ? nullptr : v.data();
        return v.empty() ? hipSuccess : hipMemcpyAsync(v.data(), src, v.size() * sizeof(v[0]), hipMemcpyDeviceToHost, st);
    };
    HIP_TRY(ctx, fetch(points, h.points));
    HIP_TRY(ctx, fetch(normals, h.normals));
    HIP_TRY(ctx, fetch(uvs, h.uvs));
    HIP_TRY(ctx, fetch(indices, h.indices));
    HIP_TRY(ctx, fetch(tri_mesh, h.tri_mesh));
    HIP_TRY(ctx, fetch(tri_material, h.tri_material));
    HIP_TRY(ctx, fetch(tri_al, h.tri_area_light));
    HIP_TRY(ctx, fetch(order, h.shape_order));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::shared_ptr<SceneImage> img;  // this entry point always asks for the device layout, and for the device builder unless it has refused
    yk_status rc = yk_build_scene_image(ctx, &h, img, SceneBuild{refused.reason == 0, true, 0u});
    if (rc != YK_OK || (rc = yk_upload_scene_image(ctx, img, out)) != YK_OK) return rc;
    if (refused.reason) {  // who built the tree is the host path's answer, why is the refusal's
        const uint32_t builder = (*out)->build_info.builder;
        (*out)->build_info = refused;
        (*out)->build_info.builder = builder;
    }
    return YK_OK;
}

extern "C" {

yk_status yk_scene_create(yk_context* ctx, const yk_scene_desc* d, yk_scene** out) {
    std::unique_lock<std::recursive_mutex> yk_lock_;
    if (ctx) yk_lock_ = std::unique_lock<std::recursive_mutex>(ctx->mu);
    if (!d || !out) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene description");
    *out = nullptr;
    std::shared_ptr<SceneImage> img;
    const SceneBuild what{ctx && ctx->bvh_builder == 1, ctx && ctx->scene_layout == 1, 0u};  // what the context's options ask for
    yk_status st = yk_build_scene_image(ctx, d, img, what);
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
    const size_t nv = d->n_vertices, nt = d->n_triangles, ns = nt + d->n_spheres;
    rc = check_device_arrays(ctx, {{"points", d->points, 12 * nv}, {"normals", d->normals, 12 * nv}, {"uvs", d->uvs, 8 * nv},
                                   {"indices", d->indices, 12 * nt}, {"tri_mesh", d->tri_mesh, 4 * nt}, {"tri_material", d->tri_material, 4 * nt},
                                   {"tri_area_light", d->tri_area_light, 4 * nt}, {"shape_order", d->shape_order, 4 * ns}});
    if (rc != YK_OK) return rc;
    hipStream_t st = ctx->stream;
    if ((rc = wait_for_caller_stream(ctx, stream)) != YK_OK) return rc;
    bool fall_back = false;
    yk_bvh_build_info refused;
    rc = create_scene_on_device(ctx, d, st, out, &fall_back, &refused);
    if (rc != YK_OK || !fall_back) {
        if (rc != YK_OK) (void)hipStreamSynchronize(st);  // the caller may free its arrays on return
        return rc;
    }
    return create_scene_from_host_copy(ctx, d, st, refused, out);
} YK_CATCH(ctx)

yk_status yk_scene_get_update_info(const yk_scene* s, yk_scene_update_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->upd.info;
    return YK_OK;
}

yk_status yk_scene_get_edit_info(const yk_scene* s, yk_scene_edit_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->upd.edit_info;
    return YK_OK;
}

yk_status yk_scene_get_transform_info(const yk_scene* s, yk_scene_transform_info* out) {
    if (!s || !out) return YK_ERR_INVALID_ARGUMENT;
    *out = s->xf.info;
    return YK_OK;
}

void yk_scene_destroy(yk_scene* s) {
    if (!s) return;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    for (DevBuf* b : scene_buffers(s)) b->release();
    for (DevBuf* b : {&s->upd.depth, &s->upd.list, &s->upd.sphere_b, &s->upd.mat_kind_d, &s->upd.words}) b->release();
    for (DevBuf* b : {&s->xf.rest_points, &s->xf.rest_normals, &s->xf.vertex_mesh, &s->xf.mesh_words, &s->xf.cost_words}) b->release();
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
