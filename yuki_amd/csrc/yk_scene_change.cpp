// yk_scene_change.cpp — a live scene changed in place ("One plan, one prelude, named phases"): the entry points
// yk_scene_update[_device], yk_scene_apply_edit[_device] and yk_scene_transform[_device], their prelude and the phases (Change)
// that run a ChangePlan (yk_scene_change.h) and the host route.  The device route's steps are yk_scene_update.hip's,
// yk_scene_edit.hip's and yk_scene_transform.hip's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "yk_internal.h"
#include "yk_scene_change.h"
#include "yk_scene_transform.h"
#include "yk_scene_update.h"

using namespace yk_change;

namespace {

bool all_finite(const float* p, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        if (upd::not_finite_bits(u)) return false;
    }
    return true;
}

// An array the call brings: on the host, on the device, or — once it went up for staging or came down for the host route — both.
template <class T> struct Brought {
    const T *h = nullptr, *d = nullptr;
    std::vector<T> fetched;
    hipError_t to_device(DevScratch& tmp, size_t count) {
        T* up = nullptr;
        if (!tmp.get(up, count)) return tmp.err;
        d = up;
        return hipMemcpy(up, h, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess ? hipSuccess : hipErrorUnknown;  // no allocation that failed
    }
    hipError_t to_host(size_t count) {
        if (h || !d || !count) return hipSuccess;
        fetched.resize(count);
        h = fetched.data();
        return hipMemcpy(fetched.data(), d, count * sizeof(T), hipMemcpyDeviceToHost);
    }
};

// the host tables of an edit, checked against the scene: yk_scene_create's checks with its messages, and the two of an edit
yk_status check_edit_tables(yk_context* ctx, const yk_scene* s, const yk_scene_edit* e) {
    if (e->lights)
        for (uint32_t l = 0; l < s->n_lights; ++l)
            if ((uint8_t)e->lights[l].kind != s->upd.light_kind[l] || e->lights[l].kind > 255u) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "lights: a light's kind cannot change");
    if (e->spheres) {
        for (uint32_t k = 0; k < s->n_spheres; ++k)
            if (e->spheres[k].material < 0 || (uint32_t)e->spheres[k].material >= s->n_materials) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "sphere material out of range");
        for (uint32_t k = 0; k < s->n_spheres; ++k)
            if (!all_finite(reinterpret_cast<const float*>(&e->spheres[k]), 33)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "spheres: matrix entry or radius not finite");  // two matrices and the radius
    }
    if (e->materials)
        for (uint32_t m = 0; m < s->n_materials; ++m)
            if ((e->materials[m].flags & YK_MAT_FLAG_TEXTURED_A) && e->materials[m].kind == YK_MAT_MATTE && e->materials[m].a_texture >= s->n_textures)
                return fail(ctx, YK_ERR_INVALID_ARGUMENT, "material texture index out of range");
    return YK_OK;
}

// Every kind table the scene keeps, from u.mat_kind (just rewritten): the plan's device copy, the lazy pair, the filled shape table.
yk_status refresh_kind_tables(yk_context* ctx, yk_scene* s, const std::vector<int32_t>& sphere_material) {
    yk_scene::UpdateState& u = s->upd;
    if (ctx && u.mat_kind_d.p) HIP_TRY(ctx, put_host_array(u.mat_kind_d, u.mat_kind.data(), u.mat_kind.size()));
    if (s->shape_kind_lazy) {
        s->lazy_mat_kind = u.mat_kind;
        for (uint32_t k = 0; k < s->n_spheres; ++k) s->lazy_sphere_kind[k] = u.mat_kind[(uint32_t)sphere_material[k]];
    }
    const bool filled = s->shape_kind_lazy ? s->kind_fetched.load() != 0u : !s->shape_kind.empty();
    if (!filled) return YK_OK;  // a lazy table is filled from the pair above when something asks; a host-only scene has none
    HostArrays have;
    const yk_status rc = scene_host_arrays(ctx, s, HOST_TRI_MATERIAL, "", have);
    if (rc != YK_OK) return rc;
    const std::vector<int32_t>& mat = have->tri_material;
    if (mat.size() != s->n_triangles || s->shape_kind.size() != (size_t)s->n_triangles + s->n_spheres) return fail(ctx, YK_ERR_DEVICE, "the scene's shape kinds do not fit its shapes");
    for (uint32_t i = 0; i < s->n_triangles; ++i) s->shape_kind[i] = u.mat_kind[(uint32_t)mat[i]];
    for (uint32_t k = 0; k < s->n_spheres; ++k) s->shape_kind[(size_t)s->n_triangles + k] = u.mat_kind[(uint32_t)sphere_material[k]];
    return YK_OK;
}

// One change: the prelude of every entry point (the constructor, scene, wait: an entry point's own refusals stand between
// them, in the order they always had), then the phases, which are named as the info structs name their times.
struct Change {
    yk_context* ctx;  // NULL: a host-only scene
    std::unique_lock<std::recursive_mutex> lock;
    double t_begin;
    yk_scene* s = nullptr;
    ChangeFacts facts;
    ChangePlan plan;
    uint32_t reason = YK_LAYOUT_REASON_NONE;  // of the device step that failed
    Brought<float> points, normals;           // an update's arrays ...
    const yk_scene_edit* e = nullptr;         // ... or an edit's tables, the spheres maybe on the device
    Brought<yk_sphere_desc> spheres;
    std::vector<Material> mats;  // made of e->materials before anything of the scene is written
    std::vector<uint8_t> mat_kind;
    DevScratch tmp;  // uploads for staging, and what the stage wrote
    StagedSpheres staged;
    Brought<yk_mesh_transform> xf;                    // ... or a transform's records
    std::vector<float> xf_points, xf_normals;         // what the host route made of the rest pose (points.h, normals.h)
    std::vector<uint32_t> xf_flags;                   // ... and the mesh flags that go with them
    uint32_t n_moved = 0, n_flipped = 0;
    double tree_cost = 0.0;
    double check = 0.0, tables = 0.0, boxes = 0.0, records = 0.0;  // the phases' seconds: the info structs are filled from these
    explicit Change(yk_context* c) : ctx(c) {
        if (ctx) lock = std::unique_lock<std::recursive_mutex>(ctx->mu);
        t_begin = now_seconds();
    }
    // the scene is this context's, and the context's device is current
    yk_status scene(yk_scene* sc) {
        if (ctx ? (!sc->on_device || sc->device != ctx->device) : sc->on_device) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "scene was not created on this context's device");
        if (ctx) (void)hipSetDevice(ctx->device);
        s = sc;
        facts.has_context = ctx != nullptr;
        facts.device_laid = ctx && s->layout.layout == YK_LAYOUT_DEVICE;
        facts.n_spheres = s->n_spheres;
        facts.n_lights = s->n_lights;
        facts.n_materials = s->n_materials;
        return YK_OK;
    }
    // the caller's stream, then everything the context has enqueued: renders enqueued before the change finish on the old scene
    yk_status wait(void* stream) {
        if (!ctx) return YK_OK;
        const yk_status rc = wait_for_caller_stream(ctx, stream);
        if (rc != YK_OK) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (WorkSet& w : ctx->ws) {
            if (w.stream && w.stream != ctx->stream) HIP_TRY(ctx, hipStreamSynchronize(w.stream));
            if (w.side) HIP_TRY(ctx, hipStreamSynchronize(w.side));
        }
        return YK_OK;
    }

    yk_status run() {
        plan = plan_change(facts);
        yk_status rc = plan.transform ? check_and_stage_transform() : check_and_stage();
        if (rc == YK_OK && (rc = write_tables()) == YK_OK && (rc = boxes_and_records()) == YK_OK && (rc = cost_of_tree()) == YK_OK) publish();
        return rc;
    }

    // The rest pose on the host for the host route of a transform: snapshotted now where the scene has none (a host-only scene keeps
    // no normals and has no records that read them), fetched where a device-route call left it in HBM.
    struct RestOnHost {
        const float *points = nullptr, *normals = nullptr;
        const uint32_t *vertex_mesh = nullptr, *mesh_lit = nullptr, *flags_created = nullptr;
        std::vector<float> f_points, f_normals;
        std::vector<uint32_t> f_vertex_mesh, f_words;
    };
    yk_status rest_on_host(RestOnHost& r) {
        yk_scene::TransformState& x = s->xf;
        const size_t nv = s->upd.n_vertices, nt = s->n_triangles, run = std::max<uint32_t>(s->n_meshes, 1u);
        const bool normals_kept = ctx && s->upd.has_normals;
        if (ctx && !x.active) {  // a scene in device memory keeps its rest pose there whatever the route: the motion pass reads it
            const uint32_t why = snapshot_rest_device(ctx, s, false);
            if (why != YK_LAYOUT_REASON_NONE)
                return fail(ctx, why == YK_LAYOUT_REASON_OUT_OF_MEMORY ? YK_ERR_OUT_OF_MEMORY : YK_ERR_DEVICE, "transforms: the rest pose could not be kept in device memory");
        }
        if (!x.active) {  // a host-only scene: in its own vectors
            HostArrays have;
            yk_status rc = scene_host_arrays(ctx, s, HOST_INDICES | HOST_POINTS | HOST_TRI_MESH | HOST_TRI_AREA_LIGHT | HOST_MESH_FLAGS, "", have);
            if (rc != YK_OK) return rc;
            const HostBvh* bvh = scene_host_tree(s);
            if (!bvh) return fail(ctx, YK_ERR_DEVICE, "the scene's tree could not be copied back from the device");
            if (have->tri_mesh.size() != nt || have->tri_area_light.size() != nt || have->mesh_flags.size() < run) return fail(ctx, YK_ERR_DEVICE, "the scene's mesh tables do not fit its triangles");
            x.h_rest_points.assign(have->points.begin(), have->points.end());
            x.h_rest_points.resize(3 * nv);
            x.flags_created.assign(have->mesh_flags.begin(), have->mesh_flags.begin() + run);
            x.h_vertex_mesh.assign(2 * nv, 0u);
            for (size_t v = 0; v < nv; ++v) x.h_vertex_mesh[2 * v] = xfm::XF_NO_MESH;
            x.h_mesh_lit.assign(run, 0u);
            x.shared = false;
            for (size_t t = 0; t < nt; ++t) {
                const uint32_t mesh = have->tri_mesh[t];
                for (int k = 0; k < 3; ++k)
                    if (have->indices[3 * t + k] < nv) xfm::table_add(x.h_vertex_mesh.data(), have->indices[3 * t + k], mesh);
                if (have->tri_area_light[t] >= 0 && mesh < s->n_meshes) x.h_mesh_lit[mesh] = 1u;
            }
            for (size_t v = 0; v < nv; ++v) x.shared = x.shared || xfm::vertex_shared(x.h_vertex_mesh[2 * v], x.h_vertex_mesh[2 * v + 1]);
            x.info.tree_cost_rest = xfm::tree_cost(reinterpret_cast<const uint32_t*>(bvh->nodes.data()), bvh->nodes.size());
            x.info.rest_bytes = 4 * (x.h_rest_points.size() + x.h_vertex_mesh.size() + x.h_mesh_lit.size() + x.flags_created.size());
            x.active = true;
        }
        if (!x.rest_points.p) {
            r.points = x.h_rest_points.data();
            r.vertex_mesh = x.h_vertex_mesh.data();
            r.mesh_lit = x.h_mesh_lit.data();
            r.flags_created = x.flags_created.data();
            return YK_OK;
        }
        r.f_points.resize(3 * nv);  // a scene in device memory: it comes down for the call (yk_scene_transform.hip: mesh_words holds lit, kinds, created)
        r.f_vertex_mesh.resize(2 * nv);
        r.f_words.resize(3 * run);
        if (nv) HIP_TRY(ctx, hipMemcpy(r.f_points.data(), x.rest_points.p, 12 * nv, hipMemcpyDeviceToHost));
        if (nv) HIP_TRY(ctx, hipMemcpy(r.f_vertex_mesh.data(), x.vertex_mesh.p, 8 * nv, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(r.f_words.data(), x.mesh_words.p, 12 * run, hipMemcpyDeviceToHost));
        if (normals_kept) {
            r.f_normals.resize(3 * nv);
            if (nv) HIP_TRY(ctx, hipMemcpy(r.f_normals.data(), x.rest_normals.p, 12 * nv, hipMemcpyDeviceToHost));
            r.normals = r.f_normals.data();
        }
        r.points = r.f_points.data();
        r.vertex_mesh = r.f_vertex_mesh.data();
        r.mesh_lit = r.f_words.data();
        r.flags_created = r.f_words.data() + 2 * run;
        return YK_OK;
    }

    // The host instance of the rule (yk_scene_transform.h): the checks, then the points, normals and mesh flags rewrite_scene_host takes.
    yk_status transform_on_host() {
        RestOnHost r;
        yk_status rc = rest_on_host(r);
        if (rc != YK_OK) return rc;
        const uint32_t nm = s->n_meshes, run = std::max<uint32_t>(nm, 1u);
        const size_t nv = s->upd.n_vertices;
        const float* records = reinterpret_cast<const float*>(xf.h);
        std::vector<uint32_t> kinds(run, 0u);
        uint32_t flag = s->xf.shared ? (uint32_t)xfm::XF_BAD_SHARED : 0u;
        n_moved = n_flipped = 0;
        for (uint32_t m = 0; m < nm; ++m) {
            uint32_t bad;
            kinds[m] = xfm::mesh_kind(records + xfm::XF_RECORD_FLOATS * (size_t)m, r.mesh_lit[m] != 0u, &bad);
            flag |= bad;
            n_moved += (kinds[m] & xfm::XF_MOVED) ? 1u : 0u;
            n_flipped += (kinds[m] & xfm::XF_FLIPS) ? 1u : 0u;
        }
        xf_points.resize(3 * nv);
        for (size_t v = 0; v < nv; ++v) {
            const uint32_t mesh = r.vertex_mesh[2 * v];
            const V3 p = xfm::vertex_point(records, kinds.data(), nm, mesh, V3{r.points[3 * v], r.points[3 * v + 1], r.points[3 * v + 2]});
            if (xfm::vertex_moves(kinds.data(), nm, mesh) && xfm::point_not_finite(p)) flag |= xfm::XF_BAD_POINT;
            std::memcpy(&xf_points[3 * v], &p, 12);
        }
        if (flag) return fail(ctx, YK_ERR_INVALID_ARGUMENT, xfm::refusal(flag));
        if (r.normals) {
            xf_normals.resize(3 * nv);
            for (size_t v = 0; v < nv; ++v) {
                const V3 n = xfm::vertex_normal(records, kinds.data(), nm, r.vertex_mesh[2 * v], V3{r.normals[3 * v], r.normals[3 * v + 1], r.normals[3 * v + 2]});
                std::memcpy(&xf_normals[3 * v], &n, 12);
            }
        }
        xf_flags.assign(r.flags_created, r.flags_created + run);
        for (uint32_t m = 0; m < nm; ++m) xf_flags[m] = xfm::mesh_flags_of(xf_flags[m], kinds[m]);
        points.h = xf_points.data();
        normals.h = r.normals ? xf_normals.data() : nullptr;
        return YK_OK;
    }

    // check_and_stage of a transform: the plan, the rest pose, the records in HBM, the per-mesh kinds and the check pass with their flag word.
    yk_status check_and_stage_transform() {
        if (plan.refused) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "scene change: arguments no entry point accepts");
        const double t0 = now_seconds();
        yk_status rc = YK_OK;
        bool on_host = false;  // fall_back ran: the host instance has checked and computed
        const auto device_step = [&](uint32_t r) {
            if ((reason = r) == YK_LAYOUT_REASON_NONE) return true;
            on_host = true;
            rc = fall_back();
            return false;
        };
        const auto records_up = [&] {  // a host table on a device-laid scene goes up
            const hipError_t e = xf.to_device(tmp, s->n_meshes);
            return e == hipSuccess ? (uint32_t)YK_LAYOUT_REASON_NONE : layout_reason_of(e);
        };
        if (plan.device_route && device_step(plan_scene_update(ctx, s)) && device_step(snapshot_rest_device(ctx, s, true)) && (!plan.upload || device_step(records_up()))) {
            uint32_t flag = 0, counts[2] = {0u, 0u};
            if (device_step(stage_transforms_device(ctx, s, xf.d, &flag, counts))) {
                if (flag) return fail(ctx, YK_ERR_INVALID_ARGUMENT, xfm::refusal(flag));
                n_moved = counts[0];
                n_flipped = counts[1];
            }
        }
        if (!plan.device_route && !on_host) rc = transform_on_host();
        check = now_seconds() - t0;
        return rc;
    }

    // The tree's cost after the refit of a transform (yk_scene_transform.h): where the tree was refitted.
    yk_status cost_of_tree() {
        if (!plan.transform) return YK_OK;
        if (plan.device_route) {  // the refitted tree is in HBM and the host copy is stale until publish() says so: never read that one
            if (tree_cost_device(ctx, s, &tree_cost) == YK_LAYOUT_REASON_NONE) return YK_OK;
            (void)hipGetLastError();  // the reduction failed: the same nodes come down and the host sums them
            std::vector<uint32_t> nodes(8 * (size_t)s->info.n_nodes);
            if (!s->tree_nodes.p || s->tree_nodes.bytes < nodes.size() * 4) return fail(ctx, YK_ERR_DEVICE, "transforms: the refitted tree is not in device memory");
            HIP_TRY(ctx, hipMemcpy(nodes.data(), s->tree_nodes.p, nodes.size() * 4, hipMemcpyDeviceToHost));
            tree_cost = xfm::tree_cost(nodes.data(), (size_t)s->info.n_nodes);
            return YK_OK;
        }
        const HostBvh* bvh = scene_host_tree(s);
        if (!bvh) return fail(ctx, YK_ERR_DEVICE, "the scene's tree could not be copied back from the device");
        tree_cost = xfm::tree_cost(reinterpret_cast<const uint32_t*>(bvh->nodes.data()), bvh->nodes.size());
        return YK_OK;
    }

    // A device step failed with `reason`: the host route does the rest.  Arrays that were in device memory only come down, once, and get the host's checks.
    yk_status fall_back() {
        (void)hipGetLastError();
        plan = after_device_failure(plan);
        if (plan.transform) {
            HIP_TRY(ctx, xf.to_host(s->n_meshes));
            return transform_on_host();
        }
        const size_t n = 3 * (size_t)s->upd.n_vertices;
        const bool new_points = plan.points && !points.h, new_spheres = plan.spheres && !spheres.h;
        HIP_TRY(ctx, points.to_host(n));
        HIP_TRY(ctx, normals.to_host(n));
        HIP_TRY(ctx, spheres.to_host(s->n_spheres));
        if (new_points && !all_finite(points.h, n)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "points: coordinate not finite");
        const yk_scene_edit only_spheres = {spheres.h, nullptr, nullptr, nullptr};  // checked as a spheres-only edit
        return new_spheres ? check_edit_tables(ctx, s, &only_spheres) : YK_OK;
    }

    // All or nothing: the last checks before a byte of the scene is written — the device route's plan, stage and flag word (host tables: edit_scene).
    yk_status check_and_stage() {
        if (plan.refused) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "scene change: arguments no entry point accepts");
        yk_status rc = YK_OK;
        if (plan.device_plan && (reason = plan_scene_update(ctx, s)) != YK_LAYOUT_REASON_NONE) rc = fall_back();  // its time counts in seconds_total only
        if (plan.upload) {  // host arrays on a device-laid scene go up
            const size_t n = 3 * (size_t)s->upd.n_vertices;
            hipError_t err = plan.points ? points.to_device(tmp, n) : spheres.to_device(tmp, s->n_spheres);
            if (err == hipSuccess && normals.h) err = normals.to_device(tmp, n);
            reason = err == hipSuccess ? (uint32_t)YK_LAYOUT_REASON_NONE : plan.points ? (uint32_t)YK_LAYOUT_REASON_OUT_OF_MEMORY : layout_reason_of(err);  // (an update has always said so)
            if (err != hipSuccess) rc = fall_back();
        }
        const double t0 = plan.points ? now_seconds() : t_begin;  // an update: the finite test alone; an edit: the call so far
        if (plan.stage) {
            uint32_t flag = 0;
            reason = plan.points ? stage_points_device(ctx, s, points.d, &flag) : stage_spheres_device(ctx, s, spheres.d, tmp, &staged, &flag);
            if (reason != YK_LAYOUT_REASON_NONE)
                rc = fall_back();
            else if (flag)
                return fail(ctx, YK_ERR_INVALID_ARGUMENT, plan.points ? "points: coordinate not finite" : (flag & YK_SPHERES_MATERIAL) ? "sphere material out of range" : "spheres: matrix entry or radius not finite");
        }
        if (!plan.points || plan.stage) check = now_seconds() - t0;  // (an update on the host route: its entry point's own test)
        return rc;
    }

    // The sphere table by the host route: the device table, the bounds (host copy and the plan's) and the material column.
    yk_status write_spheres_host(std::vector<int32_t>& sphere_material) {
        yk_scene::UpdateState& u = s->upd;
        std::vector<DevSphere> table(s->n_spheres);
        for (size_t k = 0; k < table.size(); ++k) {
            table[k] = make_sphere(spheres.h[k]);
            sphere_material[k] = spheres.h[k].material;
            float b[6];
            inp::sphere_bound(spheres.h[k].object_to_world, spheres.h[k].radius, b);
            std::memcpy(&u.sphere_bounds[6 * k], b, sizeof(b));
        }
        if (!ctx) s->host.spheres = table;
        if (ctx && u.sphere_b.p) HIP_TRY(ctx, put_host_array(u.sphere_b, u.sphere_bounds.data(), u.sphere_bounds.size() * 4));
        return ctx ? upload(ctx, s->spheres, table.data(), table.size()) : YK_OK;
    }

    // The scene's own arrays and small tables take what the call brings; the device route commits what it staged.
    yk_status write_tables() {
        const size_t ns = s->n_spheres;
        const double t0 = now_seconds();
        yk_status rc;
        if (plan.lights) {
            std::vector<DevLight> lights(s->n_lights);
            for (uint32_t l = 0; l < s->n_lights; ++l) lights[l] = make_light(e->lights[l]);
            if (ctx && (rc = upload(ctx, s->lights, lights.data(), lights.size())) != YK_OK) return rc;
        }
        if (plan.materials) {
            if (ctx && (rc = upload(ctx, s->materials, mats.data(), mats.size())) != YK_OK) return rc;
            if (!ctx) s->host.materials = mats;
            s->upd.mat_kind = mat_kind;
        }
        std::vector<int32_t> sphere_material(ns);
        if (plan.points && !plan.transform && (rc = drop_rest(ctx, s)) != YK_OK) return rc;  // an update makes a new rest pose: the flags are creation's again
        if (plan.transform) {
            if (plan.stage && (reason = commit_transforms_device(ctx, s, xf.d)) != YK_LAYOUT_REASON_NONE && (rc = fall_back()) != YK_OK) return rc;
            if (!plan.stage) {  // the host route (also the one just fallen back to): the flags its records are laid out with
                if (ctx && (rc = upload(ctx, s->mesh_flags, xf_flags.data(), xf_flags.size())) != YK_OK) return rc;
                if (!ctx) s->host.mesh_flags = xf_flags;
            }
        } else if (plan.points && plan.stage) {
            if ((reason = commit_points_device(ctx, s, points.d, normals.d)) != YK_LAYOUT_REASON_NONE && (rc = fall_back()) != YK_OK) return rc;
        } else if (plan.spheres && plan.stage) {
            if ((reason = commit_spheres_device(ctx, s, staged, &sphere_material)) != YK_LAYOUT_REASON_NONE) return fail(ctx, YK_ERR_DEVICE, "the staged sphere table could not be copied into the scene");
        } else if (plan.spheres) {
            if ((rc = write_spheres_host(sphere_material)) != YK_OK) return rc;
        } else if (plan.kind_tables && ns) {  // the spheres' materials as the scene has them
            HostArrays have;
            if ((rc = scene_host_arrays(ctx, s, HOST_SPHERES, "", have)) != YK_OK) return rc;
            for (size_t k = 0; k < ns; ++k) sphere_material[k] = have->spheres[k].material;
        }
        if (plan.kind_tables && (rc = refresh_kind_tables(ctx, s, sphere_material)) != YK_OK) return rc;
        if (plan.background)
            for (int k = 0; k < 3; ++k) s->dev.background[k] = e->background[k];
        tables = now_seconds() - t0;
        return YK_OK;
    }

    // The host route: yk_bvh_refit on a copy of the host tree (no boxes planned: the tree stays), then — a scene in device memory —
    // layout_records_host and the uploads.  The points are the caller's, tested finite, or — an edit — the scene's own, which stay.
    yk_status rewrite_scene_host() {
        yk_scene::UpdateState& u = s->upd;
        const float *h_points = points.h, *h_normals = normals.h;
        const size_t nt = s->n_triangles, ns = s->n_spheres, nv = u.n_vertices;
        const HostBvh* old = scene_host_tree(s);
        if (!old) return fail(ctx, YK_ERR_DEVICE, "the scene's tree could not be copied back from the device");
        double t0 = now_seconds();
        HostArrays geo;
        yk_status rc = scene_host_arrays(ctx, s, HOST_INDICES | (h_points ? 0u : HOST_POINTS), "", geo);
        if (rc != YK_OK) return rc;
        if (!h_points) h_points = geo->points.data();
        std::shared_ptr<HostBvh> tree = std::make_shared<HostBvh>(*old);  // never through a tree that may be shared
        if (plan.boxes) {
            std::vector<float> sb(6 * (nt + ns));  // per source shape
            for (size_t i = 0; i < nt; ++i) {
                float b[6];
                (void)inp::tri_bound(h_points, geo->indices.data(), (uint32_t)i, b);
                std::memcpy(&sb[6 * i], b, sizeof(b));
            }
            std::copy(u.sphere_bounds.begin(), u.sphere_bounds.end(), sb.begin() + 6 * nt);
            if ((rc = yk_bvh_refit(tree->nodes.data(), tree->nodes.size(), tree->shape_order.data(), nt + ns, sb.data())) != YK_OK) return fail(ctx, rc, "the scene's tree does not fit its shapes");
            boxes = now_seconds() - t0;
        }
        t0 = now_seconds();
        if (ctx) {
            HostArrays rest;
            if ((rc = scene_host_arrays(ctx, s, (h_normals ? 0u : HOST_NORMALS) | HOST_UVS | HOST_TRI_MESH | HOST_MESH_FLAGS | HOST_TRI_MATERIAL | HOST_TRI_AREA_LIGHT | HOST_SPHERES, "", rest)) != YK_OK) return rc;
            std::vector<int32_t> sphere_material(ns);
            for (size_t k = 0; k < ns; ++k) sphere_material[k] = rest->spheres[k].material;
            HostLayoutInput in;
            in.bvh = tree.get();
            in.n_interior = s->info.n_interior;
            in.indices = geo->indices.data();
            in.points = h_points;
            in.normals = h_normals ? h_normals : (u.has_normals ? rest->normals.data() : nullptr);
            in.uvs = u.has_uvs ? rest->uvs.data() : nullptr;
            in.tri_material = rest->tri_material.data();
            in.tri_area_light = rest->tri_area_light.data();
            in.tri_mesh = rest->tri_mesh.data();
            in.mesh_flags = rest->mesh_flags.data();
            in.n_triangles = s->n_triangles;
            in.sphere_material = sphere_material.data();
            in.mat_kind = u.mat_kind.data();
            in.opt = u.opt;  // the records as creation laid them out, whatever the context's options say today
            if ((points.h && (rc = upload(ctx, s->points, points.h, 3 * nv)) != YK_OK) || (h_normals && (rc = upload(ctx, s->normals, h_normals, 3 * nv)) != YK_OK) ||
                (rc = upload_records(ctx, s, layout_records_host(in))) != YK_OK)
                return rc;
            if (s->tree_nodes.p && plan.boxes)  // the tree a later device-route change starts from
                HIP_TRY(ctx, hipMemcpy(s->tree_nodes.p, tree->nodes.data(), tree->nodes.size() * sizeof(yk_bvh_node), hipMemcpyHostToDevice));
        }
        std::memcpy(s->info.bounds_min, tree->nodes[0].bmin, sizeof(s->info.bounds_min));
        std::memcpy(s->info.bounds_max, tree->nodes[0].bmax, sizeof(s->info.bounds_max));
        std::lock_guard<std::mutex> lock(s->tree_mu);
        s->bvh = tree;
        s->bvh_lazy.reset();
        s->tree_fetched.store(1u);
        if (!ctx && points.h) s->host.points.assign(points.h, points.h + 3 * nv);  // what a later sphere edit folds the leaves from
        records = now_seconds() - t0;
        return YK_OK;
    }

    yk_status boxes_and_records() {
        if (!plan.boxes && !plan.records) return YK_OK;
        if (plan.device_route) {
            if ((reason = refit_scene_device(ctx, s, plan.boxes, &boxes, &records)) == YK_LAYOUT_REASON_NONE) return YK_OK;
            boxes = records = 0.0;
            const yk_status rc = fall_back();  // (what an edit committed is read from the scene)
            if (rc != YK_OK) return rc;
        }
        return rewrite_scene_host();
    }

    // The kernels' view of the rewritten records, the host tree's state and the info struct of the entry point.
    void publish() {
        yk_scene::UpdateState& u = s->upd;
        if (plan.device_route && plan.boxes) {  // the device refitted: the host copy of the tree is stale, the next reader fetches the refitted one
            std::lock_guard<std::mutex> lock(s->tree_mu);
            std::shared_ptr<HostBvh> fresh = std::make_shared<HostBvh>();
            fresh->max_leaf_shapes = s->bvh->max_leaf_shapes;
            fresh->depth = s->bvh->depth;
            fresh->split_failed = s->bvh->split_failed;
            s->bvh = s->bvh_lazy = fresh;
            s->tree_fetched.store(0u);
        }
        if (ctx && plan.records) bind_records(s);
        const uint32_t route = plan.device_route ? YK_UPDATE_ROUTE_DEVICE : YK_UPDATE_ROUTE_HOST, said = reported_reason(facts, reason);
        const double total = now_seconds() - t_begin;
        if (plan.transform) {
            yk_scene_transform_info& i = s->xf.info;  // rest_bytes and tree_cost_rest are the snapshot's
            i = yk_scene_transform_info{i.n_transforms + 1u, route, said, n_moved, n_flipped, 0u, i.rest_bytes, tree_cost, i.tree_cost_rest, check, tables, boxes, records, total};
        } else if (plan.points)  // seconds_check: the finite test, with the copy of the arrays into the scene; n_levels and plan_bytes are the plan's
            u.info = yk_scene_update_info{u.info.n_updates + 1u, route, said, u.info.n_levels, u.info.plan_bytes, check + tables, boxes, records, total};
        else
            u.edit_info = yk_scene_edit_info{u.edit_info.n_edits + 1u, route, said, plan.rewrote, check, tables, boxes, records, total};
    }
};

// ------------------------------------------------------------------ the entry points, host arrays and device arrays alike
yk_status update_scene(yk_context* ctx, yk_scene* s, const float* points, const float* normals, bool on_device, void* stream) {
    Change c(ctx);
    if (!s) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene");
    if (!points) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null points");
    if (normals && !s->upd.has_normals) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "normals given for a scene created without normals");
    yk_status rc = c.scene(s);
    if (rc != YK_OK) return rc;
    const size_t n = 3 * (size_t)s->upd.n_vertices;  // device arrays: the pointer checks of yk_scene_create_device, with its messages
    if (on_device && (rc = check_device_arrays(ctx, {{"points", points, 4 * n}, {"normals", normals, 4 * n}})) != YK_OK) return rc;
    if (!on_device && !all_finite(points, n)) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "points: coordinate not finite");
    c.check = now_seconds() - c.t_begin;
    if ((rc = c.wait(stream)) != YK_OK) return rc;
    (on_device ? c.points.d : c.points.h) = points;
    (on_device ? c.normals.d : c.normals.h) = normals;
    (on_device ? c.facts.points_device : c.facts.points_host) = true;
    c.facts.normals = normals != nullptr;
    return c.run();
}

yk_status transform_scene(yk_context* ctx, yk_scene* s, const void* transforms, bool on_device, void* stream) {
    Change c(ctx);
    if (!s) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene");
    if (!transforms) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null transforms");
    yk_status rc = c.scene(s);
    if (rc != YK_OK) return rc;
    if (on_device && s->n_meshes) {  // the pointer checks of yk_scene_create_device, with its messages
        if ((rc = check_device_arrays(ctx, {{"transforms", transforms, sizeof(yk_mesh_transform) * (size_t)s->n_meshes}})) != YK_OK) return rc;
        if (reinterpret_cast<uintptr_t>(transforms) & 3u) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "transforms must be 4-byte aligned");
    }
    if ((rc = c.wait(stream)) != YK_OK) return rc;
    (on_device ? c.xf.d : c.xf.h) = static_cast<const yk_mesh_transform*>(transforms);
    (on_device ? c.facts.transforms_device : c.facts.transforms_host) = true;
    return c.run();
}

yk_status edit_scene(yk_context* ctx, yk_scene* s, const yk_scene_edit* e, const void* d_spheres, void* stream) {
    Change c(ctx);
    if (!s) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null scene");
    if (!e) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "null edit");
    if (e->spheres && d_spheres) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "spheres given as a host table and as a device table");
    yk_status rc = c.scene(s);
    if (rc != YK_OK) return rc;
    if (d_spheres && s->n_spheres) {  // the pointer checks of yk_scene_create_device, with its messages
        if ((rc = check_device_arrays(ctx, {{"spheres", d_spheres, sizeof(yk_sphere_desc) * (size_t)s->n_spheres}})) != YK_OK) return rc;
        if (reinterpret_cast<uintptr_t>(d_spheres) & 3u) return fail(ctx, YK_ERR_INVALID_ARGUMENT, "spheres must be 4-byte aligned");
    }
    if ((rc = c.wait(stream)) != YK_OK || (rc = check_edit_tables(ctx, s, e)) != YK_OK) return rc;
    c.e = e;
    c.spheres.h = e->spheres;
    c.spheres.d = static_cast<const yk_sphere_desc*>(d_spheres);
    for (uint32_t m = 0; e->materials && m < s->n_materials; ++m) {
        c.mats.push_back(make_material(e->materials[m]));
        c.mat_kind.push_back((uint8_t)(c.mats[m].kind & 7u));
    }
    c.facts.spheres_host = e->spheres != nullptr;
    c.facts.spheres_device = d_spheres != nullptr;
    c.facts.lights = e->lights != nullptr;
    c.facts.materials = e->materials != nullptr;
    c.facts.background = e->background != nullptr;
    c.facts.kinds_changed = !c.mats.empty() && c.mat_kind != s->upd.mat_kind;
    return c.run();
}

}  // namespace

extern "C" {

yk_status yk_scene_update(yk_context* ctx, yk_scene* s, const float* points, const float* normals) try {
    return update_scene(ctx, s, points, normals, false, nullptr);
} YK_CATCH(ctx)

yk_status yk_scene_update_device(yk_context* ctx, yk_scene* s, const float* d_points, const float* d_normals, void* stream) try {
    return ctx ? update_scene(ctx, s, d_points, d_normals, true, stream) : YK_ERR_INVALID_ARGUMENT;
} YK_CATCH(ctx)

yk_status yk_scene_transform(yk_context* ctx, yk_scene* s, const yk_mesh_transform* transforms) try {
    return transform_scene(ctx, s, transforms, false, nullptr);
} YK_CATCH(ctx)

yk_status yk_scene_transform_device(yk_context* ctx, yk_scene* s, const void* d_transforms, void* stream) try {
    return ctx ? transform_scene(ctx, s, d_transforms, true, stream) : YK_ERR_INVALID_ARGUMENT;
} YK_CATCH(ctx)

yk_status yk_scene_apply_edit(yk_context* ctx, yk_scene* s, const yk_scene_edit* edit) try {
    return edit_scene(ctx, s, edit, nullptr, nullptr);
} YK_CATCH(ctx)

yk_status yk_scene_apply_edit_device(yk_context* ctx, yk_scene* s, const yk_scene_edit* edit, const void* d_spheres, void* stream) try {
    if (!ctx) return fail(nullptr, YK_ERR_INVALID_ARGUMENT, edit && edit->spheres && d_spheres ? "spheres given as a host table and as a device table" : "a sphere table in device memory needs a context");
    return edit_scene(ctx, s, edit, d_spheres, stream);
} YK_CATCH(ctx)

}  // extern "C"
