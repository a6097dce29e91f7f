// yk_scene_change.h — what yk_scene_update[_device], yk_scene_apply_edit[_device] and yk_scene_transform[_device] decide before
// they write anything, as pure functions over plain values.  The specification is the comment of yk_scene_apply_edit in
// include/yuki_hip.h ("What is rewritten follows from what changed"), and for a transform that of yk_scene_transform;
// yk_scene_change.cpp runs the plan.  No HIP here: tests/cpp/scene_change_plan_test.cpp and scene_transform_plan_test.cpp
// compile this header alone.  Library-private.
#pragma once
#include <cstdint>

#include "../../include/yuki_hip.h"

namespace yk_change {

// What the caller knows before anything of the scene is written.
struct ChangeFacts {
    bool has_context = false, device_laid = false;  // no context: a host-only scene; device_laid: its layout is YK_LAYOUT_DEVICE
    uint32_t n_spheres = 0, n_lights = 0, n_materials = 0;
    bool points_host = false, points_device = false, normals = false;  // what the call brings: an update ...
    bool spheres_host = false, spheres_device = false, lights = false, materials = false, background = false;  // ... or an edit
    bool kinds_changed = false;  // the new material table's device BSDF kinds differ from the scene's
    bool transforms_host = false, transforms_device = false;  // ... or a transform: one matrix pair a mesh (yk_scene_transform[_device])
};

struct ChangePlan {
    bool refused = false;       // no entry point lets these facts through (a device array without a context, an update with an edit)
    bool device_route = false;  // the route asked for (after_device_failure: the route taken)
    bool device_plan = false;   // plan_scene_update is needed: the device route rewrites records
    bool stage = false, upload = false;  // points or spheres are tested, staged and committed on the device; a host array goes up for it
    bool points = false, spheres = false, lights = false, materials = false, background = false;  // what is rewritten of the scene's own
    bool kind_tables = false;   // the scene's tables of its shapes' BSDF kinds are refreshed
    bool boxes = false, records = false;  // the tree is refitted; the seven record buffers are rewritten
    uint32_t rewrote = 0;       // YK_EDIT_* for the edit info
    bool transform = false;     // the points (and normals) are made of the rest pose by the call's matrices: it plans like an update of points ...
    bool mesh_flags = false;    // ... plus the table of mesh flags, which a mirroring matrix flips
};

// the scene's layout decides, and arrays that are in device memory already stay there
inline bool asks_device_route(const ChangeFacts& f) { return f.has_context && (f.device_laid || f.points_device || f.transforms_device || (f.spheres_device && f.n_spheres != 0)); }

inline ChangePlan plan_change(const ChangeFacts& f) {
    ChangePlan p;
    const bool update = f.points_host || f.points_device;
    const bool edit = f.spheres_host || f.spheres_device || f.lights || f.materials || f.background || f.kinds_changed;
    const bool transform = f.transforms_host || f.transforms_device;  // alone in its call: with an update or an edit it is refused
    p.refused = ((f.points_device || f.spheres_device || f.transforms_device || f.device_laid) && !f.has_context) || (f.points_host && f.points_device) || (f.spheres_host && f.spheres_device) ||
                (f.transforms_host && f.transforms_device) || (update && edit) || (transform && (update || edit)) || (f.normals && !update) || (f.kinds_changed && !f.materials);
    if (p.refused) return p;
    p.points = update || transform;
    p.transform = p.mesh_flags = transform;
    p.spheres = (f.spheres_host || f.spheres_device) && f.n_spheres != 0;
    p.lights = f.lights && f.n_lights != 0;
    p.materials = f.materials && f.n_materials != 0;
    p.background = f.background;
    const bool kinds = p.materials && f.kinds_changed;
    p.kind_tables = p.spheres || kinds;
    p.boxes = p.points || p.spheres;
    p.records = f.has_context && (p.boxes || kinds);  // a host-only scene has none: its tree alone is refitted
    p.device_route = asks_device_route(f);
    p.device_plan = p.device_route && p.records;
    p.stage = p.device_route && p.boxes;
    p.upload = p.stage && (f.points_host || f.spheres_host || f.transforms_host);
    p.rewrote = (p.lights ? YK_EDIT_LIGHTS : 0u) | (p.materials ? YK_EDIT_MATERIALS : 0u) | (p.spheres ? YK_EDIT_SPHERES : 0u) | (p.boxes ? YK_EDIT_BOXES : 0u) |
                (p.records ? YK_EDIT_RECORDS : 0u) | (p.background ? YK_EDIT_BACKGROUND : 0u);
    return p;
}

// The plan that follows a device step that failed, before staging or after the commit: the same rewrites by the host route.
inline ChangePlan after_device_failure(ChangePlan p) {
    p.device_route = p.device_plan = p.stage = p.upload = false;
    return p;
}

// A call that asked for the host route reports no reason, whatever happened on the way.
inline uint32_t reported_reason(const ChangeFacts& f, uint32_t reason) { return asks_device_route(f) ? reason : (uint32_t)YK_LAYOUT_REASON_NONE; }

}  // namespace yk_change
