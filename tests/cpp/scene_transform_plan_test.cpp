// scene_transform_plan_test.cpp — the transform facts of a scene change (yuki_amd/csrc/yk_scene_change.h): a transform plans
// like an update of points plus the table of mesh flags; the route follows the scene's layout for a host table and is the
// device's for a table in device memory; a transform combined with an update or an edit, given twice, or in device memory
// without a context is refused; and facts without a transform plan what they planned before (the defaults are false).
// Plain host C++: the header includes no HIP.  Built and run by tests/test_scene_transform.py.
#include <cstdio>
#include <initializer_list>

#include "../../yuki_amd/csrc/yk_scene_change.h"

using namespace yk_change;

static int failures = 0, checked = 0;
#define CHECK(cond)                                                                           \
    do {                                                                                      \
        ++checked;                                                                            \
        if (!(cond)) {                                                                        \
            std::printf("%s:%d: CHECK(%s) failed for %s\n", __FILE__, __LINE__, #cond, what); \
            ++failures;                                                                       \
        }                                                                                     \
    } while (0)

enum Scene { HOST_ONLY, HOST_LAID, DEVICE_LAID };

static ChangeFacts facts_of(Scene scene, bool spheres) {
    ChangeFacts f;
    f.has_context = scene != HOST_ONLY;
    f.device_laid = scene == DEVICE_LAID;
    f.n_spheres = spheres ? 3u : 0u;
    f.n_lights = 2u;
    f.n_materials = 5u;
    return f;
}

static bool same_plan(const ChangePlan& a, const ChangePlan& b) {
    return a.refused == b.refused && a.device_route == b.device_route && a.device_plan == b.device_plan && a.stage == b.stage && a.upload == b.upload && a.points == b.points &&
           a.spheres == b.spheres && a.lights == b.lights && a.materials == b.materials && a.background == b.background && a.kind_tables == b.kind_tables && a.boxes == b.boxes &&
           a.records == b.records && a.rewrote == b.rewrote;
}

int main() {
    char what[96];
    for (Scene scene : {HOST_ONLY, HOST_LAID, DEVICE_LAID})
        for (int device_table = 0; device_table < 2; ++device_table)
            for (int spheres = 0; spheres < 2; ++spheres) {
                std::snprintf(what, sizeof(what), "transform: scene %d, device table %d, spheres %d", scene, device_table, spheres);
                ChangeFacts f = facts_of(scene, spheres != 0);
                (device_table ? f.transforms_device : f.transforms_host) = true;
                const ChangePlan p = plan_change(f);
                if (scene == HOST_ONLY && device_table) {  // a table in device memory needs a context
                    CHECK(p.refused);
                    continue;
                }
                const bool device = scene == DEVICE_LAID || device_table;
                CHECK(!p.refused && p.transform && p.mesh_flags);
                CHECK(asks_device_route(f) == device && p.device_route == device);
                // like an update that brings its points the same way ...
                ChangeFacts u = facts_of(scene, spheres != 0);
                (device_table ? u.points_device : u.points_host) = true;
                const ChangePlan q = plan_change(u);
                CHECK(same_plan(p, q) && !q.transform && !q.mesh_flags);
                CHECK(p.points && p.boxes && !p.spheres && !p.lights && !p.materials && !p.background && !p.kind_tables);
                CHECK(p.records == (scene != HOST_ONLY));  // a host-only scene has none: its tree alone is refitted
                CHECK(p.device_plan == device && p.stage == device && p.upload == (device && !device_table));
                CHECK(p.rewrote == (uint32_t)(YK_EDIT_BOXES | (p.records ? YK_EDIT_RECORDS : 0)));
                // ... and the same rewrites by the host route after a device step that failed
                const ChangePlan h = after_device_failure(p);
                CHECK(h.transform && h.mesh_flags && h.points && h.boxes && h.records == p.records && !h.device_route && !h.device_plan && !h.stage && !h.upload);
                for (uint32_t reason : {(uint32_t)YK_LAYOUT_REASON_NONE, (uint32_t)YK_LAYOUT_REASON_OUT_OF_MEMORY, (uint32_t)YK_LAYOUT_REASON_DEVICE_ERROR})
                    CHECK(reported_reason(f, reason) == (device ? reason : (uint32_t)YK_LAYOUT_REASON_NONE));
            }
    {
        std::snprintf(what, sizeof(what), "refusals");
        ChangeFacts f = facts_of(DEVICE_LAID, true);
        f.transforms_host = f.transforms_device = true;  // given twice
        CHECK(plan_change(f).refused);
        for (int with = 0; with < 8; ++with) {  // with an update or an edit: separate calls
            f = facts_of(DEVICE_LAID, true);
            f.transforms_host = true;
            f.points_host = with == 0;
            f.points_device = with == 1;
            f.spheres_host = with == 2;
            f.spheres_device = with == 3;
            f.lights = with == 4;
            f.materials = with == 5;
            f.background = with == 6;
            f.normals = with == 7;  // normals belong to an update
            CHECK(plan_change(f).refused);
        }
    }
    {
        std::snprintf(what, sizeof(what), "defaults");
        const ChangePlan none = plan_change(facts_of(DEVICE_LAID, true));
        CHECK(!none.refused && !none.transform && !none.mesh_flags && !none.points && !none.boxes && !none.records);
        ChangeFacts f = facts_of(HOST_LAID, true);
        f.points_host = true;
        CHECK(!plan_change(f).transform && !plan_change(f).mesh_flags && !asks_device_route(f));
    }
    if (failures) {
        std::printf("scene_transform_plan_test: %d of %d checks failed\n", failures, checked);
        return 1;
    }
    std::printf("scene_transform_plan_test: ok (%d checks)\n", checked);
    return 0;
}
