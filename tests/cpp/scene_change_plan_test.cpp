// scene_change_plan_test.cpp — the decisions of a scene change (yuki_amd/csrc/yk_scene_change.h) against the table written
// by hand in scene_change_table.inc: every combination of scene kind, sphere table, sphere count, lights, materials and
// background for an edit, the update rows, what follows a device step that failed, the reported reason, and the combinations
// no entry point lets through.  Plain host C++: the header includes no HIP.  Built and run by tests/test_scene_change_plan.py.
#include <cstdio>
#include <initializer_list>

#include "../../yuki_amd/csrc/yk_scene_change.h"

using namespace yk_change;

static int failures = 0, checked = 0;
#define CHECK(cond)                                                                               \
    do {                                                                                          \
        ++checked;                                                                                \
        if (!(cond)) {                                                                            \
            std::printf("%s:%d: CHECK(%s) failed for %s\n", __FILE__, __LINE__, #cond, what);     \
            ++failures;                                                                           \
        }                                                                                         \
    } while (0)

enum Scene { HOST_ONLY, HOST_LAID, DEVICE_LAID };
enum Brings { NONE, SPHERES_HOST, SPHERES_DEVICE, POINTS_HOST, POINTS_DEVICE };
enum Verdict { REFUSED, HOST, DEVICE };
struct Row {
    Scene scene;
    Brings brings;
    int has_spheres, kinds_changed;
    Verdict verdict;
    int device_plan, upload, spheres, kind_tables, boxes, records;
};
#define ROW(scene, brings, has_spheres, kinds_changed, verdict, device_plan, upload, spheres, kind_tables, boxes, records) \
    {scene, brings, has_spheres, kinds_changed, verdict, device_plan, upload, spheres, kind_tables, boxes, records},
static const Row TABLE[] = {
#include "scene_change_table.inc"
};
static const int N_ROWS = (int)(sizeof(TABLE) / sizeof(TABLE[0]));

static const Row* row_of(Scene scene, Brings brings, bool has_spheres, bool kinds_changed) {
    const Row* found = nullptr;
    for (int i = 0; i < N_ROWS; ++i)
        if (TABLE[i].scene == scene && TABLE[i].brings == brings && (TABLE[i].has_spheres != 0) == has_spheres && (TABLE[i].kinds_changed != 0) == kinds_changed) {
            if (found) return nullptr;  // a key twice
            found = &TABLE[i];
        }
    return found;
}

static ChangeFacts facts_of(Scene scene, Brings brings, bool has_spheres) {
    ChangeFacts f;
    f.has_context = scene != HOST_ONLY;
    f.device_laid = scene == DEVICE_LAID;
    f.n_spheres = has_spheres ? 3u : 0u;
    f.n_lights = 2u;
    f.n_materials = 5u;
    f.spheres_host = brings == SPHERES_HOST;
    f.spheres_device = brings == SPHERES_DEVICE;
    f.points_host = brings == POINTS_HOST;
    f.points_device = brings == POINTS_DEVICE;
    return f;
}

// one combination of facts against its row; `lights`, `materials`, `background`: the tables beside it
static void check_case(const ChangeFacts& f, const Row* r, bool lights, bool materials, bool background, const char* what) {
    CHECK(r != nullptr);
    if (!r) return;
    const ChangePlan p = plan_change(f);
    CHECK(p.refused == (r->verdict == REFUSED));
    if (r->verdict == REFUSED) return;
    const bool device = r->verdict == DEVICE, update = r->brings == POINTS_HOST || r->brings == POINTS_DEVICE;
    const uint32_t rewrote = (lights ? YK_EDIT_LIGHTS : 0u) | (materials ? YK_EDIT_MATERIALS : 0u) | (background ? YK_EDIT_BACKGROUND : 0u) | (r->spheres ? YK_EDIT_SPHERES : 0u) |
                             (r->boxes ? YK_EDIT_BOXES : 0u) | (r->records ? YK_EDIT_RECORDS : 0u);
    CHECK(p.device_route == device);
    CHECK(p.device_plan == (r->device_plan != 0));
    CHECK(p.upload == (r->upload != 0));
    CHECK(p.stage == (device && r->boxes));  // what moves boxes is tested and staged where the route runs
    CHECK(p.points == update);
    CHECK(p.spheres == (r->spheres != 0));
    CHECK(p.lights == lights && p.materials == materials && p.background == background);
    CHECK(p.kind_tables == (r->kind_tables != 0));
    CHECK(p.boxes == (r->boxes != 0));
    CHECK(p.records == (r->records != 0));
    CHECK(p.rewrote == rewrote);
    const ChangePlan q = after_device_failure(p);  // the same rewrites by the host route
    CHECK(!q.refused && !q.device_route && !q.device_plan && !q.upload && !q.stage);
    CHECK(q.points == p.points && q.spheres == p.spheres && q.lights == p.lights && q.materials == p.materials && q.background == p.background);
    CHECK(q.kind_tables == p.kind_tables && q.boxes == p.boxes && q.records == p.records && q.rewrote == rewrote);
    for (uint32_t reason : {(uint32_t)YK_LAYOUT_REASON_NONE, (uint32_t)YK_LAYOUT_REASON_OUT_OF_MEMORY, (uint32_t)YK_LAYOUT_REASON_DEVICE_ERROR})
        CHECK(reported_reason(f, reason) == (device ? reason : (uint32_t)YK_LAYOUT_REASON_NONE));  // a call that asked for the host route reports none
}

static void edits() {
    for (Scene scene : {HOST_ONLY, HOST_LAID, DEVICE_LAID})
        for (Brings brings : {NONE, SPHERES_HOST, SPHERES_DEVICE})
            for (int has_spheres = 0; has_spheres < 2; ++has_spheres)
                for (int lights = 0; lights < 2; ++lights)
                    for (int materials = 0; materials < 3; ++materials)  // none, the same kinds, changed kinds
                        for (int background = 0; background < 2; ++background) {
                            ChangeFacts f = facts_of(scene, brings, has_spheres != 0);
                            f.lights = lights != 0;
                            f.materials = materials != 0;
                            f.kinds_changed = materials == 2;
                            f.background = background != 0;
                            char what[96];
                            std::snprintf(what, sizeof(what), "edit: scene %d, brings %d, spheres %d, lights %d, materials %d, background %d", scene, brings, has_spheres, lights, materials, background);
                            check_case(f, row_of(scene, brings, has_spheres != 0, materials == 2), lights != 0, materials != 0, background != 0, what);
                        }
    // tables of a scene that has none of the kind are not rewritten
    const char* what = "edit: no lights, no materials";
    ChangeFacts f = facts_of(DEVICE_LAID, NONE, true);
    f.lights = f.materials = f.kinds_changed = true;
    f.n_lights = f.n_materials = 0;
    const ChangePlan p = plan_change(f);
    CHECK(!p.refused && !p.lights && !p.materials && !p.kind_tables && !p.records && p.rewrote == 0u && p.device_route && !p.device_plan);
}

static void updates() {
    for (Scene scene : {HOST_ONLY, HOST_LAID, DEVICE_LAID})
        for (Brings brings : {POINTS_HOST, POINTS_DEVICE})
            for (int has_spheres = 0; has_spheres < 2; ++has_spheres)
                for (int normals = 0; normals < 2; ++normals) {
                    ChangeFacts f = facts_of(scene, brings, has_spheres != 0);
                    f.normals = normals != 0;
                    char what[96];
                    std::snprintf(what, sizeof(what), "update: scene %d, brings %d, spheres %d, normals %d", scene, brings, has_spheres, normals);
                    check_case(f, row_of(scene, brings, has_spheres != 0, false), false, false, false, what);
                }
}

// what no entry point lets through, beside the table's REFUSED rows
static void refusals() {
    const char* what = "refusals";
    ChangeFacts f = facts_of(DEVICE_LAID, SPHERES_HOST, true);
    f.spheres_device = true;  // "spheres given as a host table and as a device table"
    CHECK(plan_change(f).refused);
    f = facts_of(DEVICE_LAID, POINTS_HOST, true);
    f.points_device = true;
    CHECK(plan_change(f).refused);
    f = facts_of(DEVICE_LAID, POINTS_DEVICE, true);
    f.lights = true;  // an update and an edit in one call: two calls back to back (include/yuki_hip.h)
    CHECK(plan_change(f).refused);
    f = facts_of(HOST_LAID, SPHERES_HOST, true);
    f.normals = true;  // normals belong to an update
    CHECK(plan_change(f).refused);
    f = facts_of(HOST_ONLY, NONE, true);
    f.device_laid = true;  // a layout on a device the scene is not on
    CHECK(plan_change(f).refused);
    f = facts_of(HOST_LAID, NONE, true);
    f.kinds_changed = true;  // without a material table
    CHECK(plan_change(f).refused);
}

int main() {
    const char* what = "the table";
    CHECK(N_ROWS == 48);  // 3 scenes x (3 sphere tables x 2 x 2 + 2 updates x 2)
    edits();
    updates();
    refusals();
    if (failures) {
        std::printf("scene_change_plan_test: %d of %d checks failed\n", failures, checked);
        return 1;
    }
    std::printf("scene_change_plan_test: ok (%d checks over %d rows)\n", checked, N_ROWS);
    return 0;
}
