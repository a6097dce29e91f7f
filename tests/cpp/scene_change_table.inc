// What a change of a live scene decides, row by row: written by hand from the comment of yk_scene_apply_edit and
// yk_scene_update in include/yuki_hip.h ("What is rewritten follows from what changed", "It follows the scene's layout")
// and from the code those comments were written for — never from yuki_amd/csrc/yk_scene_change.h, which is checked
// against it (tests/cpp/scene_change_plan_test.cpp; tests/test_scene_edit.py and tests/test_gpu_scene_edit.py read the
// same rows and hold the library to them).
//
// ROW(scene, brings, has_spheres, kinds_changed,   verdict, device_plan, upload,   spheres, kind_tables, boxes, records)
//   scene          HOST_ONLY (no context) | HOST_LAID | DEVICE_LAID (a context; who laid the records out)
//   brings         NONE | SPHERES_HOST | SPHERES_DEVICE (an edit's sphere table) | POINTS_HOST | POINTS_DEVICE (an update)
//   has_spheres    the scene was created with spheres
//   kinds_changed  the edit brings materials whose device BSDF kinds differ from the scene's
//   verdict        REFUSED by the entry point, or the route the call asks for: HOST | DEVICE
//   device_plan    the plan of the device route (tree, levels and small tables in HBM) is needed
//   upload         a host array goes up to be tested and staged on the device
//   spheres        the sphere table and the spheres' bounds are rewritten
//   kind_tables    the scene's tables of its shapes' BSDF kinds are refreshed
//   boxes, records the tree is refitted; the seven record buffers are rewritten
// Lights, materials and the background are independent of all this: each given table is rewritten (lights and materials
// where the scene has any) and sets its YK_EDIT_* bit; `spheres`, `boxes` and `records` set theirs.  After a device step
// fails the verdict is HOST, device_plan and upload are 0 and the rest of the row stands.

// ---- a host-only scene: the host route, and no records to rewrite
ROW(HOST_ONLY, NONE, 0, 0,             HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, NONE, 0, 1,             HOST, 0, 0,   0, 1, 0, 0)
ROW(HOST_ONLY, NONE, 1, 0,             HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, NONE, 1, 1,             HOST, 0, 0,   0, 1, 0, 0)
ROW(HOST_ONLY, SPHERES_HOST, 0, 0,     HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, SPHERES_HOST, 0, 1,     HOST, 0, 0,   0, 1, 0, 0)
ROW(HOST_ONLY, SPHERES_HOST, 1, 0,     HOST, 0, 0,   1, 1, 1, 0)
ROW(HOST_ONLY, SPHERES_HOST, 1, 1,     HOST, 0, 0,   1, 1, 1, 0)
ROW(HOST_ONLY, SPHERES_DEVICE, 0, 0,   REFUSED, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, SPHERES_DEVICE, 0, 1,   REFUSED, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, SPHERES_DEVICE, 1, 0,   REFUSED, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, SPHERES_DEVICE, 1, 1,   REFUSED, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, POINTS_HOST, 0, 0,      HOST, 0, 0,   0, 0, 1, 0)
ROW(HOST_ONLY, POINTS_HOST, 1, 0,      HOST, 0, 0,   0, 0, 1, 0)
ROW(HOST_ONLY, POINTS_DEVICE, 0, 0,    REFUSED, 0, 0,   0, 0, 0, 0)
ROW(HOST_ONLY, POINTS_DEVICE, 1, 0,    REFUSED, 0, 0,   0, 0, 0, 0)

// ---- a host-laid scene: the host route, unless the arrays are in device memory already
ROW(HOST_LAID, NONE, 0, 0,             HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_LAID, NONE, 0, 1,             HOST, 0, 0,   0, 1, 0, 1)
ROW(HOST_LAID, NONE, 1, 0,             HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_LAID, NONE, 1, 1,             HOST, 0, 0,   0, 1, 0, 1)
ROW(HOST_LAID, SPHERES_HOST, 0, 0,     HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_LAID, SPHERES_HOST, 0, 1,     HOST, 0, 0,   0, 1, 0, 1)
ROW(HOST_LAID, SPHERES_HOST, 1, 0,     HOST, 0, 0,   1, 1, 1, 1)
ROW(HOST_LAID, SPHERES_HOST, 1, 1,     HOST, 0, 0,   1, 1, 1, 1)
ROW(HOST_LAID, SPHERES_DEVICE, 0, 0,   HOST, 0, 0,   0, 0, 0, 0)
ROW(HOST_LAID, SPHERES_DEVICE, 0, 1,   HOST, 0, 0,   0, 1, 0, 1)
ROW(HOST_LAID, SPHERES_DEVICE, 1, 0,   DEVICE, 1, 0,   1, 1, 1, 1)
ROW(HOST_LAID, SPHERES_DEVICE, 1, 1,   DEVICE, 1, 0,   1, 1, 1, 1)
ROW(HOST_LAID, POINTS_HOST, 0, 0,      HOST, 0, 0,   0, 0, 1, 1)
ROW(HOST_LAID, POINTS_HOST, 1, 0,      HOST, 0, 0,   0, 0, 1, 1)
ROW(HOST_LAID, POINTS_DEVICE, 0, 0,    DEVICE, 1, 0,   0, 0, 1, 1)
ROW(HOST_LAID, POINTS_DEVICE, 1, 0,    DEVICE, 1, 0,   0, 0, 1, 1)

// ---- a device-laid scene: the device route; it needs its plan only where records are rewritten
ROW(DEVICE_LAID, NONE, 0, 0,           DEVICE, 0, 0,   0, 0, 0, 0)
ROW(DEVICE_LAID, NONE, 0, 1,           DEVICE, 1, 0,   0, 1, 0, 1)
ROW(DEVICE_LAID, NONE, 1, 0,           DEVICE, 0, 0,   0, 0, 0, 0)
ROW(DEVICE_LAID, NONE, 1, 1,           DEVICE, 1, 0,   0, 1, 0, 1)
ROW(DEVICE_LAID, SPHERES_HOST, 0, 0,   DEVICE, 0, 0,   0, 0, 0, 0)
ROW(DEVICE_LAID, SPHERES_HOST, 0, 1,   DEVICE, 1, 0,   0, 1, 0, 1)
ROW(DEVICE_LAID, SPHERES_HOST, 1, 0,   DEVICE, 1, 1,   1, 1, 1, 1)
ROW(DEVICE_LAID, SPHERES_HOST, 1, 1,   DEVICE, 1, 1,   1, 1, 1, 1)
ROW(DEVICE_LAID, SPHERES_DEVICE, 0, 0, DEVICE, 0, 0,   0, 0, 0, 0)
ROW(DEVICE_LAID, SPHERES_DEVICE, 0, 1, DEVICE, 1, 0,   0, 1, 0, 1)
ROW(DEVICE_LAID, SPHERES_DEVICE, 1, 0, DEVICE, 1, 0,   1, 1, 1, 1)
ROW(DEVICE_LAID, SPHERES_DEVICE, 1, 1, DEVICE, 1, 0,   1, 1, 1, 1)
ROW(DEVICE_LAID, POINTS_HOST, 0, 0,    DEVICE, 1, 1,   0, 0, 1, 1)
ROW(DEVICE_LAID, POINTS_HOST, 1, 0,    DEVICE, 1, 1,   0, 0, 1, 1)
ROW(DEVICE_LAID, POINTS_DEVICE, 0, 0,  DEVICE, 1, 0,   0, 0, 1, 1)
ROW(DEVICE_LAID, POINTS_DEVICE, 1, 0,  DEVICE, 1, 0,   0, 0, 1, 1)
