//! `yuki/src/app/gpu_worker.rs` — show a moved mesh without building its scene again.  The reference has no animation:
//! a changed mesh means a new `Scene` and a new BVH.  With `yk_scene_update[_device]` the worker keeps the `yk_scene` it
//! made for the first frame and hands every later frame's vertex positions to it: the tree keeps its topology, its
//! boxes are refitted bottom-up and the traversal records are rewritten, all on the device when the positions are
//! there already (a skinning or simulation kernel's output).  What the caller must keep in mind:
//!   * indices and uvs stay; positions (and, optionally, normals) move through `update_scene`, spheres, lights,
//!     materials and the background change through `edit_scene` (yk_scene_apply_edit): counts and light kinds stay;
//!   * a rectangular light and its two triangles move together only when the caller moves both: `update_scene` with
//!     the moved vertices and `edit_scene` with the moved light record, nothing rendered in between;
//!   * every coordinate must be finite, or the call is refused and the scene stays as it was;
//!   * the call waits for what this context has enqueued; renders from other contexts must not be in flight;
//!   * a refit never improves the tree: after a large deformation traversal is slower than through a rebuilt tree
//!     (profiles/scene_update_device.json has both), so a worker may rebuild every so often.
//! A mesh that moves by a matrix needs none of this bookkeeping: `transform.rs` (yk_scene_transform) takes the matrix.
//! The rule: yuki_amd/csrc/yk_scene_update.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use std::ffi::c_void;
use yuki_hip_sys as sys;

/// Host positions (3 floats a vertex, the scene's own vertex count) and optional normals of the same size.
pub fn update_scene(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, points: &[f32], normals: Option<&[f32]>) -> Result<sys::yk_scene_update_info, String> {
    if let Some(n) = normals {
        assert!(n.len() == points.len());
    }
    let status = unsafe { sys::yk_scene_update(ctx, scene, points.as_ptr(), normals.map_or(std::ptr::null(), |n| n.as_ptr())) };
    finish(ctx, scene, status)
}

/// Device positions produced on `stream` (a hipStream_t, or null): nothing crosses the host link.
pub fn update_scene_device(
    ctx: *mut sys::yk_context,
    scene: *mut sys::yk_scene,
    d_points: *const f32,
    d_normals: *const f32,
    stream: *mut c_void,
) -> Result<sys::yk_scene_update_info, String> {
    let status = unsafe { sys::yk_scene_update_device(ctx, scene, d_points, d_normals, stream) };
    finish(ctx, scene, status)
}

fn finish(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, status: sys::yk_status) -> Result<sys::yk_scene_update_info, String> {
    if status != sys::YK_OK {
        return Err(sys::last_error(ctx));
    }
    let mut info = sys::yk_scene_update_info::default();
    unsafe { sys::yk_scene_get_update_info(scene, &mut info) };
    if info.route == sys::YK_UPDATE_ROUTE_HOST && info.reason != 0 {
        log::warn!("scene update fell back to the host route (reason {})", info.reason);
    }
    Ok(info)
}

/// Spheres, lights, materials and the background in place; a `None` table keeps what the scene has.  Every table is as
/// long as the scene's own.  Lights and materials whose kinds stay rewrite their table alone; a changed material kind
/// also the records; spheres also the bounds, the refit and the records.
pub fn edit_scene(
    ctx: *mut sys::yk_context,
    scene: *mut sys::yk_scene,
    spheres: Option<&[sys::yk_sphere_desc]>,
    lights: Option<&[sys::yk_light_desc]>,
    materials: Option<&[sys::yk_material_desc]>,
    background: Option<&[f32; 3]>,
) -> Result<sys::yk_scene_edit_info, String> {
    let edit = sys::yk_scene_edit {
        spheres: spheres.map_or(std::ptr::null(), |t| t.as_ptr()),
        lights: lights.map_or(std::ptr::null(), |t| t.as_ptr()),
        materials: materials.map_or(std::ptr::null(), |t| t.as_ptr()),
        background: background.map_or(std::ptr::null(), |b| b.as_ptr()),
    };
    let status = unsafe { sys::yk_scene_apply_edit(ctx, scene, &edit) };
    finish_edit(ctx, scene, status)
}

/// The sphere table in device memory (the scene's count of `yk_sphere_desc` records, produced on `stream`): a particle
/// simulation's output never crosses the host link.  `edit.spheres` must be null.
pub fn edit_scene_device(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, edit: &sys::yk_scene_edit, d_spheres: *const c_void, stream: *mut c_void) -> Result<sys::yk_scene_edit_info, String> {
    let status = unsafe { sys::yk_scene_apply_edit_device(ctx, scene, edit, d_spheres, stream) };
    finish_edit(ctx, scene, status)
}

fn finish_edit(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, status: sys::yk_status) -> Result<sys::yk_scene_edit_info, String> {
    if status != sys::YK_OK {
        return Err(sys::last_error(ctx));
    }
    let mut info = sys::yk_scene_edit_info::default();
    unsafe { sys::yk_scene_get_edit_info(scene, &mut info) };
    if info.route == sys::YK_UPDATE_ROUTE_HOST && info.reason != 0 {
        log::warn!("scene edit fell back to the host route (reason {})", info.reason);
    }
    Ok(info)
}
