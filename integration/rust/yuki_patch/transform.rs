//! `yuki/src/app/gpu_worker.rs` — "this mesh is now at that matrix".  `update.rs` moves vertices: its caller transforms
//! every vertex and normal itself, keeps the rest pose, hands over a full vertex array every frame and keeps the previous
//! one alive for `motion.rs`.  With `yk_scene_transform[_device]` the worker hands over one pair of matrices a mesh — 128
//! bytes — and the library keeps the rest pose (the points and normals after creation or the last update), applies
//! `Transform * Point3` and `Transform * Normal` as `Mesh::new` does (shapes/mesh.rs:27-33), flips a mirrored mesh's
//! `swaps_handedness`, refits the tree and rewrites the records, on the device when the records are there or the scene was
//! laid out there.  For the film, `yk_surface_motion_transforms[_device]` takes the PREVIOUS frame's records where
//! `motion.rs` takes the previous vertex buffer.  What the caller must keep in mind:
//!   * transforms are absolute, relative to the rest pose: A then B is B, the identity restores the rest pose's bytes;
//!   * the pair (rest_to_world, world_to_rest) is the caller's, as a sphere's pair is: the library does not invert;
//!   * a mesh whose triangles carry a rectangular light cannot move, a vertex must belong to one mesh, every matrix entry
//!     and every result must be finite — otherwise the call is refused and the scene stays as it was;
//!   * `update_scene` afterwards makes a new rest pose and resets the flags to creation's;
//!   * a refit keeps the tree's topology: `tree_cost` against `tree_cost_rest` (both relative to their root's area) says
//!     how much worse the tree has become; re-create the scene when it has drifted too far;
//!   * no instancing, no change of counts or indices, no scenes of a yk_multi.
//! The rule: yuki_amd/csrc/yk_scene_transform.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use std::ffi::c_void;
use yuki_hip_sys as sys;

/// The identity pair: the mesh stands at its rest pose.
pub fn identity() -> sys::yk_mesh_transform {
    let mut m = [0.0f32; 16];
    for k in 0..4 {
        m[5 * k] = 1.0;
    }
    sys::yk_mesh_transform { rest_to_world: m, world_to_rest: m }
}

/// A record from yuki's `Transform` (row-major matrix and its inverse, both kept by the type).
pub fn record(m: &[[f32; 4]; 4], m_inv: &[[f32; 4]; 4]) -> sys::yk_mesh_transform {
    let mut out = identity();
    for r in 0..4 {
        for c in 0..4 {
            out.rest_to_world[4 * r + c] = m[r][c];
            out.world_to_rest[4 * r + c] = m_inv[r][c];
        }
    }
    out
}

/// One record for each of the scene's meshes, on the host.
pub fn transform_scene(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, transforms: &[sys::yk_mesh_transform]) -> Result<sys::yk_scene_transform_info, String> {
    let status = unsafe { sys::yk_scene_transform(ctx, scene, transforms.as_ptr()) };
    finish(ctx, scene, status)
}

/// The records in device memory (4-byte aligned, produced on `stream`): an animation kernel's output never crosses the host link.
pub fn transform_scene_device(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, d_transforms: *const c_void, stream: *mut c_void) -> Result<sys::yk_scene_transform_info, String> {
    let status = unsafe { sys::yk_scene_transform_device(ctx, scene, d_transforms, stream) };
    finish(ctx, scene, status)
}

fn finish(ctx: *mut sys::yk_context, scene: *mut sys::yk_scene, status: sys::yk_status) -> Result<sys::yk_scene_transform_info, String> {
    if status != sys::YK_OK {
        return Err(sys::last_error(ctx));
    }
    let mut info = sys::yk_scene_transform_info::default();
    unsafe { sys::yk_scene_get_transform_info(scene, &mut info) };
    if info.route == sys::YK_UPDATE_ROUTE_HOST && info.reason != 0 {
        log::warn!("scene transform fell back to the host route (reason {})", info.reason);
    }
    Ok(info)
}

/// `motion.rs`' step with the previous frame's records (null: the scene stood at rest) instead of the previous vertex
/// buffer; `d_prev_spheres` as there (null: the spheres did not move).  Enqueued on `stream`, one launch.
pub fn motion_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    d_ids: *const c_void,
    d_guides: *const c_void,
    d_prev_transforms: *const c_void,
    d_prev_spheres: *const c_void,
    res: (u16, u16),
    d_out: *mut c_void,
    stream: *mut c_void,
) -> Result<(), String> {
    let status = unsafe { sys::yk_surface_motion_transforms_device(ctx, scene, d_ids, d_guides, d_prev_transforms, d_prev_spheres, res.0, res.1, d_out, stream) };
    if status != sys::YK_OK {
        return Err(sys::last_error(ctx));
    }
    Ok(())
}
