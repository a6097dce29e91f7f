//! `yuki/src/app/gpu_worker.rs` — keep the film when the GEOMETRY moves.  After `update_device` (update.rs) the worker
//! used to clear the film: `reproject_device` (temporal.rs) projects a pixel's CURRENT position into the previous camera,
//! and that position belongs to another surface point of the previous frame.  With these three calls the worker carries
//! the film through the move instead, all on its stream, with no allocation and no synchronisation:
//!   1. `guides_ids_device`   the new geometry's guides with a surface id beside each (one trace, the guide pass itself);
//!   2. `motion_device`       id + the PREVIOUS vertex buffer -> where every pixel's surface point stood;
//!   3. `reproject_moved_device`  the previous history carried from there;
//! then `blend_device`, `denoise_device` and the tone map as after a camera move.  The worker keeps the vertex buffer it
//! handed to the previous update (the scene copies what it is given) and swaps its two vertex buffers with every update.
//! The normal in the plane and normal tests is the current one: exact for translations, approximate under rotations; a
//! surface that turns by more than acos(normal_cos_min) between frames loses its history.  Carried radiance is the
//! radiance the surface had: shadows and reflections of things that moved lag for as long as `max_history` lets them.
//! Spheres move through `edit_scene` (update.rs): `motion_spheres_device` takes the sphere table from before the edit
//! beside the previous vertex buffer and carries a moved sphere's pixels along.  Lights carry no film.  After
//! `transform_scene_device` (transform.rs) the previous frame's records, 128 bytes a mesh, stand in for the previous vertex
//! buffer: `transform::motion_device`.  The rule: yuki_amd/csrc/yk_motion.h, yk_temporal.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::Vec2;
use crate::yuki_patch::temporal::TemporalParams;
use std::ffi::c_void;
use yuki_hip_sys as sys;

fn done(status: sys::yk_status) -> Result<(), sys::yk_status> {
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// # Safety
/// `d_guides` (`res.x * res.y * 32` bytes) and `d_ids` (`res.x * res.y * 16` bytes) are device allocations on `ctx`'s
/// device, 16-byte aligned and apart; either may be null, not both.
pub unsafe fn guides_ids_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera: &sys::yk_camera,
    res: Vec2<u16>,
    d_guides: *mut c_void,
    d_ids: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    done(sys::yk_render_guides_ids_device(ctx, scene, camera, res.x, res.y, d_guides, d_ids, stream))
}

/// # Safety
/// As above; `d_prev_points` holds three floats for each of the scene's vertices (the library cannot see its length) and
/// `d_motion` is `res.x * res.y * 16` bytes, 16-byte aligned, overlapping no input.
pub unsafe fn motion_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    d_ids: *const c_void,
    d_guides: *const c_void,
    d_prev_points: *const f32,
    res: Vec2<u16>,
    d_motion: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    done(sys::yk_surface_motion_device(ctx, scene, d_ids, d_guides, d_prev_points, res.x, res.y, d_motion, stream))
}

/// `motion_device` with the sphere case: `d_prev_spheres` is the scene's count of `yk_sphere_desc` records as they were
/// before the last edit (4-byte aligned); null is `motion_device`.
///
/// # Safety
/// As `motion_device`; `d_prev_points` may be null for a scene without triangles.
pub unsafe fn motion_spheres_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    d_ids: *const c_void,
    d_guides: *const c_void,
    d_prev_points: *const f32,
    d_prev_spheres: *const c_void,
    res: Vec2<u16>,
    d_motion: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    done(sys::yk_surface_motion_spheres_device(ctx, scene, d_ids, d_guides, d_prev_points, d_prev_spheres, res.x, res.y, d_motion, stream))
}

/// # Safety
/// As `temporal::reproject_device`, with `d_motion` from `motion_device`.
pub unsafe fn reproject_moved_device(
    ctx: *mut sys::yk_context,
    params: &TemporalParams,
    d_prev_history: *const c_void,
    d_prev_guides: *const c_void,
    prev_camera: &sys::yk_camera,
    d_guides: *const c_void,
    d_motion: *const c_void,
    res: Vec2<u16>,
    d_history: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let desc = sys::yk_temporal_desc {
        plane_tolerance: params.plane_tolerance,
        normal_cos_min: params.normal_cos_min,
        max_history: params.max_history,
    };
    done(sys::yk_history_reproject_moved_device(ctx, &desc, d_prev_history, d_prev_guides, prev_camera, d_guides, d_motion, res.x, res.y, d_history, stream))
}

/// The worker's sequence after the geometry moved, before the frame's accumulating passes.  `d_prev_points` is the buffer
/// given to the PREVIOUS update; `d_new_points` the one this update takes.
///
/// # Safety
/// Everything above, and `update.rs`' `update_device` for the two vertex buffers.
pub unsafe fn carry_film_through_update(
    ctx: *mut sys::yk_context,
    scene: *mut sys::yk_scene,
    camera: &sys::yk_camera,
    params: &TemporalParams,
    res: Vec2<u16>,
    d_new_points: *const f32,
    d_prev_points: *const f32,
    d_prev_history: *const c_void,
    d_prev_guides: *const c_void,
    d_guides: *mut c_void,
    d_ids: *mut c_void,
    d_motion: *mut c_void,
    d_history: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    done(sys::yk_scene_update_device(ctx, scene, d_new_points, std::ptr::null(), stream))?;
    guides_ids_device(ctx, scene, camera, res, d_guides, d_ids, stream)?;
    motion_device(ctx, scene, d_ids, d_guides, d_prev_points, res, d_motion, stream)?;
    // the camera stood: the previous camera is the current one
    reproject_moved_device(ctx, params, d_prev_history, d_prev_guides, camera, d_guides, d_motion, res, d_history, stream)
}
