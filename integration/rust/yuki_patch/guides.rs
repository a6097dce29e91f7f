//! `yuki/src/app/gpu_worker.rs` — guides that see through glass.  Every film pass of the worker (denoise.rs, temporal.rs,
//! motion.rs, rectify.rs, upsample.rs) steers itself by the guide and the surface id of the pixel's FIRST hit; where that
//! is a pane, the records describe the pane: one normal, one plane, an albedo of ones.  `guides_through_device` stands where
//! `motion::guides_ids_device` stood and writes the same two records at the first hit that is not glass — transmission
//! followed, reflection on total internal reflection or a black Kt — for up to `max_through` interfaces, with the number
//! of interfaces crossed beside them.  Same layouts, so every later call takes the buffers unchanged; `max_through = 0`
//! is `guides_ids_device` byte for byte.  One stream, no allocation, no read-back: 1 + max_through traces.
//! Limits: one branch per interface (a pane's mirror image is not guided); the albedo behind tinted glass ignores Kt;
//! `p` is the real position of what is seen, so reprojection through refraction is approximate.
//! The rule: yuki_amd/csrc/yk_guides_through.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::Vec2;
use std::ffi::c_void;
use yuki_hip_sys as sys;

fn done(status: sys::yk_status) -> Result<(), sys::yk_status> {
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// The worker's default: a window in front of a room is two interfaces, a glass ball two, a ball behind a window four.
pub const DEFAULT_MAX_THROUGH: u32 = 4;

/// # Safety
/// `d_guides` (`res.x * res.y * 32` bytes) and `d_ids` (`res.x * res.y * 16` bytes) are device allocations on `ctx`'s
/// device, 16-byte aligned; `d_through` (`res.x * res.y * 4` bytes) is 4-byte aligned; no two overlap; any may be null,
/// not all three.  `max_through <= sys::YK_GUIDES_THROUGH_MAX`.
pub unsafe fn guides_through_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera: &sys::yk_camera,
    res: Vec2<u16>,
    max_through: u32,
    d_guides: *mut c_void,
    d_ids: *mut c_void,
    d_through: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    done(sys::yk_render_guides_through_device(ctx, scene, camera, res.x, res.y, max_through, d_guides, d_ids, d_through, stream))
}

/// Once per view, before the frame's passes: the guides and ids of what every pixel shows, then the albedo of those ids
/// (denoise.rs' `albedo_device` takes them as it takes first-hit ids).
///
/// # Safety
/// As above; `d_albedo` is `res.x * res.y * 16` bytes, 16-byte aligned, apart from the ids.
pub unsafe fn guides_and_albedo_through(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera: &sys::yk_camera,
    res: Vec2<u16>,
    d_guides: *mut c_void,
    d_ids: *mut c_void,
    d_albedo: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    guides_through_device(ctx, scene, camera, res, DEFAULT_MAX_THROUGH, d_guides, d_ids, std::ptr::null_mut(), stream)?;
    done(sys::yk_surface_albedo_device(ctx, scene, d_ids, res.x, res.y, d_albedo, stream))
}
