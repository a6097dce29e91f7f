//! `yuki/src/app/gpu_worker.rs` — a carried film that notices when it is wrong.  temporal.rs and motion.rs carry the
//! history across moves of the camera and of the geometry, but nothing there compares it with the frame at hand: on
//! glass and metal, under moved shadows and after a change of lighting the old radiance lingers until `max_history` lets
//! it go.  `rectify_device` runs on the worker's stream before `temporal::blend_device` on EVERY frame — after
//! `reproject_device` / `motion.rs` when something moved, on the last blend's history while the view stands — and clips
//! each pixel's history to the box (mean +- gamma standard deviations, per channel) of the current film around it; a
//! clipped pixel's count shrinks by how far it was moved, so the blend behind it trusts the new samples.  With the moments
//! buffer of variance.rs beside the history, hand both: the moments' count follows the history's.
//! Limits: a per-channel RGB box; the moments' m1 and m2 are not rectified; a wrong history inside the frame's noise box
//! stays; `yk_multi` scenes are not served.  The rule: yuki_amd/csrc/yk_rectify.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::Vec2;
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct RectifyParams {
    /// The window is (2 radius + 1)^2 pixels, radius 1 .. 3.
    pub radius: u32,
    /// The half-width of the box in standard deviations, >= 0; `f32::INFINITY` lets every history through.
    pub gamma: f32,
}

impl Default for RectifyParams {
    /// The best row of profiles/rectify_quality.json.
    fn default() -> Self {
        Self { radius: 2, gamma: 0.75 }
    }
}

impl RectifyParams {
    fn desc(&self) -> sys::yk_rectify_desc {
        sys::yk_rectify_desc { radius: self.radius, gamma: self.gamma }
    }
}

/// Before `temporal::blend_device`, from the same `d_film` and sample table: `d_history` -> `d_out_history` (may be
/// `d_history`), and `d_moments` -> `d_out_moments` (may be `d_moments`; both null without a moments buffer).  One launch.
///
/// # Safety
/// Device allocations on `ctx`'s device: the film `res.x * res.y * 12` bytes, 4-byte aligned; history and moments
/// `res.x * res.y * 16` bytes each, 16-byte aligned; an output overlaps nothing but the input it may replace.
pub unsafe fn rectify_device(
    ctx: *mut sys::yk_context,
    params: &RectifyParams,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_history: *const c_void,
    d_moments: *const c_void,
    d_out_history: *mut c_void,
    d_out_moments: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_history_rectify_device(ctx, &params.desc(), d_film, res.x, res.y, tile_dim, samples.map_or(std::ptr::null(), |s| s.as_ptr()), d_history, d_moments, d_out_history, d_out_moments, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
