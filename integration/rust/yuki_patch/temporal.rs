//! `yuki/src/app/window.rs` / `gpu_worker.rs` — keep the film across camera moves.  The reference (and the GPU worker so
//! far) clears the film when the camera moves and starts again at one sample a pixel.  With these two passes the worker
//! carries the previous view's film to the new view instead: `reproject_device` once per move (previous history,
//! previous guides, previous camera, the new view's guides -> a history per pixel of the new view), and `blend_device`
//! with every displayed frame (the new view's accumulating film folded into that history), both on the worker's stream,
//! between the accumulating pass and `denoise_device` (denoise.rs), which then runs WITHOUT the sample table.  The last
//! blend's history output and that view's guides are the next move's inputs: the worker keeps two history buffers and
//! two guide buffers and swaps them when the camera moves.
//! Reprojected radiance is exact for diffuse surfaces only; on glass and metal it lags the view for as long as
//! `max_history` lets it.  `ctx` null runs the library's host instance (bit-identical).
//! The rule: yuki_amd/csrc/yk_temporal.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Bounds3, Spectrum, Vec2};
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct TemporalParams {
    /// In scene units; `for_scene` scales it to the scene.  `f32::INFINITY` switches the plane test off.
    pub plane_tolerance: f32,
    pub normal_cos_min: f32,
    /// The history never counts for more samples than this: a new sample weighs at least `1 / (max_history + 1)`.
    pub max_history: f32,
}

impl TemporalParams {
    /// Plane tolerance 0.01 x the diagonal of `scene.bvh.bounds()`, normals within acos(0.9), 64 samples of history.
    pub fn for_scene(bounds: Bounds3<f32>) -> Self {
        Self {
            plane_tolerance: 0.01 * (bounds.p_max - bounds.p_min).len(),
            normal_cos_min: 0.9,
            max_history: 64.0,
        }
    }

    fn desc(&self) -> sys::yk_temporal_desc {
        sys::yk_temporal_desc {
            plane_tolerance: self.plane_tolerance,
            normal_cos_min: self.normal_cos_min,
            max_history: self.max_history,
        }
    }
}

/// Host records in, host records out (headless sequences, tests).
pub fn reproject_history(
    ctx: *mut sys::yk_context,
    params: &TemporalParams,
    prev_history: &[sys::yk_history],
    prev_guides: &[sys::yk_guide],
    prev_camera: &sys::yk_camera,
    guides: &[sys::yk_guide],
    res: Vec2<u16>,
) -> Vec<sys::yk_history> {
    let n = res.x as usize * res.y as usize;
    assert!(prev_history.len() == n && prev_guides.len() == n && guides.len() == n);
    let mut out = vec![sys::yk_history::default(); n];
    let status = unsafe {
        sys::yk_history_reproject(
            ctx,
            &params.desc(),
            prev_history.as_ptr(),
            prev_guides.as_ptr(),
            prev_camera,
            guides.as_ptr(),
            res.x,
            res.y,
            out.as_mut_ptr(),
        )
    };
    assert!(status == sys::YK_OK, "yk_history_reproject failed: {}", status);
    out
}

/// Host pixels in: (the film of the means, the new history).  `samples` = `Film::samples` for an accumulating film.
pub fn blend_history(
    ctx: *mut sys::yk_context,
    params: &TemporalParams,
    film: &[Spectrum<f32>],
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    history: Option<&[sys::yk_history]>,
) -> (Vec<Spectrum<f32>>, Vec<sys::yk_history>) {
    let n = res.x as usize * res.y as usize;
    assert!(film.len() == n && history.map_or(true, |h| h.len() == n));
    let mut rgb = vec![Spectrum::zeros(); n];
    let mut out = vec![sys::yk_history::default(); n];
    let status = unsafe {
        sys::yk_history_blend(
            ctx,
            &params.desc(),
            film.as_ptr() as *const f32,
            res.x,
            res.y,
            tile_dim,
            samples.map_or(std::ptr::null(), |s| s.as_ptr()),
            history.map_or(std::ptr::null(), |h| h.as_ptr()),
            out.as_mut_ptr(),
            rgb.as_mut_ptr() as *mut f32,
        )
    };
    assert!(status == sys::YK_OK, "yk_history_blend failed: {}", status);
    (rgb, out)
}

/// The GPU worker, when the camera has moved (gpu_worker.rs: where it used to clear the film only), after
/// `render_guides_device` for the new view: one launch on `stream`, no allocation, no synchronisation.
///
/// # Safety
/// The pointers are device allocations on `ctx`'s device, 16-byte aligned: histories `res.x * res.y * 16` bytes, guides
/// `res.x * res.y * 32` bytes; the output overlaps none of the inputs.
pub unsafe fn reproject_device(
    ctx: *mut sys::yk_context,
    params: &TemporalParams,
    d_prev_history: *const c_void,
    d_prev_guides: *const c_void,
    prev_camera: &sys::yk_camera,
    d_guides: *const c_void,
    res: Vec2<u16>,
    d_history: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_history_reproject_device(ctx, &params.desc(), d_prev_history, d_prev_guides, prev_camera, d_guides, res.x, res.y, d_history, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// The GPU worker's first step of a displayed frame, behind the accumulating pass on `stream`: `d_film` (the raw sums of
/// the current view) and `d_reprojected` (null before the first move) -> `d_out_history` (what the next move reprojects)
/// and `d_rgb` (the means: what `denoise_device` and `yk_tone_map_device` take, with `samples = None`).  Either output
/// may be null, not both.
///
/// # Safety
/// The pointers are device allocations on `ctx`'s device: film and RGB `res.x * res.y * 12` bytes, 4-byte aligned;
/// histories `res.x * res.y * 16` bytes, 16-byte aligned; an output overlaps an input only where it is that input's own
/// counterpart (`d_out_history == d_reprojected`, `d_rgb == d_film`).
pub unsafe fn blend_device(
    ctx: *mut sys::yk_context,
    params: &TemporalParams,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_reprojected: *const c_void,
    d_out_history: *mut c_void,
    d_rgb: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_history_blend_device(
        ctx,
        &params.desc(),
        d_film,
        res.x,
        res.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_reprojected,
        d_out_history,
        d_rgb,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
