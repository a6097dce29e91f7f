//! `yuki/src/app/gpu_worker.rs` — a denoiser that knows how converged each pixel is.  Beside the colour history of
//! temporal.rs the worker keeps a moments buffer of the same size and layout: `moments_blend_device` folds every frame's
//! film into it (the same film `blend_device` folds into the history), and when the camera or the geometry moves the
//! buffer goes through `temporal::reproject_device` / `motion.rs` exactly as the history does — `yk_moments` has the
//! layout of `yk_history`.  Per displayed frame, behind `blend_device` on the worker's stream: `variance_device` (moments +
//! the blended RGB -> one float a pixel), then `denoise_variance_device` where `denoise_device` stood (denoise.rs).
//! Variance of luminance only; `yk_multi` scenes are not served; on glass and metal the temporal estimate lags with the
//! history.  The rule: yuki_amd/csrc/yk_variance.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Bounds3, Vec2};
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct VarianceParams {
    pub iterations: u32,
    pub sigma_variance: f32,
    pub sigma_normal: f32,
    /// In scene units; `for_scene` scales it to the scene.
    pub sigma_plane: f32,
    pub epsilon: f32,
    pub spatial_scale: f32,
}

impl VarianceParams {
    /// The defaults of profiles/variance_quality.json, the plane stop 0.01 x the diagonal of `scene.bvh.bounds()`.
    pub fn for_scene(bounds: Bounds3<f32>) -> Self {
        Self {
            iterations: 5,
            sigma_variance: 3.0,
            sigma_normal: 0.3,
            sigma_plane: 0.01 * (bounds.p_max - bounds.p_min).len(),
            epsilon: 1e-8,
            spatial_scale: 1.0,
        }
    }

    fn desc(&self) -> sys::yk_variance_desc {
        sys::yk_variance_desc {
            iterations: self.iterations,
            sigma_variance: self.sigma_variance,
            sigma_normal: self.sigma_normal,
            sigma_plane: self.sigma_plane,
            epsilon: self.epsilon,
            spatial_scale: self.spatial_scale,
        }
    }
}

fn result(status: sys::yk_status) -> Result<(), sys::yk_status> {
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// Behind `temporal::blend_device`, from the same `d_film` and with the same `temporal` desc: `d_reprojected` (null
/// before the first frame) -> `d_out_moments` (may be `d_reprojected`).
///
/// # Safety
/// Device allocations on `ctx`'s device: the film `res.x * res.y * 12` bytes, 4-byte aligned; moments
/// `res.x * res.y * 16` bytes, 16-byte aligned.
pub unsafe fn moments_blend_device(
    ctx: *mut sys::yk_context,
    temporal: &sys::yk_temporal_desc,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_reprojected: *const c_void,
    d_out_moments: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    result(sys::yk_moments_blend_device(ctx, temporal, d_film, res.x, res.y, tile_dim, samples.map_or(std::ptr::null(), |s| s.as_ptr()), d_reprojected, d_out_moments, stream))
}

/// `d_rgb` is `blend_device`'s RGB output (the means: no sample table); `d_albedo` null unless the demodulated filter runs.
///
/// # Safety
/// Device allocations on `ctx`'s device: RGB and variance 4-byte aligned (`res.x * res.y * 12` and `* 4` bytes), moments,
/// guides and albedo 16-byte aligned; the output overlaps no input.
pub unsafe fn variance_device(
    ctx: *mut sys::yk_context,
    params: &VarianceParams,
    d_moments: *const c_void,
    d_rgb: *const c_void,
    d_guides: *const c_void,
    d_albedo: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    d_variance: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    result(sys::yk_variance_device(ctx, &params.desc(), d_moments, d_rgb, d_guides, d_albedo, res.x, res.y, tile_dim, std::ptr::null(), d_variance, stream))
}

/// Where `denoise::denoise_device` stood; `d_out` may be `d_rgb`.
///
/// # Safety
/// As `variance_device`; the output overlaps no input but the film it may replace.
pub unsafe fn denoise_variance_device(
    ctx: *mut sys::yk_context,
    params: &VarianceParams,
    d_rgb: *const c_void,
    d_guides: *const c_void,
    d_variance: *const c_void,
    d_albedo: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    d_out: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    result(sys::yk_denoise_variance_device(ctx, &params.desc(), d_rgb, d_guides, d_variance, d_albedo, res.x, res.y, tile_dim, std::ptr::null(), d_out, stream))
}
