//! `yuki/src/app/gpu_worker.rs` — a progressive render that puts its samples where the film is still noisy.  Instead of
//! one more uniform pass over every tile the worker keeps, beside a film of RGB SUMS, one `yk_pixel_stats` a pixel (both
//! cleared with zeros) and calls `render_adaptive_device`: rounds of select -> render the selected pixels -> fold, until
//! nothing is selected.  A later call with a larger `max_samples` refines the same film.  For display:
//! `resolve_device` (sums + statistics -> the mean film and the variance of that mean), whose variance goes straight into
//! `variance::denoise_variance_device`.  Luminance only; `yk_multi` scenes are not served; selecting on the samples' own
//! variance biases the estimate slightly.  The rule: yuki_amd/csrc/yk_adaptive.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::Vec2;
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct AdaptiveParams {
    pub min_samples: u32,
    /// At most the sampler's samples per pixel.
    pub max_samples: u32,
    pub round_passes: u32,
    /// 0: until nothing is selected.
    pub max_rounds: u32,
    pub dilate: bool,
    pub threshold: f32,
    pub epsilon: f32,
}

impl AdaptiveParams {
    /// The defaults of profiles/adaptive_quality.json under a sampler of `samples_per_pixel`.
    pub fn for_sampler(samples_per_pixel: u32) -> Self {
        Self { min_samples: 16, max_samples: samples_per_pixel, round_passes: 8, max_rounds: 0, dilate: true, threshold: 0.2, epsilon: 0.05 }
    }

    fn desc(&self) -> sys::yk_adaptive_desc {
        sys::yk_adaptive_desc {
            min_samples: self.min_samples,
            max_samples: self.max_samples,
            round_passes: self.round_passes,
            max_rounds: self.max_rounds,
            dilate: self.dilate as u32,
            threshold: self.threshold,
            epsilon: self.epsilon,
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

/// Continues from whatever `d_film_sum` and `d_stats` hold; synchronous (one count read-back per round).  After
/// `YK_ERR_CANCELLED` both buffers are undefined.
///
/// # Safety
/// Device allocations on `ctx`'s device: the film sums `res.x * res.y * 12` bytes, 4-byte aligned; the statistics
/// `res.x * res.y * 16` bytes, 16-byte aligned; they do not overlap.
pub unsafe fn render_adaptive_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera: &sys::yk_camera,
    sampler: &sys::yk_sampler_desc,
    integrator: &sys::yk_integrator_desc,
    params: &AdaptiveParams,
    res: Vec2<u16>,
    d_film_sum: *mut c_void,
    d_stats: *mut c_void,
    stream: *mut c_void,
    cancel: sys::yk_cancel_fn,
    user: *mut c_void,
) -> Result<sys::yk_adaptive_info, sys::yk_status> {
    let mut info = sys::yk_adaptive_info::default();
    result(sys::yk_render_adaptive_device(ctx, scene, camera, sampler, integrator, &params.desc(), res.x, res.y, d_film_sum, d_stats, stream, &mut info, cancel, user))?;
    Ok(info)
}

/// The mean film and / or the variance of that mean (null: not wanted), one launch on `stream`.
///
/// # Safety
/// As `render_adaptive_device`; the outputs (`res.x * res.y * 12` and `* 4` bytes, 4-byte aligned) overlap nothing.
pub unsafe fn resolve_device(
    ctx: *mut sys::yk_context,
    d_film_sum: *const c_void,
    d_stats: *const c_void,
    res: Vec2<u16>,
    d_rgb: *mut c_void,
    d_variance: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    result(sys::yk_adaptive_resolve_device(ctx, d_film_sum, d_stats, res.x, res.y, d_rgb, d_variance, stream))
}
