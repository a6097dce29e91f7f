//! `yuki/src/app/window.rs` — a frame sooner: the GPU worker renders the film at 1/s of the window's resolution and this
//! pass takes it to full resolution before `tone_map_film` (window.rs:246-264).  The reference can only render a smaller
//! film and let `ScaleOutput` stretch it, which blurs every texture and smears every silhouette; the guided upsample reads
//! the first-hit guides of BOTH resolutions, filters radiance / albedo and multiplies the full-resolution albedo back
//! (`yk_upsample_device`), on the worker's stream, ahead of `yk_tone_map_device`, `yk_overlay_draw_device` and
//! `yk_present_device`.  `ctx` null runs the library's host instance (bit-identical).
//! The rule: yuki_amd/csrc/yk_upsample.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Bounds3, Vec2};
use std::ffi::c_void;
use yuki_hip_sys as sys;

/// The settings the UI exposes: `s` 1 shows the film as it is rendered.
#[derive(Clone, Copy)]
pub struct UpsampleParams {
    /// 1 ..= `YK_UPSAMPLE_MAX_S`; the window's resolution must be `s` times the low film's on both sides.
    pub s: u32,
    pub sigma_normal: f32,
    /// In scene units; `for_scene` scales it to the scene.
    pub sigma_plane: f32,
}

impl UpsampleParams {
    /// The denoiser's stops: normal 0.3, plane 0.01 x the diagonal of `scene.bvh.bounds()`.
    pub fn for_scene(bounds: Bounds3<f32>, s: u32) -> Self {
        Self {
            s,
            sigma_normal: 0.3,
            sigma_plane: 0.01 * (bounds.p_max - bounds.p_min).len(),
        }
    }

    fn desc(&self) -> sys::yk_upsample_desc {
        sys::yk_upsample_desc {
            s: self.s,
            sigma_normal: self.sigma_normal,
            sigma_plane: self.sigma_plane,
        }
    }
}

/// The low film's resolution for a window of `res`, or `None` where `s` does not divide both sides.
pub fn low_res(res: Vec2<u16>, s: u32) -> Option<Vec2<u16>> {
    if s == 0 || s > sys::YK_UPSAMPLE_MAX_S || res.x as u32 % s != 0 || res.y as u32 % s != 0 {
        return None;
    }
    Some(Vec2::new((res.x as u32 / s) as u16, (res.y as u32 / s) as u16))
}

/// The GPU worker's last step before the tone map.  When the camera or the scene changes it renders, once:
/// the low guides (`yk_render_guides_device` under the low camera), the full guides and ids
/// (`yk_render_guides_ids_device` under the window's camera), the full albedo (`yk_surface_albedo_device`) and the low
/// albedo (`yk_albedo_mean_device` of the FULL ids at factor `s`: the mean albedo of a low pixel over exactly the full
/// pixels it covers).  Per displayed frame: the accumulating pass into `d_low_film`, `denoise_albedo_device` on it with
/// `d_low_albedo`, then this, then `yk_tone_map_device(d_full, samples = null)`.  `samples`: the LOW film's table, or
/// `None` where a denoise has already normalised the film.  `d_weight` null: not wanted; otherwise one float per full
/// pixel, 0 where no low tap matched and the containing low pixel was copied.  No synchronisation here.
///
/// # Safety
/// The pointers are device allocations on `ctx`'s device that do not overlap: `d_low_film` `low.x * low.y * 12` bytes and
/// `d_full` `s * s` times that, 4-byte aligned; guides 32 bytes and albedo 16 bytes per pixel of their film, 16-byte
/// aligned; the two albedo pointers are both null or both set.
pub unsafe fn upsample_device(
    ctx: *mut sys::yk_context,
    params: &UpsampleParams,
    d_low_film: *const c_void,
    d_low_guides: *const c_void,
    d_low_albedo: *const c_void,
    low: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_guides: *const c_void,
    d_albedo: *const c_void,
    d_full: *mut c_void,
    d_weight: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_upsample_device(
        ctx,
        &params.desc(),
        d_low_film,
        d_low_guides,
        d_low_albedo,
        low.x,
        low.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_guides,
        d_albedo,
        d_full,
        d_weight,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
