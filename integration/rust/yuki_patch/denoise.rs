//! `yuki/src/app/window.rs` — a guided denoiser between the film and `tone_map_film` (window.rs:246-264).  The reference
//! shows its raw Monte-Carlo film; with the GPU worker an accumulating 1080p pass takes a few milliseconds, so the first
//! few dozen frames of a view are noise.  This pass filters them: first-hit guides (`yk_render_guides_device`, rendered
//! again only when the camera or the scene changes) and an edge-avoiding à-trous filter (`yk_denoise_device`), both on
//! the worker's stream, ahead of `yk_tone_map_device`, `yk_overlay_draw_device` and `yk_present_device`.
//! `ctx` null runs the library's host instance of the filter (bit-identical).  The rule: yuki_amd/csrc/yk_denoise.h.
//! SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Bounds3, Spectrum, Vec2};
use std::ffi::c_void;
use yuki_hip_sys as sys;

/// The settings the UI exposes: `iterations` 0 shows the film as it is.
#[derive(Clone, Copy)]
pub struct DenoiseParams {
    pub iterations: u32,
    pub sigma_color: f32,
    pub sigma_normal: f32,
    /// In scene units; `for_scene` scales it to the scene.
    pub sigma_plane: f32,
}

impl DenoiseParams {
    /// 5 iterations, colour 4.0, normal 0.3, plane 0.01 x the diagonal of `scene.bvh.bounds()`.
    pub fn for_scene(bounds: Bounds3<f32>) -> Self {
        Self {
            iterations: 5,
            sigma_color: 4.0,
            sigma_normal: 0.3,
            sigma_plane: 0.01 * (bounds.p_max - bounds.p_min).len(),
        }
    }

    fn desc(&self) -> sys::yk_denoise_desc {
        sys::yk_denoise_desc {
            iterations: self.iterations,
            sigma_color: self.sigma_color,
            sigma_normal: self.sigma_normal,
            sigma_plane: self.sigma_plane,
        }
    }
}

/// Host pixels in, host pixels out (headless `--out`, tests): `film` row-major `res.x * res.y`, `guides` alike,
/// `samples` = `Film::samples` for an accumulating film.  The result is normalised: tone-map it WITHOUT the table.
pub fn denoise_film(
    ctx: *mut sys::yk_context,
    params: &DenoiseParams,
    film: &[Spectrum<f32>],
    guides: &[sys::yk_guide],
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
) -> Vec<Spectrum<f32>> {
    let n = res.x as usize * res.y as usize;
    assert!(film.len() == n && guides.len() == n);
    let mut out = vec![Spectrum::zeros(); n];
    let status = unsafe {
        sys::yk_denoise(
            ctx,
            &params.desc(),
            film.as_ptr() as *const f32,
            guides.as_ptr(),
            res.x,
            res.y,
            tile_dim,
            samples.map_or(std::ptr::null(), |s| s.as_ptr()),
            out.as_mut_ptr() as *mut f32,
        )
    };
    assert!(status == sys::YK_OK, "yk_denoise failed: {}", status);
    out
}

/// The GPU worker, when the camera or the scene has changed (gpu_worker.rs: where it resets the accumulation):
/// `d_guides` is a device buffer of `res.x * res.y * 32` bytes, 16-byte aligned, made once per film size.
///
/// # Safety
/// `d_guides` is a device allocation of that size on `ctx`'s device; `scene` was created on it.
pub unsafe fn render_guides_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera: &sys::yk_camera,
    res: Vec2<u16>,
    d_guides: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_render_guides_device(ctx, scene, camera, res.x, res.y, d_guides, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// The GPU worker's first step of a displayed frame, behind the accumulating pass on `stream`: `d_film` (the raw sums)
/// -> `d_clean` (normalised and filtered; may be `d_film` itself when the sums are not needed again — the worker keeps
/// accumulating, so it passes a second buffer).  Then `yk_tone_map_device(d_clean, samples = null)`, the overlays,
/// `yk_present_device`.  No synchronisation here.
///
/// # Safety
/// The pointers are device allocations on `ctx`'s device: film and output `res.x * res.y * 12` bytes, 4-byte aligned;
/// guides as above; the guides do not overlap the output.
pub unsafe fn denoise_device(
    ctx: *mut sys::yk_context,
    params: &DenoiseParams,
    d_film: *const c_void,
    d_guides: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_clean: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_denoise_device(
        ctx,
        &params.desc(),
        d_film,
        d_guides,
        res.x,
        res.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_clean,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// Textures under the denoiser (yuki_amd/csrc/yk_albedo.h).  Where the worker renders its guides it renders the ids beside
/// them (`yk_render_guides_ids_device`, motion.rs) and turns them into the diffuse albedo of every first hit: `d_albedo`
/// is a device buffer of `res.x * res.y * 16` bytes, 16-byte aligned, made once per film size.  Like the guides it changes
/// only with the camera or the scene.
///
/// # Safety
/// `d_ids` and `d_albedo` are device allocations of `res.x * res.y * 16` bytes on `ctx`'s device, 16-byte aligned, not
/// overlapping; `scene` was created on it.
pub unsafe fn albedo_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    d_ids: *const c_void,
    res: Vec2<u16>,
    d_albedo: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_surface_albedo_device(ctx, scene, d_ids, res.x, res.y, d_albedo, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// The pixel-mean albedo (yuki_amd/csrc/yk_albedo.h, `al_mean_pixel`): where texels or edges are smaller than a pixel,
/// the worker fills `d_albedo` with this instead of `albedo_device` — the mean of the first-hit albedo over an `s x s`
/// grid of sub-pixel rays, in the same 16-byte record, so `denoise_albedo_device` below takes it unchanged.  It needs no
/// ids: the library traces the `s`-times larger film itself, in bands through a scratch the context owns.  `camera_ss` is
/// the `yk_camera` of that larger film: `yk_camera_init` with `res = (s * res.x, s * res.y)` and otherwise the parameters
/// of the film's own camera.  Like the guides it changes only with the camera or the scene; at 1080p `s = 2` costs about
/// three guide passes and `s = 4` about ten, so the worker calls it once per view, not per displayed
/// frame.
///
/// # Safety
/// `d_albedo` is a device allocation of `res.x * res.y * 16` bytes on `ctx`'s device, 16-byte aligned; `scene` was created
/// on it; `1 <= s <= YK_ALBEDO_MEAN_MAX_S` and `s * res` fits 16 bits.
pub unsafe fn albedo_mean_device(
    ctx: *mut sys::yk_context,
    scene: *const sys::yk_scene,
    camera_ss: &sys::yk_camera,
    res: Vec2<u16>,
    s: u32,
    d_albedo: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_render_albedo_mean_device(ctx, scene, camera_ss, res.x, res.y, s, d_albedo, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// `denoise_device` on radiance / albedo: the filter no longer has to choose between blurring a texture and keeping the
/// noise on it.  Glass, metal, glossy surfaces and textured spheres are filtered as before (their albedo record is all
/// ones).  `d_albedo` is `albedo_device`'s record of the centre ray or, where texels are smaller than a pixel,
/// `albedo_mean_device`'s mean over the pixel.  After a temporal blend the blended RGB goes in with `samples = None`, as
/// it goes into `denoise_device`.
///
/// # Safety
/// As `denoise_device`; `d_albedo` is `albedo_device`'s buffer and does not overlap the output.
pub unsafe fn denoise_albedo_device(
    ctx: *mut sys::yk_context,
    params: &DenoiseParams,
    d_film: *const c_void,
    d_guides: *const c_void,
    d_albedo: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_clean: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_denoise_albedo_device(
        ctx,
        &params.desc(),
        d_film,
        d_guides,
        d_albedo,
        res.x,
        res.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_clean,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
