//! `yuki/src/app/gpu_worker.rs` / `window.rs` — auto-exposure.  The reference's exposure is a slider
//! (`FilmicParams.exposure`, tonemap.rs:12-22); with the meter the GPU worker chooses it from the film it is about to show,
//! without the film leaving the device: after the blend (temporal.rs) and the denoise (denoise.rs) of a displayed frame,
//! `meter_device` reads the film and writes a 32-byte `yk_exposure_state` record into a device buffer the worker keeps for
//! as long as it lives — the record of one frame is the `prev` of the next, and may be the same buffer — and
//! `tone_map_metered_device` replaces `yk_tone_map_device`: the kernel multiplies `FilmicParams.exposure` (the slider, now
//! a compensation factor) by the record's exposure when it runs.  Everything is enqueued on the worker's stream; nothing
//! waits.  The worker turns the time since the last displayed frame into the two rates (`rate_for`): the library takes no
//! clock.  `ctx` null runs the library's host instance of `meter` (bit-identical).
//! The rule: yuki_amd/csrc/yk_exposure.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Spectrum, Vec2};
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct ExposureParams {
    /// Fractions of the counted pixels dropped at the dark and at the bright end before the mean.
    pub low_cut: f32,
    pub high_cut: f32,
    /// The luminance the metered value is brought to, and stops added on top.
    pub key: f32,
    pub compensation: f32,
    /// The stops applied stay in this range, itself inside [-24, 24].
    pub min_ev: f32,
    pub max_ev: f32,
    /// Per-frame rates in [0, 1] towards a brighter / a darker film; 1 adapts at once.
    pub adapt_up: f32,
    pub adapt_down: f32,
    /// `[x0, y0, x1, y1]`, half open; `None` meters the whole film.
    pub window: Option<[u16; 4]>,
}

impl Default for ExposureParams {
    fn default() -> Self {
        Self {
            low_cut: 0.05,
            high_cut: 0.02,
            key: 0.18,
            compensation: 0.0,
            min_ev: -8.0,
            max_ev: 8.0,
            adapt_up: 1.0,
            adapt_down: 1.0,
            window: None,
        }
    }
}

impl ExposureParams {
    /// The rate that closes `1 - e^(-dt / tau)` of the gap in a frame that took `dt` seconds.
    pub fn rate_for(dt: f32, tau: f32) -> f32 {
        if tau <= 0.0 {
            1.0
        } else {
            (1.0 - (-dt / tau).exp()).clamp(0.0, 1.0)
        }
    }

    fn desc(&self, res: Vec2<u16>) -> sys::yk_exposure_desc {
        sys::yk_exposure_desc {
            low_cut: (self.low_cut * 65536.0).round() as u32,
            high_cut: (self.high_cut * 65536.0).round() as u32,
            ev_bias: self.key.log2() + self.compensation,
            min_ev: self.min_ev,
            max_ev: self.max_ev,
            adapt_up: self.adapt_up,
            adapt_down: self.adapt_down,
            window: self.window.unwrap_or([0, 0, res.x, res.y]),
        }
    }
}

/// Host film in, record out (headless sequences, tests).  `samples`: `Film.samples`, or `None` for a normalised film.
pub fn meter(
    ctx: *mut sys::yk_context,
    params: &ExposureParams,
    film: &[Spectrum<f32>],
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    prev: Option<&sys::yk_exposure_state>,
) -> Result<sys::yk_exposure_state, sys::yk_status> {
    assert!(film.len() == res.x as usize * res.y as usize);
    let mut out = sys::yk_exposure_state::default();
    let status = unsafe {
        sys::yk_exposure_meter(
            ctx,
            &params.desc(res),
            film.as_ptr() as *const f32,
            res.x,
            res.y,
            tile_dim,
            samples.map_or(std::ptr::null(), |s| s.as_ptr()),
            prev.map_or(std::ptr::null(), |p| p as *const sys::yk_exposure_state),
            &mut out,
        )
    };
    if status == sys::YK_OK {
        Ok(out)
    } else {
        Err(status)
    }
}

/// The GPU worker's meter of a displayed frame, enqueued on `stream` behind the blend and the denoise: `d_film` (the film
/// the tone map is about to read) -> the record at `d_state`, after the record at `d_prev` (null on the first frame and
/// after a scene change; otherwise the last frame's, which may be `d_state` itself).
///
/// # Safety
/// `d_film` is a device film of `res` on `ctx`'s device; `d_prev` (when not null) and `d_state` are device allocations
/// of 32 bytes, 4-byte aligned.
pub unsafe fn meter_device(
    ctx: *mut sys::yk_context,
    params: &ExposureParams,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_prev: *const c_void,
    d_state: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_exposure_meter_device(
        ctx,
        &params.desc(res),
        d_film,
        res.x,
        res.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_prev,
        d_state,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// `yk_tone_map_device` for the Filmic tone map with the record's exposure multiplied in on the device: enqueued on
/// `stream` behind `meter_device`, before the overlays and `scale_output_device` (present.rs).
///
/// # Safety
/// As `meter_device`; `d_out` is a device film of `res` and may be `d_film`.
pub unsafe fn tone_map_metered_device(
    ctx: *mut sys::yk_context,
    desc: &sys::yk_tone_map_desc,
    d_state: *const c_void,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_out: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_tone_map_metered_device(
        ctx,
        desc,
        d_state,
        d_film,
        res.x,
        res.y,
        tile_dim,
        samples.map_or(std::ptr::null(), |s| s.as_ptr()),
        d_out,
        stream,
    );
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
