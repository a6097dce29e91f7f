//! `yuki/src/app/gpu_worker.rs` — fireflies clamped before anything keeps them.  A pixel of the current frame that is far
//! brighter than everything around it enters `temporal::blend_device` at full weight and stays visible for `max_history`
//! frames, widens the box `rectify::rectify_device` clips against, inflates the luminance moments of variance.rs and
//! survives the à-trous filter.  `despeckle_device` runs on the worker's stream FIRST in a frame, on the current frame's
//! film: a pixel whose luminance exceeds `gain` x the rank-th largest luminance among the other pixels of its
//! (2 radius + 1)^2 window is scaled down to that bound, its chromaticity kept, into a second film buffer; rectify, blend
//! and moments blend then take that buffer with the same sample table (a film of sums stays a film of sums).
//! Limits: biased by design — it removes energy from heavy-tailed light transport and is not for a film meant to
//! converge; luminance only; a real glint narrower than the window's rank is clamped too; `yk_multi` scenes are not
//! served.  Off unless the worker asks for it.  The rule: yuki_amd/csrc/yk_despeckle.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::Vec2;
use std::ffi::c_void;
use yuki_hip_sys as sys;

#[derive(Clone, Copy)]
pub struct DespeckleParams {
    /// The window is the (2 radius + 1)^2 - 1 pixels around a pixel, radius 1 .. 2.
    pub radius: u32,
    /// The rank-th largest neighbour luminance bounds the pixel, 1 .. 4 (1 = the maximum).
    pub rank: u32,
    /// >= 0; `f32::INFINITY` clamps nothing.
    pub gain: f32,
    /// Fewer usable neighbours than max(min_taps, rank) and the pixel passes through.
    pub min_taps: u32,
    /// A luminance below which nothing is clamped, >= 0 and finite.
    pub floor: f32,
    /// A pixel that is not finite becomes the mean of its usable neighbours.
    pub repair: bool,
}

impl Default for DespeckleParams {
    /// radius, rank and gain: the best row of profiles/despeckle_quality.json.
    fn default() -> Self {
        Self { radius: 2, rank: 3, gain: 1.5, min_taps: 3, floor: 0.0, repair: false }
    }
}

impl DespeckleParams {
    fn desc(&self) -> sys::yk_despeckle_desc {
        sys::yk_despeckle_desc {
            radius: self.radius,
            rank: self.rank,
            min_taps: self.min_taps.max(self.rank),
            flags: if self.repair { sys::YK_DESPECKLE_REPAIR } else { 0 },
            gain: self.gain,
            floor: self.floor,
        }
    }
}

/// First in a frame: `d_film` -> `d_out_film`, which the later passes take with the same sample table.  `d_out_mask`
/// (one byte a pixel: 0 untouched, 1 clamped, 2 repaired) and `d_out_counts` (two u32: clamped, repaired) may be null;
/// the counts cost two atomics per block on two addresses, ask for them only when they are shown.  One launch.
///
/// # Safety
/// Device allocations on `ctx`'s device: the films `res.x * res.y * 12` bytes each, 4-byte aligned, sharing no byte
/// (the pass does not run in place); the mask `res.x * res.y` bytes; the counts 8 bytes, 4-byte aligned.
pub unsafe fn despeckle_device(
    ctx: *mut sys::yk_context,
    params: &DespeckleParams,
    d_film: *const c_void,
    res: Vec2<u16>,
    tile_dim: u16,
    samples: Option<&[u32]>,
    d_out_film: *mut c_void,
    d_out_mask: *mut c_void,
    d_out_counts: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_despeckle_device(ctx, &params.desc(), d_film, res.x, res.y, tile_dim, samples.map_or(std::ptr::null(), |s| s.as_ptr()), d_out_film, d_out_mask, d_out_counts, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
