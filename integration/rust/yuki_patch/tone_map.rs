//! `yuki/src/app/headless.rs` — `apply_tone_map` (headless.rs:113-158) without a GL context: the same
//! `(width, height, pixels)` from `yk_tone_map`, so `yuki --out` writes the tone-mapped film on a machine with no
//! display.  `ctx` null runs the library's host instance; a `HipDevice`'s context runs it on the GPU (bit-identical).
//! The evaluation order and the two reproduced quirks of the shaders: include/yuki_hip.h, yk_tonemap.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::{
    app::renderpasses::{HeatmapParams, ToneMapType},
    film::{Film, FilmSettings},
    math::Spectrum,
};
use std::sync::Mutex;
use yuki_hip_sys as sys;

pub fn tone_map_desc(tone_map: ToneMapType) -> sys::yk_tone_map_desc {
    let mut d = sys::yk_tone_map_desc::default();
    match tone_map {
        ToneMapType::Raw => d.kind = sys::YK_TONE_MAP_RAW,
        ToneMapType::Filmic(p) => {
            d.kind = sys::YK_TONE_MAP_FILMIC;
            d.exposure = p.exposure;
        }
        ToneMapType::Heatmap(HeatmapParams { bounds, channel }) => {
            d.kind = sys::YK_TONE_MAP_HEATMAP;
            d.channel = channel as u32;
            // No bounds: the library runs find_min_max first, as headless.rs:135-145 does.
            if let Some((lo, hi)) = bounds {
                d.has_bounds = 1;
                d.bounds = [lo, hi];
            }
        }
    }
    d
}

/// Drop-in for headless.rs:113-158: `let (w, h, pixels) = apply_tone_map(tone_map, &film, film_settings, ptr::null_mut());`
pub fn apply_tone_map(
    tone_map: ToneMapType,
    film: &Mutex<Film>,
    _film_settings: FilmSettings,
    ctx: *mut sys::yk_context,
) -> (usize, usize, Vec<Spectrum<f32>>) {
    let film = film.lock().expect("Failed to lock film");
    let res = film.res();
    let desc = tone_map_desc(tone_map);
    // tonemap.rs:238: Film::tile_dim(), 16 without tiles; Film.samples in FilmTile.index order (None: no division)
    let tile_dim = film.tile_dim().unwrap_or(16);
    let samples = film.samples().map_or(std::ptr::null(), |s| s.as_ptr());
    let pixels = film.pixels();
    let mut out = vec![Spectrum::<f32>::zeros(); pixels.len()];
    let status = unsafe {
        sys::yk_tone_map(
            ctx,
            &desc,
            pixels.as_ptr() as *const f32,
            res.x,
            res.y,
            tile_dim,
            samples,
            out.as_mut_ptr() as *mut f32,
            std::ptr::null_mut(),
        )
    };
    assert!(status == sys::YK_OK, "yk_tone_map failed: {}", status);
    (res.x as usize, res.y as usize, out)
}
