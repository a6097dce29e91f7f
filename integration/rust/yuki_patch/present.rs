//! `yuki/src/app/window.rs` — `scale_output` (window.rs:265-270, `ScaleOutput::draw` of app/renderpasses/scale_output.rs)
//! without GL: the GPU worker hands the window a finished RGBA8 frame of the window's size instead of a float film.  The
//! film, the tone map and the overlays stay on the device (`yk_tone_map_device`, `yk_overlay_draw_device`); the frame is
//! `window.x * window.y * 4` bytes — what the window uploads as a texture and blits 1:1, or writes with `yk_write_png`.
//! `ctx` null runs the library's host instance (bit-identical).  The rule that stands in for GL's textured quad:
//! yuki_amd/csrc/yk_present.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::math::{Spectrum, Vec2};
use std::ffi::{c_void, CString};
use yuki_hip_sys as sys;

/// window.rs:265-270 passes `!self.srgb_backbuffer` as `gamma_before_output`: with an sRGB back buffer (window.rs:94-127,
/// the default off Wayland) the shader writes linear values and the buffer encodes them; without one the shader's own
/// `linearToSRGB` does.  A frame made here is final either way, so the encode names what the screen ends up showing.
pub fn present_encode(srgb_backbuffer: bool) -> u32 {
    if srgb_backbuffer {
        sys::YK_PRESENT_ENCODE_SRGB
    } else {
        sys::YK_PRESENT_ENCODE_SHADER
    }
}

/// Rows top-down, bytes R, G, B, A; the letterbox is the clear colour of window.rs:247.
pub struct Frame {
    pub size: Vec2<u16>,
    pub rgba: Vec<u8>,
}

fn desc(window: Vec2<u16>, srgb_backbuffer: bool) -> sys::yk_present_desc {
    sys::yk_present_desc {
        window_x: window.x,
        window_y: window.y,
        encode: present_encode(srgb_backbuffer),
        format: sys::YK_PRESENT_RGBA8,
    }
}

/// Drop-in for `scale_output(&self.output_scaler, tone_mapped_film, &mut render_target, !self.srgb_backbuffer)` on host
/// pixels (`tone_mapped_film`: row-major, `res.x * res.y`).
pub fn scale_output(
    ctx: *mut sys::yk_context,
    tone_mapped_film: &[Spectrum<f32>],
    res: Vec2<u16>,
    window: Vec2<u16>,
    srgb_backbuffer: bool,
) -> Frame {
    assert!(tone_mapped_film.len() == res.x as usize * res.y as usize);
    let mut rgba = vec![0u8; window.x as usize * window.y as usize * 4];
    let status = unsafe {
        sys::yk_present(
            ctx,
            &desc(window, srgb_backbuffer),
            tone_mapped_film.as_ptr() as *const f32,
            res.x,
            res.y,
            rgba.as_mut_ptr() as *mut c_void,
        )
    };
    assert!(status == sys::YK_OK, "yk_present failed: {}", status);
    Frame { size: window, rgba }
}

/// The GPU worker's last step of a displayed frame, enqueued behind the tone map and the overlays on `stream`:
/// `d_tone_mapped` (the device film after `yk_tone_map_device` / `yk_overlay_draw_device`) -> `d_frame` (a device buffer
/// of `window.x * window.y * 4` bytes, 4-byte aligned, made once per window size).  No synchronisation here: the worker
/// copies `d_frame` to the host on the same stream and waits once per frame.
///
/// # Safety
/// Both pointers are device allocations of the sizes above on `ctx`'s device, and they do not overlap.
pub unsafe fn scale_output_device(
    ctx: *mut sys::yk_context,
    d_tone_mapped: *const c_void,
    res: Vec2<u16>,
    window: Vec2<u16>,
    srgb_backbuffer: bool,
    d_frame: *mut c_void,
    stream: *mut c_void,
) -> Result<(), sys::yk_status> {
    let status = sys::yk_present_device(ctx, &desc(window, srgb_backbuffer), d_tone_mapped, res.x, res.y, d_frame, stream);
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}

/// Where the film lands in the window (for mapping a click back to a film pixel, window.rs's debug ray): top-down.
pub fn target_rect(res: Vec2<u16>, window: Vec2<u16>) -> sys::yk_present_rect {
    let mut r = sys::yk_present_rect::default();
    let status = unsafe { sys::yk_present_target_rect(res.x, res.y, window.x, window.y, &mut r) };
    assert!(status == sys::YK_OK, "yk_present_target_rect failed: {}", status);
    r
}

/// What the window shows, saved: an 8-bit RGBA PNG any viewer opens.
pub fn write_frame_png(path: &std::path::Path, frame: &Frame) -> Result<(), sys::yk_status> {
    let c_path = CString::new(path.to_string_lossy().as_bytes()).map_err(|_| sys::YK_ERR_INVALID_ARGUMENT)?;
    let status = unsafe { sys::yk_write_png(c_path.as_ptr(), frame.size.x as u32, frame.size.y as u32, 4, frame.rgba.as_ptr()) };
    if status == sys::YK_OK {
        Ok(())
    } else {
        Err(status)
    }
}
