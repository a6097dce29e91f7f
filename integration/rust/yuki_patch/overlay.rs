//! `yuki/src/app/window.rs` — `draw_visualizations` (window.rs:1033-1063) without GL: the two `draw` calls
//! (`RayVisualization::draw`, `BvhVisualization::draw`) replaced by one `yk_overlay_draw` on the tone-mapped pixels, so the
//! film the window's "write EXR (mapped)" dumps (window.rs:979-985) carries the overlays on a machine with no display.
//! `ctx` null runs the library's host instance; a `HipDevice`'s context runs it on the GPU (bit-identical).  The rule that
//! stands in for GL's line rasteriser: yuki_amd/csrc/yk_overlay.h.  SOURCE ONLY.
#![cfg(feature = "hip")]

use crate::{
    camera::{CameraParameters, FoV},
    film::FilmSettings,
    integrators::{IntegratorRay, RayType},
    math::Spectrum,
};
use yuki_hip_sys as sys;

/// What `RayVisualization::set_rays` (ray_visualization.rs:28-56) and `BvhVisualization::set_bounds`
/// (bvh_visualization.rs:27-81) keep between frames: the line list and the level whose boxes are shown.
#[derive(Default)]
pub struct Overlays {
    pub lines: Vec<sys::yk_overlay_line>,
    pub bvh_level: Option<i32>,
}

impl Overlays {
    /// window.rs:607: `self.ray_visualization.set_rays(&self.display, &rays)`
    pub fn set_rays(&mut self, rays: &[IntegratorRay]) -> Result<(), sys::yk_status> {
        let records: Vec<sys::yk_integrator_ray> = rays
            .iter()
            .map(|IntegratorRay { ray, ray_type }| sys::yk_integrator_ray {
                o: [ray.o.x, ray.o.y, ray.o.z],
                d: [ray.d.x, ray.d.y, ray.d.z],
                t_max: ray.t_max,
                ray_type: match ray_type {
                    RayType::Direct => 0,
                    RayType::Reflection => 1,
                    RayType::Refraction => 2,
                    RayType::Normal => 3,
                    RayType::Shadow => 4,
                },
            })
            .collect();
        let mut lines = vec![sys::yk_overlay_line::default(); records.len()];
        // More than 32,768 rays: the reference's u16 vertex indices wrap; here it is an error.
        let status = unsafe { sys::yk_overlay_ray_lines(records.as_ptr(), records.len(), lines.as_mut_ptr()) };
        if status != sys::YK_OK {
            return Err(status);
        }
        self.lines = lines;
        Ok(())
    }
    pub fn clear_rays(&mut self) {
        self.lines.clear();
    }
}

fn camera_params(p: CameraParameters, film_settings: FilmSettings) -> sys::yk_camera_params {
    let (fov_axis, fov_degrees) = match p.fov {
        FoV::X(angle) => (0, angle),
        FoV::Y(angle) => (1, angle),
    };
    sys::yk_camera_params {
        position: [p.position.x, p.position.y, p.position.z],
        target: [p.target.x, p.target.y, p.target.z],
        up: [p.up.x, p.up.y, p.up.z],
        fov_axis,
        fov_degrees,
        res_x: film_settings.res.x,
        res_y: film_settings.res.y,
    }
}

/// Drop-in for window.rs:1033-1063 on the pixels `tone_mapped_film` holds (row-major, `film_settings.res`):
/// `draw_visualizations(&mut pixels, &overlays, gpu.scene, active_camera_params, film_settings, gpu.ctx)`.
pub fn draw_visualizations(
    tone_mapped_film: &mut [Spectrum<f32>],
    overlays: &Overlays,
    scene: *const sys::yk_scene,
    active_camera_params: CameraParameters,
    film_settings: FilmSettings,
    ctx: *mut sys::yk_context,
) {
    let res = film_settings.res;
    assert!(tone_mapped_film.len() == res.x as usize * res.y as usize);
    // scene.bvh.bounds(): the root box
    let mut scene_bb = [0.0f32; 6];
    let n = unsafe { sys::yk_scene_node_bounds(scene, 0, scene_bb.as_mut_ptr(), 1) };
    assert!(n == 1, "yk_scene_node_bounds: no root box");
    // `self.scene.bvh.node_bounds(self.bvh_visualization_level)` (window.rs:446)
    let boxes = overlays.bvh_level.map_or(Vec::new(), |level| unsafe {
        let n = sys::yk_scene_node_bounds(scene, level, std::ptr::null_mut(), 0);
        let mut b = vec![0.0f32; 6 * n];
        sys::yk_scene_node_bounds(scene, level, b.as_mut_ptr(), n);
        b
    });
    let params = camera_params(active_camera_params, film_settings);
    let mut world_to_clip = [0.0f32; 16];
    let status = unsafe { sys::yk_overlay_world_to_clip(&params, scene_bb.as_ptr(), world_to_clip.as_mut_ptr()) };
    assert!(status == sys::YK_OK, "yk_overlay_world_to_clip failed: {}", status);
    // ray_visualization.draw(..) then bvh_visualization.draw(..): lines first, then boxes, in one call
    let status = unsafe {
        sys::yk_overlay_draw(
            ctx,
            world_to_clip.as_ptr(),
            if overlays.lines.is_empty() { std::ptr::null() } else { overlays.lines.as_ptr() },
            overlays.lines.len(),
            if boxes.is_empty() { std::ptr::null() } else { boxes.as_ptr() },
            boxes.len() / 6,
            tone_mapped_film.as_mut_ptr() as *mut f32,
            res.x,
            res.y,
        )
    };
    assert!(status == sys::YK_OK, "Ray visualization failed: {}", status);
}
